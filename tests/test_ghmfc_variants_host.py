"""GHMFC's other mention encoders without a GPU: VariantModel's keys and initial draw against the reference's goldens, the fp64
restatement against the goldens and against torch's own nn.TransformerEncoder, the configuration's forcing rule and refusals,
the shim's dispatch and its loaders, the host-side validation of drin_act_dropout_* / drin_span_mean_*, and the row draws of a
DropoutStream."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

from drin_amd import _lib
from drin_amd.attention import DropoutStream, dropout_keep
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantConfig, VariantModel, variant_config_from_reference_args
from tests.ghmfc_variant_inputs import (CASES, EMPTY_SPAN_ROW, GOLDEN_FILE, TINY, TRANSFORMER, case_keys, case_of, dataset_of, geometry,
                                        keys_for, reference_names, variant_inputs)
from tests.ghmfc_variant_restatement import transformer_encoder, variant_scores
from tests.test_ghmfc_host import as_tensors, compare

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONE = C.c_void_p(16)    # 16-byte aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)
COMBINATIONS = [("transformer", "max"), ("transformer", "avg"), ("text", "max"), ("text", "avg"), ("linear", "avg"), ("none", "max"),
                ("none", "avg")]
_files = {}


def golden(name: str, what: str):
    fname = GOLDEN_FILE.get(name, "ghmfc_variants_full.npz")
    if fname not in _files:
        _files[fname] = np.load(os.path.join(GOLDEN, fname))
    return _files[fname][f"{name}/{what}"]


def encoder_names(enc: str, rep: str) -> dict:
    return dict(mention_final_layer_name="multimodal" if enc == "text" else enc, mention_multimodal_attention="text" if enc == "text" else "bi",
                mention_final_representation="max pool" if rep == "max" else "avg extract")


def variant_cfg(name: str) -> VariantConfig:
    g, names = geometry(name), reference_names(name)
    return VariantConfig(dataset_name=dataset_of(name), num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"],
                         image_regions=g["P"], num_heads=g["H"], entity_tokens=case_of(name).get("T", 0),
                         transformer_num_layers=g["layers"], transformer_ffn_hidden_size=g["ffn"], **names)


def case_model(name: str, precision: str = "bf16x3", dropout: float = 0.0, seed: int = 0) -> VariantModel:
    torch.manual_seed(case_of(name)["seed"])
    return VariantModel(variant_cfg(name), precision=precision, dropout=dropout, seed=seed)


def restatement_args(name: str) -> dict:
    case, g = case_of(name), geometry(name)
    return dict(enc=case["enc"], rep=case["repr"], heads=g["H"], layers=g["layers"], act=case.get("act", "gelu"))


@pytest.mark.parametrize("enc,rep", COMBINATIONS)
def test_keys_and_initial_draw_of_every_combination(enc, rep):
    torch.manual_seed(0)
    model = VariantModel(VariantConfig(num_candidates=TINY["N"], embed_dim=TINY["D"], image_dim=TINY["R"], mention_tokens=TINY["L"],
                                       image_regions=TINY["P"], num_heads=TINY["H"], transformer_num_layers=TINY["layers"],
                                       transformer_ffn_hidden_size=TINY["ffn"], **encoder_names(enc, rep)))
    sd = model.state_dict()
    assert isinstance(model, VariantModel) and len(sd) == {"transformer": 26, "text": 24, "linear": 4, "none": 2}[enc]
    assert list(sd) == list(golden("state_dict_seed0", f"{enc}_{rep}/keys")) == keys_for(enc, TINY["layers"])
    sums = np.array([v.double().sum().item() for v in sd.values()])
    assert np.allclose(sums, golden("state_dict_seed0", f"{enc}_{rep}/sums"), rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", list(CASES))
def test_case_weights_are_the_references(name):
    sd = case_model(name).state_dict()
    assert list(sd) == list(golden(name, "keys")) == case_keys(name)
    sums = np.array([v.double().sum().item() for v in sd.values()])
    assert np.allclose(sums, golden(name, "w_sums"), rtol=0, atol=1e-9 * max(1.0, np.abs(sums).max()))


def test_the_eight_transformer_layers_start_equal():
    torch.manual_seed(5)
    model = VariantModel(VariantConfig(num_candidates=4, embed_dim=16, image_dim=32, mention_tokens=12, image_regions=3, num_heads=2,
                                       mention_final_layer_name="transformer", transformer_ffn_hidden_size=24))
    layers = model.mention_encoder.intermediate_layer.transformer.layers
    first = layers[0].state_dict()
    assert len(layers) == 8 and len(first) == 12 and len(model.state_dict()) == 8 * 12 + 2
    assert all(torch.equal(v, first[k]) for layer in layers[1:] for k, v in layer.state_dict().items())
    assert not torch.equal(first["linear1.weight"], torch.zeros_like(first["linear1.weight"]))
    with pytest.raises(RuntimeError, match="parameters only"):
        model.mention_encoder.intermediate_layer(torch.zeros(1, 12, 16))
    with pytest.raises(RuntimeError, match="GPU only"):               # CPU tensors are refused in both modes
        model.train()(as_tensors(variant_inputs("tr_max_b3"), torch.float32))
    with pytest.raises(RuntimeError, match="GPU only"):
        model.eval()(as_tensors(variant_inputs("tr_max_b3"), torch.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_goldens(name):
    """A VariantModel state dict loads into the fp64 restatement, which gives the reference's scores and mention representations
    to 1e-6 of max|ref| (the reference ran in fp32: 4.5e-8 from fp64 at the full widths), NaN rows at the same places."""
    sd = {k: v.double() for k, v in case_model(name).state_dict().items()}
    batch = as_tensors(variant_inputs(name), torch.float64)
    with torch.no_grad():
        scores, mention, _pre = variant_scores(batch, sd, **restatement_args(name), return_pre=True)
    if case_of(name)["spans"] == "forms":
        assert torch.isnan(scores[EMPTY_SPAN_ROW]).all() and torch.isnan(mention[EMPTY_SPAN_ROW]).all()
    compare(scores, golden(name, "scores"), 1e-6, f"{name} restatement scores")
    compare(mention, golden(name, "mention_repr"), 1e-6, f"{name} restatement mention_repr")


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_restatement_matches_torchs_transformer_encoder_in_float64(act):
    """eval mode with autograd enabled (torch's plain path, not its fused inference one): output and every parameter gradient
    within 1e-10."""
    D, H, F, layers, B, L = 16, 2, 24, 3, 4, 12
    torch.manual_seed(11)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(D, H, F, 0.1, act, batch_first=True), layers, enable_nested_tensor=False)
    enc = enc.double().eval()
    with torch.no_grad():
        for p in enc.parameters():                                    # (the layers start as copies and the biases at zero)
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(B, L, D, dtype=torch.float64)
    keep = torch.arange(L)[None, :] < torch.tensor([1, L, 5, 9])[:, None]
    G = torch.randn(B, L, D, dtype=torch.float64)
    want = enc(x, src_key_padding_mask=~keep)
    (want * G).sum().backward()
    sd = {TRANSFORMER + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    got = transformer_encoder(sd, x, keep, H, layers, act)
    grads = torch.autograd.grad((got * G).sum(), list(sd.values()))
    assert (got - want).abs().max().item() <= 1e-10 * want.abs().max().item()
    for (k, p), g in zip(enc.named_parameters(), grads):
        assert (g - p.grad).abs().max().item() <= 1e-10 * max(p.grad.abs().max().item(), 1.0), k


def reference_args(**over):
    args = types.ModuleType("common.args")
    vals = dict(dataset_name="wikidiverse", num_candidates_model=4, bert_embed_dim=16, resnet_embed_dim=32, max_mention_sentence_len=12,
                resnet_num_region=3, transformer_num_heads=2, transformer_dropout=0.3, seed=5, transformer_num_layers=2,
                transformer_ffn_hidden_size=24, preprocess_dir="", batch_size=2, dataloader_workers=0)
    vals.update(over)
    for k, v in vals.items():
        setattr(args, k, v)
    return args


def test_forcing_rule_and_refusals():
    cfg = variant_config_from_reference_args(reference_args(mention_final_layer_name="linear", mention_final_representation="max pool"))
    assert cfg.mention_final_representation == "avg extract" and not cfg.reads_mention_image and not cfg.is_default
    cfg = variant_config_from_reference_args(reference_args(mention_final_representation="avg extract"))
    assert cfg.is_default and cfg.mention_final_representation == "max pool" and cfg.reads_mention_image
    cfg = variant_config_from_reference_args(reference_args(mention_multimodal_attention="text", mention_final_representation="avg extract"))
    assert cfg.mention_final_representation == "avg extract" and cfg.reads_mention_image and not cfg.is_default
    cfg = variant_config_from_reference_args(reference_args(mention_final_layer_name="transformer", transformer_ffn_activation="relu"))
    assert (cfg.transformer_num_layers, cfg.transformer_ffn_hidden_size, cfg.transformer_ffn_activation) == (2, 24, "relu")
    assert VariantConfig().transformer_num_layers == 8 and VariantConfig().transformer_ffn_hidden_size == 512
    for name, value in (("online_bert", True), ("entity_final_layer_name", "none"), ("entity_final_pooling", "max"),
                        ("mention_final_output_dim", 32), ("entity_final_output_dim", 32)):
        with pytest.raises(NotImplementedError, match=name):
            variant_config_from_reference_args(reference_args(mention_final_layer_name="transformer", **{name: value}))
    with pytest.raises(NotImplementedError, match="multimodal_subspace_activation"):
        variant_config_from_reference_args(reference_args(multimodal_subspace_activation="relu"))
    for name in ("mention_final_layer_name", "mention_multimodal_attention", "mention_final_representation", "transformer_ffn_activation"):
        with pytest.raises(ValueError, match=name):
            VariantConfig(**{name: "other"})
    with pytest.raises(ValueError, match="multiple of 4"):
        VariantConfig(mention_final_layer_name="transformer", transformer_ffn_hidden_size=26)
    assert isinstance(VariantModel(VariantConfig(num_candidates=4, embed_dim=16, image_dim=32, mention_tokens=12, image_regions=3,
                                                 num_heads=2)), TrainableModel)
    with pytest.raises(ValueError, match="dropout"):
        VariantModel(VariantConfig(mention_final_layer_name="none"), dropout=1.0)


def bind(monkeypatch, args):
    common = types.ModuleType("common")
    common.args = args
    monkeypatch.setitem(sys.modules, "common", common)
    monkeypatch.setitem(sys.modules, "common.args", args)
    from drin_amd import ghmfc_shim
    return ghmfc_shim


def test_shim_dispatches_on_the_mention_encoder(monkeypatch):
    shim = bind(monkeypatch, reference_args())
    m = shim.Model()
    assert isinstance(m, TrainableModel) and isinstance(m, shim.Model) and len(m.state_dict()) == 52 and m.dropout == 0.3
    shim = bind(monkeypatch, reference_args(mention_final_layer_name="transformer", mention_final_representation="avg extract"))
    m = shim.Model()
    assert isinstance(m, VariantModel) and not isinstance(m, TrainableModel) and len(m.state_dict()) == 26
    assert m.dropout == 0.3 and m.dropout_stream.seed == 5 and m.cfg.mention_final_representation == "avg extract"
    assert m.mention_encoder.intermediate_layer.transformer.layers[0].dropout.p == 0.3
    shim = bind(monkeypatch, reference_args(mention_multimodal_attention="text"))
    m = shim.Model()
    assert isinstance(m, VariantModel) and len(m.state_dict()) == 24
    ca = m.mention_encoder.intermediate_layer
    assert ca.a2b_attention.dropout_stream is m.dropout_stream and ca.b2a_attention.dropout_stream is m.dropout_stream
    shim = bind(monkeypatch, reference_args(online_bert=True))
    with pytest.raises(NotImplementedError, match="online_bert"):
        shim.Model()


@pytest.mark.parametrize("layer", ["multimodal", "transformer"])
def test_loaders_open_the_mention_image_file_only_for_multimodal(monkeypatch, tmp_path, layer):
    n, N, D, L = 3, 4, 16, 12
    rng = np.random.default_rng(0)
    for split in ("train", "valid", "test"):
        np.save(tmp_path / f"mention-text-feature_{split}.npy", rng.standard_normal((n, L, D)).astype(np.float32))
        np.save(tmp_path / f"mention-text-mask_{split}.npy", np.ones((n, L), dtype=np.int64))
        np.save(tmp_path / f"entity-attr-feature_{split}.npy", rng.standard_normal((n * N, D)).astype(np.float32))
        np.save(tmp_path / f"start-pos_{split}.npy", np.zeros(n, dtype=np.int64))
        np.save(tmp_path / f"end-pos_{split}.npy", np.ones(n, dtype=np.int64))
        np.save(tmp_path / f"answer_{split}.npy", np.zeros(n, dtype=np.int64))
        if layer == "multimodal":
            np.save(tmp_path / f"mention-image-feature_{split}.npy", rng.standard_normal((n, 3, 32)).astype(np.float32))
    shim = bind(monkeypatch, reference_args(mention_final_layer_name=layer, preprocess_dir=str(tmp_path), shuffle_train_data=False))
    opened = []
    real_load = np.load
    monkeypatch.setattr(np, "load", lambda path, *a, **k: (opened.append(os.path.basename(str(path))), real_load(path, *a, **k))[1])
    loaders = shim.create_datasets()
    assert len(loaders) == 3 and any(f.startswith("mention-image-feature") for f in opened) == (layer == "multimodal")
    batch = next(iter(loaders[0]))
    assert len(batch) == 9 and tuple(batch[0].shape) == (2, L, D) and batch[2].tolist() == [1, 1] and batch[3].tolist() == [2, 2]
    if layer == "multimodal":
        assert tuple(batch[4].shape) == (2, 3, 32)
    else:
        assert batch[4].tolist() == [0, 0]                             # the loader's 0, collated


def test_act_dropout_and_span_mean_entry_points_validate_on_host():
    lib = _lib.load()

    def act_fwd(x=ONE, y=ONE, rows=3, E=16, act=2, p=0.1):
        return lib.drin_act_dropout_fwd(x, y, rows, E, act, p, 1, 2, None)

    def act_bwd(x=ONE, y=ONE, rows=3, E=16, act=2, p=0.1, dy=ONE):
        return lib.drin_act_dropout_bwd(x, dy, y, rows, E, act, p, 1, 2, None)

    def span_fwd(x=ONE, y=ONE, rows=3, E=16, start=ONE, end=ONE, L=5):
        return lib.drin_span_mean_fwd(x, start, end, y, rows, L, E, None)

    def span_bwd(x=ONE, y=ONE, rows=3, E=16, start=ONE, end=ONE, L=5):
        return lib.drin_span_mean_bwd(x, start, end, y, rows, L, E, None)

    for call in (act_fwd, act_bwd, span_fwd, span_bwd):
        assert call(x=None) == _lib.E_NULL and b"NULL" in lib.drin_last_error(), call.__name__
        assert call(y=None) == _lib.E_NULL, call.__name__
        assert call(x=ODD) == _lib.E_ALIGN and call(y=ODD) == _lib.E_ALIGN, call.__name__
        assert call(E=6) == _lib.E_SHAPE and b"multiple of 4" in lib.drin_last_error(), call.__name__
        assert call(E=0) == _lib.E_SHAPE and call(rows=0) == _lib.E_SHAPE, call.__name__
        assert b"drin_" + call.__name__.replace("act", "act_dropout").replace("span", "span_mean").encode() in lib.drin_last_error()
    for call in (act_fwd, act_bwd):
        for p in (1.0, -0.1, float("nan")):
            assert call(p=p) == _lib.E_SHAPE and b"[0, 1)" in lib.drin_last_error(), (call.__name__, p)
        for act in (-1, 3, 5):
            assert call(act=act) == _lib.E_SHAPE and b"act" in lib.drin_last_error(), (call.__name__, act)
        assert call(rows=1 << 62) == _lib.E_SHAPE
    assert act_bwd(dy=None) == _lib.E_NULL and act_bwd(dy=ODD) == _lib.E_ALIGN
    assert act_bwd(x=None, act=0, y=None) == _lib.E_NULL               # plain dropout needs no x: the next check is dx
    assert b"dx" in lib.drin_last_error()
    for call in (span_fwd, span_bwd):
        assert call(start=None) == _lib.E_NULL and call(end=None) == _lib.E_NULL and call(L=0) == _lib.E_SHAPE, call.__name__
    assert _lib.ROW_ACT == {"none": 0, "relu": 1, "gelu": 2}
    assert lib.drin_version() == _lib.ABI_VERSION == 12 and _lib.KERNEL_CLASSES == 12   # additive under ABI 12


def test_row_draws_are_logged_and_keep_their_share():
    stream = DropoutStream(seed=9)
    assert [stream.draw(2, 4, 5, 7), stream.draw_rows(1536, 512), stream.draw_rows(3, 16)] == [0, 1, 2]
    assert stream.log == [(0, 2, 4, 5, 7), (1, 1536, 1, 1, 512), (2, 3, 1, 1, 16)] and stream.counter == 3
    for p in (0.1, 0.5):
        call, rows, one, one_, width = stream.log[1]
        keep = dropout_keep(stream.seed, call, rows, one, one_, width, p)
        n = rows * width
        share = keep.double().mean().item()
        print(f"p = {p}: kept share {share:.6f} of {n}")
        assert tuple(keep.shape) == (rows, 1, 1, width) and abs(share - (1 - p)) <= 3 * math.sqrt(p * (1 - p) / n)
    # the flat index alone decides: row r, column c is element r * width + c of the attention geometry too
    assert torch.equal(dropout_keep(9, 1, 1536, 1, 1, 512, 0.1).flatten(), dropout_keep(9, 1, 4, 8, 48, 512, 0.1).flatten())
