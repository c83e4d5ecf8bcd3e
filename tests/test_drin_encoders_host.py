"""DRIN's other mention encoders without a GPU: EncoderModel's keys and initial draw against the
reference's goldens, the fp64 restatement against the goldens, `config_from_reference_args` on fake `args` objects, the default
model untouched, `reference_shim.Model()`'s dispatch, and the refusals of what is not built."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from drin_amd.config import DrinConfig, config_from_reference_args
from drin_amd.drin_encoders import EncoderModel
from drin_amd.model import IndexedBatch, Model
from drin_amd.train import GradBucket, LibraryAdam, MELRunner, OverlappedStep, make_adam
from tests.drin_encoder_inputs import CASES, EMPTY_SPAN_CASE, EMPTY_SPAN_ROW, GOLDEN_FILE, SMALL, encoder_inputs, transformer_keys
from tests.drin_encoder_restatement import encoder_forward
from tests.test_ghmfc_host import compare

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_file = {}


def golden(name: str, what: str):
    if "f" not in _file:
        _file["f"] = np.load(os.path.join(GOLDEN, GOLDEN_FILE))
    return _file["f"][f"{name}/{what}"]


def case_model(name: str, precision: str = "bf16x3", dropout=None, seed: int = 0, core: str = "fma", fused: bool = True):
    cfg, _B, _d, wseed = CASES[name]
    if dropout is not None:
        cfg = cfg.with_(transformer_dropout=dropout)
    torch.manual_seed(wseed)
    return Model(cfg, precision=precision, core=core, seed=seed, fused=fused)


@pytest.mark.parametrize("name", list(CASES))
def test_keys_and_initial_draw_are_the_references(name):
    model = case_model(name)
    cfg = CASES[name][0]
    sd = model.state_dict()
    assert type(model) is EncoderModel
    assert list(sd) == list(golden(name, "keys"))
    if cfg.mention_final_layer_name == "transformer":
        assert list(sd)[:12 * cfg.transformer_num_layers] == transformer_keys(cfg.transformer_num_layers)
    else:
        assert len(sd) == 22                                               # "none": no mention-text parameter at all
    sums = np.array([v.double().sum().item() for v in sd.values()])
    assert np.allclose(sums, golden(name, "w_sums"), rtol=0, atol=1e-9 * max(1.0, np.abs(sums).max()))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_goldens(name):
    """An EncoderModel state dict in the fp64 restatement gives the reference's scores, layer-0 vertices and layer-0 edges to 1e-6
    of max|ref| (the bar of tests/test_ghmfc_variants_host.py: the reference ran in fp32), NaN rows at the same places."""
    cfg = CASES[name][0]
    sd = {k: v.double() for k, v in case_model(name).state_dict().items()}
    batch = [t.double() if t.is_floating_point() else t for t in encoder_inputs(name)[:14]]
    trace = {}
    with torch.no_grad():
        scores = encoder_forward(sd, batch, cfg, trace=trace)
    if name == EMPTY_SPAN_CASE:
        assert torch.isnan(scores[EMPTY_SPAN_ROW]).all()
    compare(scores, golden(name, "scores"), 1e-6, f"{name} restatement scores")
    for key, v in zip(("mt0", "mi0", "et0", "ei0"), trace["vertex0"]):
        compare(v, golden(name, key), 1e-6, f"{name} restatement {key}")
    edges = torch.stack([e[..., 0] if cfg.gcn_edge_feature == "vector" else e for e in trace["edge0"]])
    compare(edges, golden(name, "edges0"), 1e-6, f"{name} restatement edges0")


def test_default_configuration_is_the_untouched_linear_model():
    torch.manual_seed(0)
    model = Model()
    assert type(model) is Model and len(list(model.parameters())) == 24 and model.flat_buckets
    assert list(model.state_dict())[:2] == ["vertex_encoder.mention_text_encoder.final_layer.linear.weight",
                                            "vertex_encoder.mention_text_encoder.final_layer.linear.bias"]
    cfg = DrinConfig()
    assert (cfg.mention_final_layer_name, cfg.mention_final_representation) == ("linear", "avg extract")
    assert (cfg.transformer_num_layers, cfg.transformer_num_heads, cfg.transformer_ffn_hidden_size, cfg.transformer_ffn_activation,
            cfg.transformer_dropout) == (8, 8, 512, "gelu", 0.1)           # args.py:60-64
    with pytest.raises(ValueError, match="linear one is drin_amd.model.Model"):
        EncoderModel(cfg)


def fake_args(**over):
    a = types.SimpleNamespace(model_type="drin", dataset_name="wikidiverse", num_candidates_data=10, num_candidates_model=11)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_config_from_reference_args_reads_the_encoder_names():
    cfg = config_from_reference_args(fake_args())
    assert cfg.linear_mention_encoder and cfg.mention_final_representation == "avg extract"
    over = dict(mention_final_layer_name="transformer", mention_final_representation="max pool", transformer_num_layers=3,
                transformer_num_heads=4, transformer_ffn_hidden_size=64, transformer_ffn_activation="relu", transformer_dropout=0.2)
    cfg = config_from_reference_args(fake_args(**over))
    assert all(getattr(cfg, k) == v for k, v in over.items()) and not cfg.linear_mention_encoder
    for name in ("none", "transformer"):
        for rep in ("avg extract", "max pool"):
            cfg = config_from_reference_args(fake_args(mention_final_layer_name=name, mention_final_representation=rep))
            assert (cfg.mention_final_layer_name, cfg.mention_final_representation) == (name, rep)
    with pytest.raises(NotImplementedError, match=r"args\.py:12-13.*DESIGN\.md section 22"):
        config_from_reference_args(fake_args(mention_final_layer_name="linear", mention_final_representation="max pool"))
    with pytest.raises(NotImplementedError, match=r"args\.py:12-13"):           # "linear" is args.py:28's default
        config_from_reference_args(fake_args(mention_final_representation="max pool"))
    by_hand = DrinConfig(mention_final_representation="max pool")               # the one refusal is the reader's: validate() passes,
    by_hand.validate()                                                          # and the linear model never reads the name
    assert type(Model(by_hand)) is Model
    with pytest.raises(ValueError, match="unknown mention_final_layer_name 'multimodal'"):
        config_from_reference_args(fake_args(mention_final_layer_name="multimodal"))
    with pytest.raises(ValueError, match="unknown mention_final_representation"):
        config_from_reference_args(fake_args(mention_final_layer_name="none", mention_final_representation="cls"))
    with pytest.raises(NotImplementedError, match="transformer_ffn_activation"):
        config_from_reference_args(fake_args(mention_final_layer_name="transformer", transformer_ffn_activation="silu"))
    with pytest.raises(NotImplementedError, match="entity_final_layer_name"):
        config_from_reference_args(fake_args(entity_final_layer_name="none"))


@pytest.mark.parametrize("layer", ["transformer", "none"])
@pytest.mark.parametrize("rep", ["avg extract", "max pool"])
def test_reference_shim_returns_the_right_class(monkeypatch, layer, rep):
    args = types.ModuleType("common.args")
    vals = dict(model_type="drin", dataset_name="wikidiverse", num_candidates_data=2, num_candidates_model=3, bert_embed_dim=16,
                gcn_embed_dim=16, resnet_embed_dim=8, max_mention_sentence_len=5, resnet_num_region=2, mention_final_layer_name=layer,
                mention_final_representation=rep, transformer_num_layers=2, transformer_num_heads=2, transformer_ffn_hidden_size=32)
    for k, v in vals.items():
        setattr(args, k, v)
    common = types.ModuleType("common")
    common.args = args
    monkeypatch.setitem(sys.modules, "common", common)
    monkeypatch.setitem(sys.modules, "common.args", args)
    from drin_amd import reference_shim
    torch.manual_seed(4 if layer == "transformer" else 2)
    model = reference_shim.Model()
    assert type(model) is EncoderModel and model.cfg.mention_final_representation == rep
    name = {"transformer": "tr_max", "none": "none_max"}[layer]          # the keys do not depend on the representation
    assert list(model.state_dict()) == list(golden(name, "keys"))
    args.mention_final_layer_name, args.mention_final_representation = "linear", "avg extract"
    linear = reference_shim.Model()
    assert type(linear) is reference_shim.Model and len(linear.state_dict()) == 24
    args.mention_final_representation = "max pool"
    with pytest.raises(NotImplementedError, match="args.py:12-13"):
        reference_shim.Model()


def test_a_reference_keyed_state_dict_round_trips():
    a, b = case_model("tr_max"), case_model("tr_avg")
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    assert list(sd) == list(golden("tr_max", "keys"))
    b.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in b.state_dict().items())
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        case_model("none_max").load_state_dict(sd)


def test_what_is_not_built_is_refused():
    model = case_model("tr_max")
    for call in (model.bucket_layout, model.flatten_parameters, model.grad_bucket):
        with pytest.raises(NotImplementedError, match="DESIGN.md section 22"):
            call()
    with pytest.raises(NotImplementedError, match="IndexedBatch.*DESIGN.md section 22"):
        model(IndexedBatch([torch.zeros(1)] * 7, None, torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3), torch.zeros(1, 3)))
    with pytest.raises(NotImplementedError, match="DESIGN.md section 22"):
        LibraryAdam(model)
    opt = make_adam(model, 1e-3)
    assert isinstance(opt, torch.optim.Adam) and not model.flat_buckets and not model.grad_bucket_enabled
    plain = GradBucket(list(model.parameters()))                       # the serial bucket is fine
    with pytest.raises(NotImplementedError, match="OverlappedStep.*DESIGN.md section 22"):
        OverlappedStep(model, plain, opt)
    with pytest.raises(NotImplementedError, match=r"GradBucket\(overlap=True\).*DESIGN.md section 22"):
        GradBucket(list(model.parameters()), overlap=True, model=model)
    assert model._layers_ready_hook is None                            # the refused bucket installed nothing
    for mode in ("forward", "backward", "both"):
        with pytest.raises(ValueError, match="overlap_allreduce needs"):
            MELRunner(model.cfg.with_(metrics_topk=(1,)), model, "cpu", overlap_allreduce=mode)
    with pytest.raises(NotImplementedError, match="folded path"):
        Model(CASES["tr_max"][0], precision="bf16x3_if16")
    with pytest.raises(RuntimeError, match="parameters only"):
        model.vertex_encoder.mention_text_encoder.intermediate_layer(torch.zeros(1, 5, 16))
    with pytest.raises(RuntimeError, match="AMD GPU only"):             # no CPU fallback, in either mode
        model.eval()(encoder_inputs("tr_max")[:14])
