"""GHMFC without a GPU: the fp64 restatement against the reference's goldens, the parameter container against the reference's
state dict, the host-side validation of drin_ghmfc_* / drin_attention, and the refusals of drin_amd.ghmfc.Model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc import GhmfcConfig, Model, config_from_reference_args
from tests.ghmfc_inputs import CASES, FULL, KEYS, dataset_of, geometry, ghmfc_inputs
from tests.ghmfc_restatement import ghmfc_scores

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def golden_of(name: str):
    case = CASES[name]
    f = "ghmfc_full.npz" if case.get("geom") is FULL else ("ghmfc_shapes.npz" if "geom" in case or name == "b300" else "ghmfc_tiny.npz")
    return np.load(os.path.join(GOLDEN, f))


def cfg_for(name: str) -> GhmfcConfig:
    g = geometry(name)
    return GhmfcConfig(dataset_name=dataset_of(name), num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"],
                       mention_tokens=g["L"], image_regions=g["P"], num_heads=g["H"], entity_tokens=CASES[name].get("T", 0))


def case_model(name: str, precision: str = "bf16x3") -> Model:
    torch.manual_seed(CASES[name]["seed"])
    return Model(cfg_for(name), precision=precision).eval()


def as_tensors(batch, dtype, device="cpu"):
    return [torch.from_numpy(x).to(device, dtype if x.dtype.kind == "f" else torch.int64) if isinstance(x, np.ndarray) else x
            for x in batch]


def compare(got, want, bound: float, what: str) -> float:
    """max |got - want| over every element (NaN exactly where the golden has NaN), printed, asserted <= bound * max|want|."""
    got, want = got.detach().double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs from the golden"
    scale = want[~nan].abs().max().item()
    err = (got[~nan] - want[~nan]).abs().max().item()
    print(f"{what}: max err {err:.3e} (max |ref| {scale:.3e})")
    assert err <= bound * scale, what
    return err


@pytest.mark.parametrize("name", list(CASES))
def test_goldens_hold_no_unexpected_nan(name):
    g = golden_of(name)
    nan = np.isnan(g[f"{name}/scores"])
    if "T" in CASES[name]:   # tokens 1 : ntok - 1 of a 2-token entity are an empty slice: torch.mean gives NaN there, only there
        assert np.array_equal(nan, ghmfc_inputs(name)[6].sum(-1) == 2)
    else:
        assert not nan.any()
    assert not np.isnan(g[f"{name}/mention_repr"]).any()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference_goldens(name):
    """The reference's own fp32-vs-fp64 gap is 1.4e-7 on scores; the bar is 1e-6 * max|ref|."""
    g = golden_of(name)
    model = case_model(name)
    assert list(model.state_dict()) == list(g[f"{name}/keys"])
    sd = {k: v.double() for k, v in model.state_dict().items()}
    with torch.no_grad():
        scores, mention = ghmfc_scores(as_tensors(ghmfc_inputs(name), torch.float64), sd, geometry(name)["H"], return_mention=True)
    compare(scores, g[f"{name}/scores"], 1e-6, f"{name} scores")
    compare(mention, g[f"{name}/mention_repr"], 1e-6, f"{name} mention_repr")


def test_model_draws_the_reference_state_dict():
    g = np.load(os.path.join(GOLDEN, "ghmfc_full.npz"))
    torch.manual_seed(0)
    sd = Model().state_dict()
    assert len(sd) == 52 and list(sd) == list(g["state_dict_seed0/keys"]) == KEYS
    sums = np.array([v.double().sum().item() for v in sd.values()])
    assert np.allclose(sums, g["state_dict_seed0/sums"], rtol=0, atol=1e-9)
    assert [tuple(p.shape) for p in Model().param_list()] == [tuple(v.shape) for v in sd.values()]   # drin_ghmfc_params order


def full_config() -> _lib.DrinGhmfcConfigC:
    return _lib.DrinGhmfcConfigC(batch=64, num_candidates=11, embed_dim=768, image_dim=2048, mention_tokens=128, image_regions=49,
                                 num_heads=8, entity_tokens=0, precision=_lib.PREC_BF16X3, layer_norm_eps=1e-5, cosine_eps=1e-8)


def test_workspace_query_and_validation():
    lib = _lib.load()
    c = full_config()
    b64 = lib.drin_ghmfc_workspace_bytes(C.byref(c))
    assert b64 > 0
    c.batch = 256
    b256 = lib.drin_ghmfc_workspace_bytes(C.byref(c))
    c.batch = 4096
    assert lib.drin_ghmfc_workspace_bytes(C.byref(c)) == b256 > b64      # one chunk of 256 mentions, whatever B
    c.entity_tokens = 64
    assert lib.drin_ghmfc_workspace_bytes(C.byref(c)) > b256             # the pooled token blocks
    for field, value, text in (("embed_dim", 772, b"divisible by num_heads"), ("num_heads", 2, b"head dims"),
                               ("mention_tokens", 513, b"<= 512"), ("image_regions", 513, b"<= 512"),
                               ("image_dim", 2050, b"multiples of 4"), ("precision", 3, b"precision"), ("batch", 0, b"batch")):
        c = full_config()
        setattr(c, field, value)
        assert lib.drin_ghmfc_workspace_bytes(C.byref(c)) == 0, field
        assert text in lib.drin_last_error(), (field, lib.drin_last_error())
    assert lib.drin_ghmfc_workspace_bytes(None) == 0


def test_entry_points_validate_on_host():
    lib = _lib.load()
    one = C.c_void_p(16)   # never dereferenced: every check below fails before a launch
    c = full_config()
    b, p = _lib.DrinGhmfcBatchC(), _lib.DrinGhmfcParamsC()
    assert lib.drin_ghmfc_forward(C.byref(c), C.byref(b), C.byref(p), one, 1 << 40, one, None, None) == _lib.E_NULL
    assert lib.drin_ghmfc_forward(C.byref(c), None, C.byref(p), one, 1 << 40, one, None, None) == _lib.E_NULL
    c.embed_dim = 772
    assert lib.drin_ghmfc_forward(C.byref(c), C.byref(b), C.byref(p), one, 1 << 40, one, None, None) == _lib.E_SHAPE
    att = lambda q, Lk, dh: lib.drin_attention(q, 64, one, 64, one, 64, None, one, 64, 2, 4, 7, Lk, dh, None)   # noqa: E731
    assert att(one, 513, 16) == _lib.E_SHAPE and b"k_len" in lib.drin_last_error()
    assert att(one, 0, 16) == _lib.E_SHAPE
    assert att(one, 8, 257) == _lib.E_SHAPE
    assert att(None, 8, 16) == _lib.E_NULL


def test_model_refuses_training_mode_and_cpu_tensors():
    model = case_model("wd_b1")
    batch = as_tensors(ghmfc_inputs("wd_b1"), torch.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        model(batch)
    model.train()
    with pytest.raises(RuntimeError, match=r"scoring only: call \.eval\(\); GHMFC training is not implemented, DESIGN.md §11"):
        model(batch)
    with pytest.raises(RuntimeError, match="scoring only"):
        model.encode_mentions(batch)


def test_config_from_reference_args_refuses_other_variants():
    class Args:
        dataset_name, num_candidates_model, bert_embed_dim, resnet_embed_dim = "wikimel", 101, 768, 2048
        max_mention_sentence_len, resnet_num_region, transformer_num_heads, max_entity_attr_token_len = 128, 49, 8, 64
        mention_final_layer_name, mention_multimodal_attention, multimodal_subspace_activation = "multimodal", "bi", "gelu"
        entity_final_layer_name, entity_final_pooling, online_bert = "linear", "avg", False
    cfg = config_from_reference_args(Args)
    assert (cfg.dataset_name, cfg.num_candidates, cfg.num_heads, cfg.entity_tokens) == ("wikimel", 101, 8, 64)
    Args.mention_multimodal_attention = "text"
    with pytest.raises(NotImplementedError, match="mention_multimodal_attention"):
        config_from_reference_args(Args)
