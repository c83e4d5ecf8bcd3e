"""GHMFC's entity encoder settings (`entity_final_pooling = "max"`, `entity_final_layer_name = "none"`) without a GPU: the models'
keys and initial draw against the reference's goldens (52 keys, or 50 without the entity Linear), the fp64 restatement against the
golden scores and entity encoder outputs, the configuration's validation, the reference binding and the shim's dispatch, and the
host-side argument checks of drin_entity_token_pool, drin_entity_token_pool_indexed and drin_ghmfc_entity_rows_ex."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

from drin_amd import _lib, ghmfc
from drin_amd.ghmfc import GhmfcConfig, Model, config_from_reference_args, entity_settings_from_reference_args
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantConfig, VariantModel, variant_config_from_reference_args
from tests.ghmfc_entity_inputs import CASES, GOLDEN_FILE, TINY_CASES, case_keys, dataset_of, entity_inputs, geometry, reference_names
from tests.ghmfc_entity_restatement import entity_case_scores
from tests.test_ghmfc_host import as_tensors, compare
from tests.test_ghmfc_variants_host import bind, reference_args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
NEW_INT = ("drin_entity_token_pool", "drin_entity_token_pool_indexed", "drin_ghmfc_entity_rows_ex")
ONE = C.c_void_p(16)      # aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)      # 4-byte aligned only
BIG = 1 << 40
_golden = {}


def golden(name: str, what: str):
    if not _golden:
        _golden["file"] = np.load(os.path.join(REPO, "tests", "golden", GOLDEN_FILE))
    return _golden["file"][f"{name}/{what}"]


def last():
    return _lib.load().drin_last_error().decode()


def entity_cfg(name: str) -> VariantConfig:
    g, names = geometry(name), reference_names(name)
    return VariantConfig(dataset_name=dataset_of(name), num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"],
                         image_regions=g["P"], num_heads=g["H"], entity_tokens=CASES[name].get("T", 0), transformer_num_layers=g["layers"],
                         transformer_ffn_hidden_size=g["ffn"], **names)


def entity_case_model(name: str, precision: str = "bf16x3", dropout: float = 0.0, seed: int = 0):
    """the case's model under its weight seed: a TrainableModel for the default mention encoder, else a VariantModel"""
    torch.manual_seed(CASES[name]["seed"])
    return VariantModel(entity_cfg(name), precision=precision, dropout=dropout, seed=seed)


def restated(name: str, sd, batch):
    case = CASES[name]
    return entity_case_scores(batch, sd, case["enc"], case["repr"], case["pooling"], geometry(name)["H"])


@pytest.mark.parametrize("name", list(CASES))
def test_keys_and_initial_draw_are_the_references(name):
    model = entity_case_model(name)
    assert isinstance(model, TrainableModel) == (CASES[name]["enc"] == "bi")
    sd = model.state_dict()
    assert list(sd) == list(golden(name, "keys")) == case_keys(name)
    if CASES[name]["enc"] == "bi":
        assert len(sd) == (52 if CASES[name]["layer"] == "linear" else 50) == len(model.param_list())
    identity = isinstance(model.entity_encoder.final_layer, nn.Identity)
    assert identity == (CASES[name]["layer"] == "none") and identity == (not any(k.startswith("entity_encoder") for k in sd))
    sums = np.array([v.double().sum().item() for v in sd.values()])
    assert np.allclose(sums, golden(name, "w_sums"), rtol=0, atol=1e-9 * max(1.0, np.abs(sums).max(initial=0.0)))


def test_the_parameterless_model_has_nothing_to_train():
    model = entity_case_model("wm_bare_max_none")
    assert list(model.parameters()) == [] and len(model.state_dict()) == 0
    assert ghmfc.model_device(model).type == "cpu" and ghmfc.model_device(model, None, torch.zeros(1)).type == "cpu"
    with pytest.raises(RuntimeError, match="GPU only"):               # found through the batch: a CPU batch is refused
        model.eval()(as_tensors(entity_inputs("wm_bare_max_none"), torch.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_goldens(name):
    """The model's state dict in the fp64 restatement gives the reference's scores and representations to 1e-6 of max|ref| (the
    reference ran in fp32); a max over fp32 values rounds nothing, so with an Identity final layer it is the golden's, exactly."""
    sd = {k: v.double() for k, v in entity_case_model(name).state_dict().items()}
    batch = as_tensors(entity_inputs(name), torch.float64)
    with torch.no_grad():
        scores, mention, entity = restated(name, sd, batch)
    compare(scores, golden(name, "scores"), 1e-6, f"{name} restatement scores")
    compare(mention, golden(name, "mention_repr"), 1e-6, f"{name} restatement mention_repr")
    if name in TINY_CASES:
        compare(entity, golden(name, "entity_repr"), 1e-6, f"{name} restatement entity_repr")
        if CASES[name]["pooling"] == "max" and CASES[name]["layer"] == "none":
            assert torch.equal(entity.float(), torch.from_numpy(golden(name, "entity_repr")))


def test_config_validation():
    cfg = GhmfcConfig()
    assert (cfg.entity_final_layer_name, cfg.entity_final_pooling) == ("linear", "avg") and cfg.entity_default
    assert not GhmfcConfig(entity_final_pooling="max").entity_default and not GhmfcConfig(entity_final_layer_name="none").entity_default
    with pytest.raises(ValueError, match="entity_final_layer_name"):
        GhmfcConfig(entity_final_layer_name="transformer")
    with pytest.raises(ValueError, match="entity_final_pooling.*bert default"):
        GhmfcConfig(entity_final_pooling="bert default")
    with pytest.raises(ValueError, match="entity_final_pooling"):
        VariantConfig(mention_final_layer_name="none", entity_final_pooling="min")
    v = VariantConfig(entity_final_layer_name="none", entity_final_pooling="max")          # inherited, and kept by base()
    assert (v.base().entity_final_layer_name, v.base().entity_final_pooling) == ("none", "max")
    model = Model(GhmfcConfig(num_candidates=4, embed_dim=16, image_dim=32, mention_tokens=12, image_regions=3, num_heads=2,
                              entity_final_layer_name="none"))
    assert len(model.state_dict()) == 50 == len(model.param_list()) and isinstance(model.entity_encoder.final_layer, nn.Identity)


def test_reference_binding_reads_the_entity_names():
    for layer in ("linear", "none"):
        for pooling in ("avg", "max"):
            got = entity_settings_from_reference_args(reference_args(entity_final_layer_name=layer, entity_final_pooling=pooling))
            assert got == dict(entity_final_layer_name=layer, entity_final_pooling=pooling)
    assert entity_settings_from_reference_args(reference_args()) == dict(entity_final_layer_name="linear", entity_final_pooling="avg")
    with pytest.raises(NotImplementedError, match="bert default.*reference's own EntityEncoder constructor\\s+raises ValueError"):
        entity_settings_from_reference_args(reference_args(entity_final_pooling="bert default"))
    with pytest.raises(NotImplementedError, match="entity_final_pooling = 'min'"):
        entity_settings_from_reference_args(reference_args(entity_final_pooling="min"))
    with pytest.raises(NotImplementedError, match="entity_final_layer_name = 'transformer'"):
        entity_settings_from_reference_args(reference_args(entity_final_layer_name="transformer"))
    with pytest.raises(NotImplementedError, match="online_bert"):
        entity_settings_from_reference_args(reference_args(online_bert=True))
    # the two legacy functions keep refusing
    for name, value in (("entity_final_layer_name", "none"), ("entity_final_pooling", "max")):
        for legacy in (config_from_reference_args, variant_config_from_reference_args):
            with pytest.raises(NotImplementedError, match=name):
                legacy(reference_args(**{name: value}))


def test_shim_honours_the_entity_names(monkeypatch):
    shim = bind(monkeypatch, reference_args(dataset_name="wikimel", entity_final_pooling="max"))
    m = shim.Model()
    assert isinstance(m, TrainableModel) and isinstance(m, shim.Model) and len(m.state_dict()) == 52
    assert (m.cfg.entity_final_layer_name, m.cfg.entity_final_pooling) == ("linear", "max") and m.dropout == 0.3
    shim = bind(monkeypatch, reference_args(dataset_name="wikimel", entity_final_pooling="max", entity_final_layer_name="none"))
    m = shim.Model()
    assert isinstance(m, TrainableModel) and len(m.state_dict()) == 50 and not m.cfg.entity_default
    shim = bind(monkeypatch, reference_args(mention_final_layer_name="linear", entity_final_layer_name="none"))
    m = shim.Model()
    assert isinstance(m, VariantModel) and list(m.state_dict()) == ["mention_encoder.final_layer.linear.weight",
                                                                    "mention_encoder.final_layer.linear.bias"]
    assert (m.cfg.entity_final_layer_name, m.cfg.entity_final_pooling) == ("none", "avg")
    shim = bind(monkeypatch, reference_args(mention_final_layer_name="none", entity_final_layer_name="none", entity_final_pooling="max"))
    assert len(shim.Model().state_dict()) == 0
    shim = bind(monkeypatch, reference_args())                                             # the default stays the default
    assert shim.Model().cfg.entity_default and len(shim.Model().state_dict()) == 52
    for over, match in ((dict(entity_final_pooling="bert default"), "bert default"), (dict(online_bert=True), "online_bert"),
                        (dict(entity_final_pooling="max", multimodal_subspace_activation="relu"), "multimodal_subspace_activation")):
        shim = bind(monkeypatch, reference_args(**over))
        with pytest.raises(NotImplementedError, match=match):
            shim.Model()
        with pytest.raises(NotImplementedError, match=match):
            shim.create_datasets()


def test_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in NEW_INT:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    assert "typedef enum { DRIN_POOL_AVG = 0, DRIN_POOL_MAX = 1 } drin_entity_pooling;" in header
    assert (_lib.POOL_AVG, _lib.POOL_MAX) == (0, 1)
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12


def test_token_pool_entry_points_validate_on_host():
    lib = _lib.load()

    def plain(feat=ONE, mask=ONE, out=ONE, pairs=5, tokens=6, width=16, pooling=_lib.POOL_MAX):
        return lib.drin_entity_token_pool(feat, mask, out, pairs, tokens, width, pooling, None)

    def indexed(feat=ONE, mask=ONE, index=ONE, E=9, out=ONE, pairs=5, tokens=6, width=16, pooling=_lib.POOL_MAX, status=ONE):
        return lib.drin_entity_token_pool_indexed(feat, mask, index, E, out, pairs, tokens, width, pooling, status, None)

    for f, who, first in ((plain, "drin_entity_token_pool", "feat"), (indexed, "drin_entity_token_pool_indexed", "text")):
        assert f(None) == _lib.E_NULL and last() == f"{who}: {first} is NULL"
        assert f(ODD) == _lib.E_ALIGN and last() == f"{who}: {first} is not 16-byte aligned"
        assert f(out=None) == _lib.E_NULL and last() == f"{who}: out is NULL"
        assert f(out=ODD) == _lib.E_ALIGN and last() == f"{who}: out is not 16-byte aligned"
        assert f(mask=None) == _lib.E_NULL and last() == f"{who}: mask is NULL"
        for pooling in (2, -1):
            assert f(pooling=pooling) == _lib.E_UNSUPPORTED and last().startswith(f"{who}: pooling = {pooling} is neither DRIN_POOL_AVG")
        for width in (0, 6, -4):
            assert f(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
        assert f(pairs=0) == _lib.E_SHAPE and "pairs = 0" in last()
        for tokens in (0, 513):
            assert f(tokens=tokens) == _lib.E_SHAPE and f"tokens = {tokens} is not in [1, 512]" in last()
    assert indexed(index=None) == _lib.E_NULL and last() == "drin_entity_token_pool_indexed: index is NULL"
    assert indexed(index=ODD) == _lib.E_ALIGN and "index must be 8-byte" in last()
    assert indexed(status=C.c_void_p(18)) == _lib.E_ALIGN and "index_status 4-byte" in last()
    for E in (0, -3):
        assert indexed(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()


def test_entity_rows_ex_validates_on_host():
    lib = _lib.load()
    who = "drin_ghmfc_entity_rows_ex"

    def run(text=ONE, mask=ONE, E=9, T=6, D=16, pooling=_lib.POOL_MAX, w=ONE, b=ONE, precision=_lib.PREC_BF16X3, rows=ONE, ws=ONE,
            nbytes=BIG):
        return lib.drin_ghmfc_entity_rows_ex(text, mask, E, T, D, pooling, w, b, precision, rows, ws, nbytes, None)

    for name in ("text", "rows", "mask", "ws"):
        assert run(**{name: None}) == _lib.E_NULL and last().startswith(who), name
    for name in ("w", "b"):                                       # exactly one of the two weights
        assert run(**{name: None}) == _lib.E_NULL and last() == f"{who}: exactly one of w_entity / b_entity is NULL (both NULL: final_layer = Identity)"
    for name in ("text", "w", "b", "rows", "ws"):
        assert run(**{name: ODD}) == _lib.E_ALIGN and last().startswith(who), name
    for identity in (dict(), dict(w=None, b=None)):
        for pooling in (2, -1):
            assert run(pooling=pooling, **identity) == _lib.E_UNSUPPORTED and f"{who}: pooling = {pooling}" in last()
        for D in (0, 6, -4):
            assert run(D=D, **identity) == _lib.E_SHAPE and "multiple of 4" in last()
        for E in (0, -1):
            assert run(E=E, **identity) == _lib.E_SHAPE and f"num_entities = {E}" in last()
        assert run(T=-1, **identity) == _lib.E_SHAPE and run(T=513, **identity) == _lib.E_SHAPE
        assert run(precision=7, **identity) == _lib.E_UNSUPPORTED
        assert run(text=None, **identity) == _lib.E_NULL and run(rows=None, **identity) == _lib.E_NULL
        assert run(mask=None, **identity) == _lib.E_NULL and run(rows=ODD, **identity) == _lib.E_ALIGN
    assert run(nbytes=16) == _lib.E_WORKSPACE and f"{who}: workspace 16 bytes <" in last()
    # Identity: the pool writes into rows, so neither a workspace nor its size is asked for - the next check is the device's
    # (reached only with real pointers: tests/test_gpu_entity_pool.py)
    assert lib.drin_ghmfc_entity_rows_workspace_bytes(9, 6, 16) >= 9 * 16 * 4
