"""-m gpu: what the folded forward's plan (csrc/fused_forward.hip: `folded_plan`) says against what one call launches.

One case per form of x_i C_i^T at the smallest shape that takes it - exact fp32, fp32 rows split in place, bf16 rows in place,
planes written by the stream pass (the table form, fp32 and bf16 tables), the one fp16 pass with its serial neighbour, the side
schedule with its neighbour just below the threshold, split-bf16 at widths off the planes - and the per-entity cache in both row
formats.  Each case profiles ONE call (`drin_profile_begin` / `_end`) and asserts the launches per kernel class against the
numbers recorded from the library before the plan existed (same shapes, same seeds), then asks `drin_image_contraction_passes` /
`drin_image_contraction_side_tiles` for the call's own config and asserts the form the case names: the query and the launch are
tied to each other here and nowhere else.  The four refusals keep their status and text."""
import ctypes as C

import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig, wikimel_config
from drin_amd.model import EntityTable, IndexedBatch, Model, _param_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
FEATURE_SLOTS = (0, 4, 5, 7, 9, 10)
CLASSES = ("gemm", "gemm_x3", "gemm_planes", "stream")


def small(dataset="wikimel", D=64, R=128):
    """N = 11; WikiMEL layout: token blocks (T = 5), WikiDiverse: pooled entity text."""
    cfg = DrinConfig(dataset_name=dataset, num_candidates_data=10, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
                     resnet_num_region=3, max_mention_sentence_len=9, max_entity_attr_token_len=5)
    cfg.validate()
    return cfg


def exact():
    """N = 101 at 768 / 2048, T = 8."""
    return wikimel_config(max_entity_attr_token_len=8, max_mention_sentence_len=16, resnet_num_region=4)


# form -> (passes, side tiles > 0) the two queries must answer for the call's config
FORMS = {"exact": (0, False), "split_rows": (3, False), "split_rows_side": (3, True), "bf16_rows": (2, False), "bf16_rows_side": (2, True),
         "stream_planes": (3, False), "stream_planes_bf16": (2, False), "f16_plane": (1, False), "cached": None}

# name: (config, B, precision, bf16-stored features, rows, form, launches (gemm, gemm_x3, gemm_planes, stream, every other class))
CASES = {
    "exact_f32": (small, 3, "f32", False, "gathered", "exact", (12, 0, 0, 1, 8)),
    "split_rows": (small, 3, "bf16x3", False, "gathered", "split_rows", (9, 1, 2, 1, 8)),
    "split_rows_exact_widths": (exact, 2, "bf16x3", False, "gathered", "split_rows", (14, 1, 2, 1, 9)),
    "bf16_rows": (small, 3, "bf16x3", True, "gathered", "bf16_rows", (9, 0, 3, 1, 8)),
    "bf16_rows_pooled_text": (lambda: small("wikidiverse"), 3, "bf16x3", True, "gathered", "bf16_rows", (9, 0, 3, 1, 8)),
    "table_f32": (small, 3, "bf16x3", False, "table", "stream_planes", (9, 0, 3, 1, 8)),
    "table_bf16": (small, 3, "bf16x3", True, "table", "stream_planes_bf16", (9, 0, 3, 1, 8)),
    "off_planes": (lambda: small(D=100, R=200), 3, "bf16x3", False, "gathered", "split_rows", (12, 0, 0, 1, 8)),
    "f16_pass": (exact, 107, "bf16x3_if16", False, "gathered", "f16_plane", (12, 1, 2, 1, 9)),
    "below_the_f16_pass": (exact, 106, "bf16x3_if16", False, "gathered", "split_rows", (14, 1, 2, 1, 9)),
    "side": (exact, 1013, "bf16x3", False, "gathered", "split_rows_side", (0, 11, 2, 1, 9)),
    "below_the_side": (exact, 1011, "bf16x3", False, "gathered", "split_rows", (0, 10, 2, 1, 9)),
    "side_bf16": (exact, 1013, "bf16x3", True, "gathered", "bf16_rows_side", (0, 9, 4, 1, 9)),
    "below_the_side_bf16": (exact, 1011, "bf16x3", True, "gathered", "bf16_rows", (0, 9, 3, 1, 9)),
    "cached_f32": (small, 3, "bf16x3", False, "cache:f32", "cached", (5, 0, 1, 1, 8)),
    "cached_mixed_f16": (small, 3, "bf16x3", False, "cache:mixed_f16", "cached", (5, 0, 1, 1, 8)),
}
BAD_ROW = 57   # one candidate row past the 50-row table, at pair (1, 2)


def build(name):
    """(model, batch) of a case: seeded weights and inputs, the same in every process."""
    make_cfg, B, precision, bf16, rows, _form, _counts = CASES[name]
    cfg = make_cfg()
    model = Model(cfg, precision=precision).to(DEV).eval()
    model.load_state_dict(synth.make_state_dict(cfg, 7))
    dtype = torch.bfloat16 if bf16 else torch.float32
    if cfg.bert_embed_dim == 768:
        batch = synth.make_device_batch(cfg, B, 11, torch.device(DEV, 0), dtype=dtype)[:14]
    else:
        batch = [t.to(DEV) for t in synth.make_batch(cfg, B, 11)[:14]]
        batch = [t.to(dtype) if i in FEATURE_SLOTS else t for i, t in enumerate(batch)]
    if rows == "gathered":
        return model, batch
    tab = synth.make_batch(cfg.with_(num_candidates_data=49), 1, 17)
    feat = lambda t: t.to(dtype)                                          # noqa: E731
    table = EntityTable(feat(tab[7][0]), tab[8][0] if cfg.token_level_entities else None, feat(tab[9][0]), feat(tab[10][0]), tab[11][0]).to(DEV)
    cand = torch.randint(0, 50, (B, cfg.num_candidates_model), generator=torch.Generator().manual_seed(5))
    cand[1, 2] = BAD_ROW
    if rows.startswith("cache:"):
        table.enable_cache(True, format=rows.split(":")[1])
    return model, IndexedBatch(batch[:7], table, cand.to(DEV), batch[12], batch[13])


def score(name, profiled=True):
    """One warm call (folds, cache rows), then the measured one: {scores, status words, launches per class, passes, side tiles}."""
    model, batch = build(name)
    lib = _lib.load()
    out = {}
    with torch.no_grad():
        for measured in (False, True):
            if measured and profiled:
                _lib.profile_begin()
            scores = model(batch).clone()
            if measured and profiled:
                prof = _lib.profile_end()
                out["launches"] = tuple(prof[k][1] for k in CLASSES) + (sum(n for k, (_ms, n) in prof.items() if k not in CLASSES),)
            torch.cuda.synchronize()
            if isinstance(batch, IndexedBatch):                       # the clamped row is reported, not raised: read, then clear
                out["status"] = model._status_words(torch.device(DEV, 0)).cpu().tolist()
                model._index_watch.clear()
                model._status_words(torch.device(DEV, 0)).zero_()
        c = model._route(batch, _param_list(model)).call.cfg          # (under no_grad: the inference route, the call's own config)
    indexed = 1 if c.num_entities > 0 else 0
    out["scores"] = scores.cpu()
    out["passes"] = lib.drin_image_contraction_passes(C.byref(c), indexed)
    out["side"] = lib.drin_image_contraction_side_tiles(C.byref(c), indexed)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_launches_and_queries_agree_with_the_form(name):
    _cfg, _B, _precision, _bf16, rows, form, launches = CASES[name]
    got = score(name)
    print(f"{name}: launches (gemm, gemm_x3, gemm_planes, stream, other) {got['launches']}, passes {got['passes']}, side tiles {got['side']}")
    assert torch.isfinite(got["scores"]).all()
    assert got["launches"] == launches
    if rows != "gathered":
        assert got["status"][0] == 1 and got["status"][1] == 1 * 11 + 2 and got["status"][2] == BAD_ROW
    if FORMS[form] is not None:
        passes, side = FORMS[form]
        assert got["passes"] == passes and (got["side"] > 0) == side


def refusal(name, edit):
    """Status and text of `drin_forward_prepared` on the call of case `name` after `edit(call)`."""
    model, batch = build(name)
    lib = _lib.load()
    params = _param_list(model)
    with torch.no_grad():
        model(batch)                                                  # the folds
        call = model._route(batch, params).call
        edit(call)
        _keep, pc = call.param_struct(params)
        pbuf = model._prepared.get(call, params, pc)
        ws, scores = call.byte_buffer(lib.drin_fused_workspace_bytes(C.byref(call.cfg))), call.scores()
        status = lib.drin_forward_prepared(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), pbuf.data_ptr(), ws.data_ptr(), ws.numel(),
                                           scores.data_ptr(), call.stream())
        torch.cuda.synchronize()
    return status, lib.drin_last_error().decode()


def _pooled_ahead(call):
    call.batch.entity_text_cls = call.batch.entity_text


def _no_tables(call):
    call.cfg.num_entities = 0


def _exact_fp32(call):
    call.cfg.precision = _lib.PREC_F32


REFUSALS = {
    "entity_text_cls": ("split_rows", _pooled_ahead, _lib.E_UNSUPPORTED,
                        "drin_forward_prepared: entity_text_cls (text pooled ahead of time) is a form of the training entry points"),
    "index_without_tables": ("table_f32", _no_tables, _lib.E_SHAPE, "drin_forward_prepared: entity_index given but cfg.num_entities = 0"),
    "table_in_exact_fp32": ("table_f32", _exact_fp32, _lib.E_UNSUPPORTED,
                            "drin_forward_prepared: entity_index needs the split-bf16 precision (the stream kernel gathers the GEMM operands "
                            "as planes); gather on the caller side for DRIN_PREC_F32"),
    "bf16_features_off_the_planes": ("bf16_rows", _exact_fp32, _lib.E_UNSUPPORTED,
                                     "drin_forward_prepared: bf16 features need the split-bf16 precision (DRIN_PREC_BF16X3) and D, R multiples of 32"),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals_keep_status_and_text(which):
    name, edit, status, text = REFUSALS[which]
    assert refusal(name, edit) == (status, text)
