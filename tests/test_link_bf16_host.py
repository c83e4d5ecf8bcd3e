"""Linking against bf16-STORED table rows, without a GPU: the `_ex` twins exist in the header, the library
and the binding under ABI 12 and 12 kernel classes; every refusal of theirs comes from the argument checks, before any launch
(no device is present here, so a launch could only fail otherwise); the workspace queries grow by exactly the regions the two
product routes add; the Python surface accepts and refuses as documented; and the margins the GPU parity rule relies on hold on
the fp64 cosines of the bf16-ROUNDED rows (tests/test_gpu_link_bf16.py runs the same cases)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from drin_amd import _lib, resources
from drin_amd.ghmfc_table import row_inv_norms, table_topk, table_topk_sum
from drin_amd.model import EntityTable, IndexedBatch, Model
from tests.drin_link_restatement import K_LINK, link_case
from tests.table_topk_sum_restatement import near_threshold, sum64, tol_of
from tests.test_gpu_table_topk import cosine64

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drin_hip.h")
EX = ("drin_row_inv_norms_ex", "drin_cosine_rows_indexed_fwd_ex", "drin_cross_modal_edges_ex", "drin_table_topk_ex",
      "drin_table_topk_workspace_bytes_ex", "drin_table_topk_sum_ex", "drin_table_topk_sum_workspace_bytes_ex")
F32, BF16 = _lib.FEAT_F32, _lib.FEAT_BF16
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
ALIGN_FLOATS = 64                                              # arena.h: every region starts on a 256-byte boundary

# ---- the cases the GPU test links, drawn here once ------------------------------------------------------------------------------
# (D, E, B, k, chunk, seed): section 24's parity shapes - the widen route with a ragged last chunk and Bp padding; the plane
# route in bf16x3 with K = one block; the reference width in one chunk.  Seeds picked on the CPU (the assertion below).
TOPK_CASES = [(16, 300, 3, 20, 64, 0), (32, 1500, 5, 64, 256, 0), (768, 2000, 5, 100, 0, 0)]
SUM_CASE = dict(E=1500, B=4, widths=(32, 16, 16), weights=(1.0, 0.5, 2.0), k=64, chunk=256, seed=0, cap=2)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 values rounded to bf16 (nearest even), still float32: what a table stored as bf16 holds"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def topk_case(D, E, B, seed):
    """x float32, rows ALREADY rounded to bf16 (as float32), and the fp64 cosines of exactly those values"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, D)).astype(np.float32)
    rows = bf16_round(g.standard_normal((E, D)).astype(np.float32))
    return x, rows, cosine64(x, rows)


def sum_case():
    c = SUM_CASE
    g = np.random.default_rng(c["seed"])
    xs = [g.standard_normal((c["B"], d)).astype(np.float32) for d in c["widths"]]
    tables = [bf16_round(g.standard_normal((c["E"], d)).astype(np.float32)) for d in c["widths"]]
    return xs, tables


# ---- the symbols ----------------------------------------------------------------------------------------------------------------
def test_the_ex_twins_exist_in_the_header_the_library_and_the_binding():
    lib, header = _lib.load(), open(HEADER).read()
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12
    declared = set(re.findall(r"DRIN_API\s+[\w\s\*]+?\b(drin_\w+)\s*\(", header))
    for name in EX:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        assert name[:-3] in declared                          # each twin stands beside the entry point it extends
    assert declared == set(_lib.EXPORTS)                      # header <-> binding, the new names included
    flowed = re.sub(r"\s*\n\s*\*\s*", " ", header)             # comment text without its line breaks
    assert flowed.count("bf16 table links exactly as its exactly-widened fp32 copy would") >= 5      # the contract, in every comment
    for route in ("PLANE route", "WIDEN route"):
        assert route in header


def test_the_new_instantiations_use_no_scratch_and_spill_nothing():
    rows = [k for k in resources.kernel_resources()
            if any(n in k["name"] for n in ("k_cross_modal_edges", "k_cosine_gather", "k_row_inv_norms", "k_widen_rows"))]
    bf16 = [k for k in rows if "DF16b" in k["name"]]          # the Itanium mangling of __bf16
    assert sum("k_cross_modal_edges" in k["name"] for k in bf16) == 6     # V = 0, 1, 2 x one edge, both
    assert sum("k_cosine_gather" in k["name"] for k in bf16) == 1 and sum("k_row_inv_norms" in k["name"] for k in bf16) == 1
    assert sum("k_widen_rows" in k["name"] for k in rows) == 1
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k   # no scratch, no spills
        assert k["group_segment_fixed_size"] == 0, k                                                                   # no LDS


# ---- refusals, all before a launch ----------------------------------------------------------------------------------------------
A = 1 << 20                                                    # a 16-byte aligned "device address": never dereferenced on the host


def err():
    return _lib.load().drin_last_error().decode()


def test_every_ex_refusal_is_an_argument_check():
    lib = _lib.load()
    term = (_lib.DrinTopkTermC * 2)()
    for t in term:
        t.x, t.rows, t.row_inv_norms, t.width, t.weight = A, A, A, 16, 1.0
    dt = (C.c_int32 * 2)(BF16, F32)
    calls = {
        "drin_row_inv_norms_ex": lambda rows=A, d=BF16, w=16: lib.drin_row_inv_norms_ex(rows, d, 5, w, 1e-8, A, None),
        "drin_cosine_rows_indexed_fwd_ex": lambda rows=A, d=BF16, w=16: lib.drin_cosine_rows_indexed_fwd_ex(A, rows, d, A, 5, A, 2, 3, w, 1e-8, None, None),
        "drin_cross_modal_edges_ex": lambda rows=A, d=BF16, w=16: lib.drin_cross_modal_edges_ex(A, A, rows, rows, d, A, 5, 2, 3, w, 1.0, 1e-8, A, A, None, None),
        "drin_table_topk_ex": lambda rows=A, d=BF16, w=16: lib.drin_table_topk_ex(A, rows, d, A, 5, 2, w, 3, 1e-8, _lib.PREC_F32, 0, A, 1 << 30, A, A, None),
    }
    for name, call in calls.items():
        assert call(d=7) == _lib.E_UNSUPPORTED and "row dtype 7" in err() and name in err(), name           # unknown dtype
        assert call(d=-1) == _lib.E_UNSUPPORTED, name
        assert call(w=12) == _lib.E_SHAPE and "multiple of 8" in err() and name in err(), name              # 12 % 4 == 0, % 8 != 0
        assert call(w=12, d=F32) != _lib.E_SHAPE or "multiple of 8" not in err(), name                      # fp32 rows keep width % 4
        assert call(rows=A + 8) == _lib.E_ALIGN and "16-byte aligned" in err(), name                        # misaligned rows
        assert call(rows=None) == _lib.E_NULL and name in err(), name
    assert lib.drin_table_topk_workspace_bytes_ex(2, 5, 12, 3, 0, BF16, _lib.PREC_F32) == 0 and "multiple of 8" in err()
    assert lib.drin_table_topk_workspace_bytes_ex(2, 5, 16, 3, 0, 9, _lib.PREC_F32) == 0 and "row dtype 9" in err()
    assert lib.drin_table_topk_workspace_bytes_ex(2, 5, 16, 3, 0, BF16, 77) == 0 and "precision 77" in err()
    # the sum: the dtypes are a host array beside the unchanged terms
    run = lambda dts, n=2: lib.drin_table_topk_sum_ex(term, dts, n, 5, 2, 3, 1e-8, _lib.PREC_F32, 0, A, 1 << 30, A, A, None)   # noqa: E731
    assert run(None) == _lib.E_NULL and "row_dtypes is NULL" in err()
    assert run((C.c_int32 * 2)(BF16, 5)) == _lib.E_UNSUPPORTED and "row dtype 5" in err()
    term[0].width = 12
    assert run(dt) == _lib.E_SHAPE and "multiple of 8" in err()
    assert lib.drin_table_topk_sum_workspace_bytes_ex(term, dt, 2, 2, 5, 3, 0, _lib.PREC_F32) == 0 and "multiple of 8" in err()
    term[0].width, term[0].rows = 16, A + 8
    assert run(dt) == _lib.E_ALIGN
    term[0].rows = None
    assert run(dt) == _lib.E_NULL
    term[0].weight, term[0].width = 0.0, 12                   # a dropped term: neither its pointers nor its dtype are read
    assert lib.drin_table_topk_sum_workspace_bytes_ex(term, (C.c_int32 * 2)(99, F32), 2, 2, 5, 3, 0, _lib.PREC_F32) > 0
    assert lib.drin_table_topk_sum_workspace_bytes_ex(term, None, 2, 2, 5, 3, 0, _lib.PREC_F32) == 0 and "row_dtypes is NULL" in err()


# ---- the workspace ---------------------------------------------------------------------------------------------------------------
def region(floats: int) -> int:
    return -(-floats // ALIGN_FLOATS) * ALIGN_FLOATS * 4     # bytes a region of `floats` floats takes


def test_workspace_queries_grow_by_exactly_the_new_regions():
    lib = _lib.load()
    assert lib.drin_host_selftest() == 0, err()
    old = lib.drin_table_topk_workspace_bytes
    new = lib.drin_table_topk_workspace_bytes_ex
    for B, E, D, k, chunk in [(3, 300, 16, 20, 64), (5, 1500, 32, 64, 256), (5, 2000, 768, 100, 512), (5, 2000, 776, 100, 512), (64, 5000, 768, 100, 1024)]:
        base, Bp = old(B, E, D, k, chunk), -(-B // 4) * 4
        assert base > 0
        for prec in (_lib.PREC_F32, _lib.PREC_BF16X3):
            assert new(B, E, D, k, chunk, F32, prec) == base                                   # fp32 rows: the old bytes
            planes = prec == _lib.PREC_BF16X3 and D % 32 == 0
            extra = region(Bp * D) if planes else region(min(chunk, E) * D)                    # hi + lo planes of xpad | one widened chunk
            assert new(B, E, D, k, chunk, BF16, prec) == base + extra, (B, E, D, k, chunk, prec)
    # the default chunk: unchanged on the plane route, bounded by the widened region on the widen route (256 MiB of fp32 rows)
    B, E, D, k = 64, 1_000_000, 768, 100
    base = old(B, E, D, k, 0)
    assert new(B, E, D, k, 0, BF16, _lib.PREC_BF16X3) == base + region(64 * D)
    chunk = (256 << 20) // (4 * D) // 256 * 256
    assert chunk * D * 4 <= 256 << 20 < (chunk + 256) * D * 4
    assert new(B, E, D, k, 0, BF16, _lib.PREC_F32) == old(B, E, D, k, chunk) + region(chunk * D)
    # the sum: planes per plane-route term, ONE widened chunk as wide as the widest widen-route term
    widths, chunk, B, E, k = (32, 16, 24), 256, 5, 1500, 64
    term = (_lib.DrinTopkTermC * 3)()
    for t, w in zip(term, widths):
        t.width, t.weight = w, 1.0
    base = lib.drin_table_topk_sum_workspace_bytes(term, 3, B, E, k, chunk)
    q = lambda dts, prec: lib.drin_table_topk_sum_workspace_bytes_ex(term, (C.c_int32 * 3)(*dts), 3, B, E, k, chunk, prec)   # noqa: E731
    assert base > 0 and q((F32, F32, F32), _lib.PREC_BF16X3) == base
    assert q((BF16, BF16, BF16), _lib.PREC_BF16X3) == base + region(8 * 32) + region(chunk * 24)
    assert q((BF16, F32, BF16), _lib.PREC_BF16X3) == base + region(8 * 32) + region(chunk * 24)
    assert q((BF16, BF16, F32), _lib.PREC_BF16X3) == base + region(8 * 32) + region(chunk * 16)
    assert q((BF16, BF16, BF16), _lib.PREC_F32) == base + region(chunk * 32)
    assert q((F32, F32, BF16), _lib.PREC_F32) == base + region(chunk * 24)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_set_clip_takes_one_storage_for_both_tables():
    t = link_case("wm")["table"]
    table = EntityTable(t.text, t.mask, t.image, t.object, t.object_score)
    E = table.num_entities
    good = torch.randn(E, 8)
    for bad in (good.double(), good.half()):
        with pytest.raises(ValueError, match="float32"):
            table.set_clip(bad, good)
        with pytest.raises(ValueError, match="float32"):
            table.set_clip(good.bfloat16(), bad)
    with pytest.raises(ValueError, match="differ in dtype"):
        table.set_clip(good.bfloat16(), good)
    with pytest.raises(ValueError, match="multiple of 8"):
        table.set_clip(torch.randn(E, 12).bfloat16(), torch.randn(E, 12).bfloat16())
    assert table.clip_text is None
    stored = good.bfloat16()
    assert table.set_clip(stored, stored) is table and table.clip_text.dtype == torch.bfloat16 and torch.equal(table.clip_text, stored)
    moved = table.to("cpu")
    assert moved.clip_text.dtype == torch.bfloat16 and moved.clip_image.dtype == torch.bfloat16 and torch.equal(moved.clip_image, stored)
    assert table.set_clip(torch.randn(E, 12), torch.randn(E, 12)).clip_text.dtype == torch.float32      # fp32 keeps C % 4


def test_the_wrappers_refuse_what_they_cannot_read_in_place():
    x, rows = torch.randn(3, 16), torch.randn(50, 16).bfloat16()
    inv = torch.ones(50)
    with pytest.raises(ValueError, match="contiguous float32"):
        table_topk(x.double(), rows, inv, 5, 1e-8, "f32")
    with pytest.raises(ValueError, match="contiguous float32"):
        table_topk(x, rows, inv.double(), 5, 1e-8, "f32")
    with pytest.raises(ValueError, match="read in place"):
        row_inv_norms(torch.randn(50, 32).bfloat16()[:, :16], 1e-8)
    with pytest.raises(ValueError, match="term 0: x must be a contiguous float32"):   # x of a bf16 term stays float32; a term in
        table_topk_sum([(x.bfloat16(), rows, inv, 1.0)], 5, 1e-8, "f32")              # order stops at the device: GPU only (the
    with pytest.raises(ValueError, match="term 0: x must be .* on the GPU"):           # rows' own refusals: tests/test_gpu_link_bf16.py)
        table_topk_sum([(x, rows, inv, 1.0)], 5, 1e-8, "f32")


def test_a_wrong_span_is_refused_before_the_launch_of_the_bf16_span_mean():
    text = torch.randn(3, 12, 64).bfloat16()
    with pytest.raises(ValueError, match="are not \\[batch\\]"):
        Model._span_mean_stored(text, torch.zeros(2, dtype=torch.int32), torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="are not \\[batch\\]"):
        Model._span_mean_stored(text, torch.zeros(3, dtype=torch.int64), torch.ones(3, 1, dtype=torch.int64))


def stored_case():
    """the "wm" link case with its six feature tensors and the CLIP tables as bf16"""
    c = link_case("wm")
    t, bf = c["table"], torch.bfloat16
    table = EntityTable(t.text.to(bf), t.mask, t.image.to(bf), t.object.to(bf), t.object_score).set_clip(t.clip_text.to(bf), t.clip_image.to(bf))
    mention = [m.to(bf) if i in (0, 4, 5) else m for i, m in enumerate(c["mention"])]
    return c, table, mention


def test_model_link_accepts_and_refuses_bf16_storage_as_documented():
    c, table, mention = stored_case()
    model = Model(c["cfg"]).eval()
    E = table.num_entities
    clips = (c["clip_image"], c["clip_text"])
    # all of these pass every check of the bf16 storage and stop at the device check alone: no CPU fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(mention, table, K_LINK, *clips, first_stage="edges")
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(mention, table, K_LINK, *clips, queries=torch.randn(3, 16), rows=torch.randn(E, 16).bfloat16())
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(mention, table, K_LINK, *clips, candidates=c["candidates"])
    with pytest.raises(RuntimeError, match="GPU only"):
        IndexedBatch.from_clip(mention, table, c["candidates"], *clips)
    # the storage rule: all six feature tensors as bfloat16, or none
    with pytest.raises(NotImplementedError, match="bf16-stored rows"):
        model.link(c["mention"], table, K_LINK, *clips, first_stage="edges")                   # bf16 table text, float32 mention text
    with pytest.raises(NotImplementedError, match="bf16-stored rows"):
        model.link(mention, c["table"], K_LINK, *clips, first_stage="edges")                   # and the other way round
    with pytest.raises(RuntimeError, match="GPU only"):                                        # a dropped tt does not look at the text
        model.link(c["mention"], table, K_LINK, *clips, first_stage="edges", edge_weights=(0, 1, 1))
    with pytest.raises(ValueError, match="float32 \\[3, 64\\]"):                               # the mentions' CLIP rows stay float32
        model.link(mention, table, K_LINK, clips[0].bfloat16(), clips[1], first_stage="edges")
    with pytest.raises(ValueError, match="float32 \\[3, 64\\]"):
        IndexedBatch.from_clip(mention, table, c["candidates"], clips[0], clips[1].bfloat16())
    with pytest.raises(ValueError, match="Dq % 8"):
        model.link(mention, table, K_LINK, *clips, queries=torch.randn(3, 12), rows=torch.randn(E, 12).bfloat16())
    with pytest.raises(ValueError, match="must be float32"):
        model.link(mention, table, K_LINK, *clips, queries=torch.randn(3, 16).bfloat16(), rows=torch.randn(E, 16).bfloat16())
    with pytest.raises(ValueError, match="must be float32"):
        model.link(mention, table, K_LINK, *clips, queries=torch.randn(3, 16), rows=torch.randn(E, 16).half())


# ---- the margins of the GPU parity rule, on the rounded rows --------------------------------------------------------------------
@pytest.mark.parametrize("D,E,B,k,chunk,seed", TOPK_CASES)
def test_topk_cases_have_room_around_the_kth_cosine_of_the_rounded_rows(D, E, B, k, chunk, seed):
    _x, _rows, ref = topk_case(D, E, B, seed)
    for precision, tol in TOL.items():
        assert near_threshold(ref, k, tol) <= 2, (D, E, precision)
    if D == 16:
        # this case takes the widen route in bf16x3 too, where a chunk under 256 rows runs the exact fp32 kernel and one chunk of
        # all 300 rows the split-bf16 one: two DIFFERENT kernels.  The GPU test still asserts that both chunkings return the same
        # list, and this margin is why it may: the (k + 1)-th cosine lies more than twice the bar under the k-th, so any two
        # calls that hold section 24's rule return the same k rows (and the re-score orders them alike)
        ranked = np.sort(ref, axis=1)[:, ::-1]
        assert float((ranked[:, k - 1] - ranked[:, k]).min()) > 2 * TOL["bf16x3"]


def test_sum_case_has_room_around_the_kth_score_of_the_rounded_tables():
    c = SUM_CASE
    xs, tables = sum_case()
    for weights in (c["weights"], (c["weights"][0], 0.0, c["weights"][2])):
        ref = sum64(xs, tables, weights)
        for precision in TOL:
            assert near_threshold(ref, c["k"], tol_of(weights, precision)) <= c["cap"], (weights, precision)
