"""-m gpu: linking against bf16-STORED table rows.  The contract is one sentence - a bf16 table links exactly
as its exactly-widened fp32 copy would - and the references are that widened copy (`rows.float()`, torch) and fp64:

* the row kernels (`drin_row_inv_norms_ex`, `drin_cosine_rows_indexed_fwd_ex`, `drin_cross_modal_edges_ex`) bit for bit against the
  fp32 entry points on the widened rows, and each `_ex` with DRIN_FEAT_F32 bit for bit against the entry point it extends;
* `drin_table_topk_ex` / `drin_table_topk_sum_ex` by section 24's rule against fp64 on the rounded rows (1e-4 bf16x3, 1e-5 f32), their
  scores the bits of the `_ex` cosines, and in f32 precision rows AND scores those of the fp32 call on the widened table; which
  product route ran is read from the library's profiler record;
* `Model.link` on the small WikiMEL-shaped case with all six features and the CLIP tables as bf16, in its three forms.
The cases and their margins: tests/test_link_bf16_host.py.  Every test prints its maxima; set LINK_BF16_PARITY_OUT to a path to have
them written there as JSON (profiles/link_bf16_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk, table_topk_sum
from drin_amd.model import IndexedBatch, Model
from tests.drin_link_restatement import K_LINK, canonical, rank_order
from tests.table_topk_sum_restatement import chain32, sum64, tol_of
from tests.test_gpu_table_topk import PRECISION, dev, holds_rule, is_contract_ordered
from tests.test_gpu_table_topk_sum import holds_rule as holds_sum_rule
from tests.test_link_bf16_host import SUM_CASE, TOL, TOPK_CASES, stored_case, sum_case, topk_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, SCALE = 1e-8, 100.0
F32, BF16 = _lib.FEAT_F32, _lib.FEAT_BF16
BF = torch.bfloat16
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)   # noqa: E731
same = lambda a, b: torch.equal(bits(a), bits(b))   # noqa: E731
dtype_of = lambda t: BF16 if t.dtype == BF else F32   # noqa: E731


_PARITY = {}


def record(key: str, value: float) -> None:
    _PARITY[key] = value
    out = os.environ.get("LINK_BF16_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(_PARITY.items())), f, indent=1)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def status_value(w):
    value = ((w[3] & 0xFFFFFFFF) << 32 | (w[2] & 0xFFFFFFFF))
    return value - ((1 << 64) if value >= (1 << 63) else 0)


# ---- the row kernels, bit for bit against the fp32 entry points on rows.float() --------------------------------------------------
def inv_norms_ex(rows):
    out = torch.full((rows.shape[0],), 7.0, device=DEV)
    _lib.check(_lib.load().drin_row_inv_norms_ex(ptr(rows), dtype_of(rows), rows.shape[0], rows.shape[1], EPS, ptr(out), stream()))
    return out


def inv_norms_old(rows):
    out = torch.full((rows.shape[0],), 7.0, device=DEV)
    _lib.check(_lib.load().drin_row_inv_norms(ptr(rows), rows.shape[0], rows.shape[1], EPS, ptr(out), stream()))
    return out


@pytest.mark.parametrize("E", [1, 5, 257])
@pytest.mark.parametrize("width", [8, 40, 512, 768, 776])
def test_row_inv_norms_of_bf16_rows_are_the_bits_of_the_widened_rows(width, E):
    stored = randn(E, width, seed=width + E).to(BF)
    stored[E // 2] = 0                                                  # a zero row: 1 / eps
    wide = stored.float()
    want = inv_norms_old(wide)
    assert same(inv_norms_ex(stored), want) and same(inv_norms_ex(wide), want)       # bf16 in place | the twin on fp32 rows
    assert same(row_inv_norms(stored, EPS), want)
    ref = 1.0 / wide.double().norm(dim=1).clamp_min(EPS)
    assert ((want.double() / ref) - 1).abs().max().item() <= 2e-6       # tests/test_gpu_table_topk.py's bound on the fp32 kernel


def indexed_ex(x, rows, index, status=None):
    out = torch.full(tuple(index.shape), 7.0, device=DEV)
    _lib.check(_lib.load().drin_cosine_rows_indexed_fwd_ex(ptr(x), ptr(rows), dtype_of(rows), ptr(index), rows.shape[0], ptr(out),
                                                           index.shape[0], index.shape[1], x.shape[1], EPS, ptr(status), stream()))
    return out


def indexed_old(x, rows, index, status=None):
    out = torch.full(tuple(index.shape), 7.0, device=DEV)
    _lib.check(_lib.load().drin_cosine_rows_indexed_fwd(ptr(x), ptr(rows), ptr(index), rows.shape[0], ptr(out), index.shape[0],
                                                        index.shape[1], x.shape[1], EPS, ptr(status), stream()))
    return out


@pytest.mark.parametrize("N", [1, 5, 101])
@pytest.mark.parametrize("width", [8, 520, 768])
def test_indexed_cosine_on_bf16_rows_is_the_bits_of_the_widened_rows(width, N):
    B, E = 3, 9
    x, stored = randn(B, width, seed=3 * width + N), randn(E, width, seed=width + N + 1).to(BF)
    wide = stored.float()
    index = torch.randint(0, E, (B, N), generator=torch.Generator().manual_seed(N)).to(DEV)
    want = indexed_old(x, wide, index)
    assert same(indexed_ex(x, stored, index), want) and same(indexed_ex(x, wide, index), want)
    assert same(cosine_rows_indexed(x, stored, index, EPS, None), want)
    # one index of -1 and one of E: both clamped before an address is formed, the first reported pair and value kept
    bad = index.clone()
    bad[0, 0], bad[B - 1, N - 1] = -1, E
    for which, (b, n, value) in enumerate(((0, 0, -1), (B - 1, N - 1, E))):
        one = index.clone()
        one[b, n] = value
        st_bf, st_f32 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
        got, ref = indexed_ex(x, stored, one, st_bf), indexed_old(x, wide, one, st_f32)
        assert same(got, ref) and same(got, indexed_old(x, wide, one.clamp(0, E - 1)))
        w = st_bf.tolist()
        assert w == st_f32.tolist() and w[0] == 1 and w[1] == b * N + n and status_value(w) == value, (which, w)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert same(indexed_ex(x, stored, bad, st), indexed_old(x, wide, bad.clamp(0, E - 1))) and st[0].item() == 1   # both in one call


def edges_ex(m_image, m_text, t_text, t_image, index, miet=True, mtei=True, status=None):
    B, N = index.shape
    oi, ot = torch.full((B, N), 7.0, device=DEV), torch.full((B, N), 7.0, device=DEV)
    _lib.check(_lib.load().drin_cross_modal_edges_ex(
        ptr(m_image) if miet else None, ptr(m_text) if mtei else None, ptr(t_text) if miet else None, ptr(t_image) if mtei else None,
        dtype_of(t_text), ptr(index), t_text.shape[0], B, N, m_image.shape[1], SCALE, EPS, ptr(oi) if miet else None,
        ptr(ot) if mtei else None, ptr(status), stream()))
    return oi, ot


def edges_old(m_image, m_text, t_text, t_image, index, status=None):
    B, N = index.shape
    oi, ot = torch.full((B, N), 7.0, device=DEV), torch.full((B, N), 7.0, device=DEV)
    _lib.check(_lib.load().drin_cross_modal_edges(ptr(m_image), ptr(m_text), ptr(t_text), ptr(t_image), ptr(index), t_text.shape[0], B, N,
                                                  m_image.shape[1], SCALE, EPS, ptr(oi), ptr(ot), ptr(status), stream()))
    return oi, ot


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 101])                       # the trip boundaries for 2 and 4 candidates per trip, a partial last wave
@pytest.mark.parametrize("width", [8, 256, 512, 520])                  # V = 1, 1, 2 and the any-width form
def test_cross_modal_edges_on_bf16_tables_are_the_bits_of_the_widened_tables(width, N, B):
    E = 7
    m_image, m_text = randn(B, width, seed=width + N), randn(B, width, seed=width + N + 1)
    t_text, t_image = randn(E, width, seed=width + N + 2).to(BF), randn(E, width, seed=width + N + 3).to(BF)
    index = torch.randint(0, E, (B, N), generator=torch.Generator().manual_seed(N + B)).to(DEV)
    wide = (m_image, m_text, t_text.float(), t_image.float())
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    want_i, want_t = edges_old(*wide, index, status)
    got_i, got_t = edges_ex(m_image, m_text, t_text, t_image, index, status=status)
    assert same(got_i, want_i) and same(got_t, want_t) and status.tolist() == [0, 0, 0, 0]
    f32_i, f32_t = edges_ex(*wide, index)                               # the twin with DRIN_FEAT_F32: the old entry point's bits
    assert same(f32_i, want_i) and same(f32_t, want_t)
    only_i, none_t = edges_ex(m_image, m_text, t_text, t_image, index, mtei=False)       # each edge alone: the same bits, the other untouched
    none_i, only_t = edges_ex(m_image, m_text, t_text, t_image, index, miet=False)
    assert same(only_i, want_i) and same(only_t, want_t) and bool((none_t == 7.0).all()) and bool((none_i == 7.0).all())
    bad = index.clone()                                                 # an out-of-range candidate: clamped, reported like the fp32 kernel
    bad[B - 1, N - 1] = E + 5
    st_bf, st_f32 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    got_i, got_t = edges_ex(m_image, m_text, t_text, t_image, bad, status=st_bf)
    want_i, want_t = edges_old(*wide, bad, st_f32)
    w = st_bf.tolist()
    assert same(got_i, want_i) and same(got_t, want_t) and w == st_f32.tolist()
    assert w[0] == 1 and w[1] == (B - 1) * N + N - 1 and status_value(w) == E + 5


# ---- drin_table_topk_ex ----------------------------------------------------------------------------------------------------------------
def topk_ex(x, rows, inv, k, precision, chunk):
    lib = _lib.load()
    (B, D), E = x.shape, rows.shape[0]
    nbytes = lib.drin_table_topk_workspace_bytes_ex(B, E, D, k, chunk, dtype_of(rows), PRECISION[precision])
    assert nbytes > 0, lib.drin_last_error()
    guard = 256
    whole = torch.full((nbytes + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV)     # nothing is written outside the workspace
    ws = whole[guard:guard + nbytes]
    scores = torch.full((B, k), 7.0, device=DEV)
    best = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.drin_table_topk_ex(ptr(x), ptr(rows), dtype_of(rows), ptr(inv), E, B, D, k, EPS, PRECISION[precision], chunk, ptr(ws),
                                      nbytes, ptr(scores), ptr(best), stream()))
    torch.cuda.synchronize()
    assert bool((whole[:guard] == 0x5A).all()) and bool((whole[-guard:] == 0x5A).all())
    return scores, best


def topk_old(x, rows, inv, k, precision, chunk):
    lib = _lib.load()
    (B, D), E = x.shape, rows.shape[0]
    nbytes = lib.drin_table_topk_workspace_bytes(B, E, D, k, chunk)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    scores = torch.full((B, k), 7.0, device=DEV)
    best = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.drin_table_topk(ptr(x), ptr(rows), ptr(inv), E, B, D, k, EPS, PRECISION[precision], chunk, ptr(ws), nbytes, ptr(scores),
                                   ptr(best), stream()))
    return scores, best


_ON_DEVICE = {}


def device_case(D, E, B, seed):
    """x, the bf16 table, its widened copy and the inverse norms on the device, the fp64 cosines on the host: once per case"""
    key = (D, E, B, seed)
    if key not in _ON_DEVICE:
        x, rows, ref = topk_case(D, E, B, seed)
        wide = dev(rows)
        stored = wide.to(BF)
        assert torch.equal(stored.float(), wide)                        # the host case holds bf16 values: the widening is exact
        _ON_DEVICE[key] = (dev(x), stored, wide, inv_norms_ex(stored), ref)
    return _ON_DEVICE[key]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("D,E,B,k,chunk,seed", TOPK_CASES)
def test_table_topk_on_bf16_rows_links_as_the_widened_table(D, E, B, k, chunk, seed, precision):
    x, stored, wide, inv, ref = device_case(D, E, B, seed)
    assert same(inv, inv_norms_old(wide))
    what = f"bf16 rows D{D} E{E} B{B} k{k} chunk{chunk} {precision}"
    _lib.profile_begin()
    scores, best = topk_ex(x, stored, inv, k, precision, chunk)
    prof = _lib.profile_end()
    # which route ran: the plane kernel's class counts one launch per chunk on the plane route and none on the widen route
    chunks = -(-E // chunk) if chunk else 1
    as_planes = precision == "bf16x3" and D % 32 == 0
    print(f"{what}: gemm_planes {prof['gemm_planes'][1]}, gemm {prof['gemm'][1]}, gemm_x3 {prof['gemm_x3'][1]} launches over {chunks} chunks")
    assert prof["gemm_planes"][1] == (chunks if as_planes else 0), what
    assert as_planes or prof["gemm"][1] + prof["gemm_x3"][1] >= chunks, what        # the widen route: today's product, per chunk
    got_rows, got_scores = best.cpu().numpy(), scores.cpu().numpy()
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    assert same(scores, indexed_ex(x, stored, best)), what               # the bits of the _ex cosine on the returned rows
    holds_rule(ref, got_rows, k, TOL[precision], what)                   # section 24's rule, fp64 on the ROUNDED rows
    err = float(np.abs(got_scores - np.take_along_axis(ref, got_rows, 1)).max())
    print(f"{what}: max |returned score - fp64| = {err:.3e}")
    record(f"topk_D{D}_E{E}_{precision}_score_err", err)
    assert err <= 1e-5 and is_contract_ordered(got_scores, got_rows), what
    again_scores, again_rows = topk_ex(x, stored, inv, k, precision, chunk)
    assert torch.equal(again_rows, best) and same(again_scores, scores), what         # the same bits every run
    f32_scores, f32_rows = topk_ex(x, wide, inv, k, precision, chunk)                 # the twin with DRIN_FEAT_F32 ...
    old_scores, old_rows = topk_old(x, wide, inv, k, precision, chunk)
    assert torch.equal(f32_rows, old_rows) and same(f32_scores, old_scores), what     # ... is the old entry point
    if precision == "f32":                                               # the same kernel reads the same values: the same list
        assert torch.equal(best, old_rows) and same(scores, old_scores), what
    one_scores, one_rows = topk_ex(x, stored, inv, k, precision, E)      # one chunk | chunked: the same list
    assert torch.equal(one_rows, best) and same(one_scores, scores), what
    if not as_planes:
        # the widen route in EITHER precision: the same kernel reads the same values as on fp32 rows, so each chunking equals
        # drin_table_topk on the widened table under the same chunking, bit for bit (bf16x3 at D 16: chunks of 64 rows run the
        # exact fp32 kernel, one chunk of 300 the split-bf16 one - the host test asserts the margin that makes their lists equal)
        assert torch.equal(best, old_rows) and same(scores, old_scores), what
        whole_scores, whole_rows = topk_old(x, wide, inv, k, precision, E)
        assert torch.equal(one_rows, whole_rows) and same(one_scores, whole_scores), what
    assert same(table_topk(x, stored, inv, k, EPS, precision, chunk).scores, scores)


# ---- drin_table_topk_sum_ex -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("storage", ["mixed", "all", "dropped"])
def test_table_topk_sum_on_bf16_tables_links_as_the_widened_tables(storage, precision):
    c = SUM_CASE
    xs, tables = sum_case()
    weights = (c["weights"][0], 0.0, c["weights"][2]) if storage == "dropped" else c["weights"]
    k, chunk, E = c["k"], c["chunk"], c["E"]
    xs_t, wide_t = [dev(x) for x in xs], [dev(t) for t in tables]
    as_bf16 = (True, False, True) if storage == "mixed" else (True, True, True)       # tt bf16, ti f32, it bf16 | all bf16
    stored_t = [w.to(BF) if b else w for w, b in zip(wide_t, as_bf16)]
    invs = [inv_norms_ex(t) for t in stored_t]
    terms = [(x, t, i, w) for x, t, i, w in zip(xs_t, stored_t, invs, weights)]
    if storage == "dropped":
        terms[1] = (None, None, None, 0.0)                               # NULL pointers: nothing of the term is read
    what = f"sum {storage} {precision}"
    got = table_topk_sum(terms, k, EPS, precision, chunk)
    got_rows, got_scores = got.rows.cpu().numpy(), got.scores.cpu().numpy()
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    cosines = [indexed_ex(x, t, got.rows).cpu().numpy() for x, t in zip(xs_t, stored_t)]
    assert np.array_equal(got_scores.view(np.uint32), chain32(cosines, weights).view(np.uint32)), what     # the documented chain
    ref = sum64(xs, tables, weights)
    err = float(np.abs(got_scores - np.take_along_axis(ref, got_rows, 1)).max())
    print(f"{what}: max |returned score - fp64| = {err:.3e} (bar {tol_of(weights, 'f32'):.1e})")
    record(f"sum_{storage}_{precision}_score_err", err)
    assert err <= tol_of(weights, "f32"), what
    holds_sum_rule(ref, got_rows, k, tol_of(weights, precision), c["cap"], what)
    assert is_contract_ordered(got_scores, got_rows), what
    again = table_topk_sum(terms, k, EPS, precision, chunk)
    assert torch.equal(again.rows, got.rows) and same(again.scores, got.scores), what
    wide_terms = [(None, None, None, 0.0) if t[0] is None else (t[0], w, t[2], t[3]) for t, w in zip(terms, wide_t)]
    want = table_topk_sum(wide_terms, k, EPS, precision, chunk)          # all fp32: the wrapper takes the old entry point
    if precision == "f32":                                               # the fp32 call on the widened tables, bit for bit
        assert torch.equal(got.rows, want.rows) and same(got.scores, want.scores), what
    # the twin itself with every dtype DRIN_FEAT_F32 is the old entry point: its workspace bytes, its bits
    lib, S = _lib.load(), len(wide_terms)
    arr, dts = (_lib.DrinTopkTermC * S)(), (C.c_int32 * S)(*[F32] * S)
    for a, (x, t, i, w) in zip(arr, wide_terms):
        a.weight = w
        if w != 0.0:
            a.x, a.rows, a.row_inv_norms, a.width = x.data_ptr(), t.data_ptr(), i.data_ptr(), x.shape[1]
    B = xs_t[0].shape[0]
    nbytes = lib.drin_table_topk_sum_workspace_bytes_ex(arr, dts, S, B, E, k, chunk, PRECISION[precision])
    assert nbytes == lib.drin_table_topk_sum_workspace_bytes(arr, S, B, E, k, chunk) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ex_scores, ex_rows = torch.full((B, k), 7.0, device=DEV), torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.drin_table_topk_sum_ex(arr, dts, S, E, B, k, EPS, PRECISION[precision], chunk, ptr(ws), nbytes, ptr(ex_scores),
                                          ptr(ex_rows), stream()))
    assert torch.equal(ex_rows, want.rows) and same(ex_scores, want.scores), what


def test_table_topk_sum_refuses_rows_it_cannot_read_in_place():
    x, rows = randn(3, 16, seed=1), randn(50, 16, seed=2).to(BF)
    inv = row_inv_norms(rows, EPS)
    for bad_rows in (rows.half(), rows.double(), randn(50, 32, seed=3).to(BF)[:, :16]):
        with pytest.raises(ValueError, match="term 0: rows must be a contiguous float32 .*or bfloat16"):
            table_topk_sum([(x, bad_rows, inv, 1.0)], 5, EPS, "f32")
    with pytest.raises(ValueError, match="term 0: rows must be .* on the GPU"):
        table_topk_sum([(x, rows.cpu(), inv, 1.0)], 5, EPS, "f32")


# ---- Model.link on bf16-stored features and tables ------------------------------------------------------------------------------------
def link_models(precision):
    c, table, mention = stored_case()
    model = Model(c["cfg"], precision=precision).to(DEV)
    model.load_state_dict(c["sd"])
    model.eval()
    model.validate_indices = True
    on = lambda v: [t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)   # noqa: E731
    widened = c["table"].to(DEV)
    widened.text, widened.image, widened.object = table.text.float().to(DEV), table.image.float().to(DEV), table.object.float().to(DEV)
    widened.set_clip(table.clip_text.float(), table.clip_image.float())
    wide_mention = [m.float() if m.dtype == BF else m for m in on(mention)]
    return c, model, table.to(DEV), on(mention), widened, wide_mention, on(c["candidates"]), on(c["clip_image"]), on(c["clip_text"])


def check_link(model, got, mention, table, cand, clip_image, clip_text, k):
    """the result is drin_rank_rows over the model's own forward on the same candidates"""
    with torch.no_grad():
        own = model(IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)).cpu().numpy()
    rows, scores, cand_h = got.rows.cpu().numpy(), got.scores.cpu().numpy(), cand.cpu().numpy()
    for b in range(cand_h.shape[0]):
        slots = rank_order(own[b], cand_h[b])[:k]
        assert np.array_equal(rows[b], cand_h[b, slots]), b
        assert np.array_equal(scores[b].view(np.uint32), canonical(own[b, slots])), b


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_model_link_on_bf16_storage_in_its_three_forms(precision):
    c, model, table, mention, widened, wide_mention, cand, clip_image, clip_text = link_models(precision)
    cfg, k = c["cfg"], K_LINK
    N, E = cfg.num_candidates_model, table.num_entities
    assert table.text.dtype == BF and table.clip_text.dtype == BF and mention[0].dtype == BF
    # (a) candidates=: the CLIP edges from the bf16 tables are the bits of the widened tables', the forward is the bf16 table's own
    batch = IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)
    wide_batch = IndexedBatch.from_clip(wide_mention, widened, cand, clip_image, clip_text, model=model)
    assert same(batch.miet_similarity, wide_batch.miet_similarity) and same(batch.mtei_similarity, wide_batch.mtei_similarity)
    got = model.link(mention, table, k, clip_image, clip_text, candidates=cand)
    check_link(model, got, mention, table, cand, clip_image, clip_text, k)
    with torch.no_grad():                                               # the second stage: the forward on the bf16 table, route "prepared"
        apart = (model(batch) - model(wide_batch)).abs().max().item()
    print(f"Model.link {precision}: max |forward(bf16 storage) - forward(widened copies)| = {apart:.3e} (each within {TOL[precision]:g} of fp64)")
    record(f"link_{precision}_forward_bf16_vs_widened", apart)
    assert apart <= 2 * TOL[precision]                                  # both are within the bar of the fp64 oracle on the same values
    # (b) rows=: a bf16 first-stage table, read in place
    g = torch.Generator().manual_seed(4)
    queries, rows = torch.randn(3, 16, generator=g).to(DEV), torch.randn(E, 16, generator=g).to(DEV).to(BF)
    got = model.link(mention, table, k, clip_image, clip_text, queries=queries, rows=rows)
    name = "f32" if precision == "f32" else "bf16x3"
    first = table_topk(queries, rows, row_inv_norms(rows, cfg.cosine_eps), N, cfg.cosine_eps, name).rows
    check_link(model, got, mention, table, first, clip_image, clip_text, k)
    assert model._link_inv[3].dtype == BF and model._link_inv[3].data_ptr() == rows.data_ptr()       # no copy of the table was made
    if precision == "f32":
        wide_first = table_topk(queries, rows.float(), row_inv_norms(rows.float(), cfg.cosine_eps), N, cfg.cosine_eps, name).rows
        assert torch.equal(first, wide_first)
    # (c) first_stage="edges": DRIN lists its own candidates from the bf16 text and CLIP tables
    got = model.link(mention, table, k, clip_image, clip_text, first_stage="edges")
    listed = model._edge_candidates(mention, table, clip_image, clip_text, None)
    assert tuple(listed.shape) == (3, N)
    check_link(model, got, mention, table, listed, clip_image, clip_text, k)
    assert all(entry[3].dtype == BF for entry in model._link_edges_inv.values()) and len(model._link_edges_inv) == 3
    if precision == "f32":                                               # the same call on the widened copies lists the same rows
        model.invalidate()
        wide_listed = model._edge_candidates(wide_mention, widened, clip_image, clip_text, None)
        assert torch.equal(listed, wide_listed)
        model.invalidate()
    # the span positions in another integer dtype (the converted copies must live across the launch), and on the host: the same rows
    odd = [mention[0], mention[1], mention[2].to(torch.int32), mention[3].to(torch.int32)] + mention[4:]
    assert torch.equal(model._edge_candidates(odd, table, clip_image, clip_text, None), listed)
    tt = model._span_mean_stored(mention[0], mention[2], mention[3])
    assert same(model._span_mean_stored(mention[0], mention[2].to(torch.int32), mention[3].to(torch.int16)), tt)
    assert same(model._span_mean_stored(mention[0], mention[2].cpu().to(torch.int32), mention[3].cpu()), tt)
    assert torch.isfinite(tt).all() and tuple(tt.shape) == (3, cfg.bert_embed_dim)
    want_tt = torch.stack([mention[0][b, int(mention[2][b]):int(mention[3][b])].double().mean(0) for b in range(3)])
    assert (tt.double() - want_tt).abs().max().item() <= 1e-5 * want_tt.abs().max().item()
    # a zero tt weight leaves the bf16 text untouched: the CLIP terms alone, whatever stands in the text tensors
    no_tt = model._edge_candidates(mention, table, clip_image, clip_text, (0.0, 1.0, 1.0))
    poisoned = [torch.full_like(mention[0], float("nan"))] + mention[1:]
    assert torch.equal(model._edge_candidates(poisoned, table, clip_image, clip_text, (0.0, 1.0, 1.0)), no_tt)
    assert 0 not in model._link_edges_inv or model._link_edges_inv[0][3].dtype == BF
    # the per-entity cache is built from fp32 tables only: a bf16 table with the cache enabled keeps its ValueError
    table.enable_cache()
    with pytest.raises(ValueError, match="fp32 tables"):
        model.link(mention, table, k, clip_image, clip_text, candidates=cand)
    table.enable_cache(False)
