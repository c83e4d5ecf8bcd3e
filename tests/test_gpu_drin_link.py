"""-m gpu: DRIN behind a first stage.  `drin_cross_modal_edges` bit for bit against `scale *
drin_cosine_rows_indexed_fwd` and against fp64 at every width band and grid shape; `drin_rank_rows` exactly against the restated
contract order; and through the model - `IndexedBatch.from_clip` scored on every route against the fp64 oracle, `Model.link` by
the rule of section 24.  The restatements and the CPU cases: tests/drin_link_restatement.py.  Every test prints its maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk
from drin_amd.model import IndexedBatch, Model
from tests.drin_link_restatement import CASES, K_LINK, TOL, canonical, cos64, expected_rank, link_case, near_threshold, rank_order

pytestmark = pytest.mark.gpu

DEV = "cuda"
KERNEL_TOL = 1e-5                      # the bar tests/test_gpu_step_kernels.py puts on drin_cosine_rows_fwd: x max |ref|
SCALE, EPS, E_ROWS = 100.0, 1e-8, 7
CANARY = 12345.678
PAD = 8
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)   # noqa: E731


def canaried(shape, dtype=torch.float32, fill=CANARY):
    """`(whole, view)`: a buffer with PAD canary elements on either side of the `shape` view, all filled with the canary"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return whole, whole[PAD:PAD + n].view(*shape)


def canaries_intact(whole, fill=CANARY):
    ref = torch.full((PAD,), fill, dtype=whole.dtype, device=DEV)
    return torch.equal(whole[:PAD], ref) and torch.equal(whole[-PAD:], ref)


# ---- drin_cross_modal_edges -------------------------------------------------------------------------------------------------------
WIDTHS = [4, 64, 256, 260, 512, 516, 1028]            # D4 = 1, 16, 64 | 65, 128 | 129, 257: both register bands and the any-width form
GRIDS = [(1, 1), (1, 3), (3, 5), (2, 11), (5, 33)]
LONG = (900, 41)                                       # enough waves that one takes several trips, the last one partly idle


def edge_inputs(B, N, width, seed):
    g = torch.Generator().manual_seed(seed)
    t_text, t_image = torch.randn(E_ROWS, width, generator=g), torch.randn(E_ROWS, width, generator=g)
    m_image, m_text = torch.randn(B, width, generator=g), torch.randn(B, width, generator=g)
    index = torch.randint(0, E_ROWS, (B, N), generator=g)             # N > 7 repeats rows; smaller lists often do
    return [t.to(DEV) for t in (m_image, m_text, t_text, t_image, index)]


def run_edges(m_image, m_text, t_text, t_image, index, miet=True, mtei=True, status=None):
    """the call on canaried outputs; an edge left out passes NULL for its three pointers and keeps a canaried buffer to look at"""
    B, N = index.shape
    wi, oi = canaried((B, N))
    wt, ot = canaried((B, N))
    _lib.check(_lib.load().drin_cross_modal_edges(
        ptr(m_image) if miet else None, ptr(m_text) if mtei else None, ptr(t_text) if miet else None, ptr(t_image) if mtei else None,
        ptr(index), t_text.shape[0], B, N, m_image.shape[1], SCALE, EPS, ptr(oi) if miet else None, ptr(ot) if mtei else None,
        ptr(status), stream()))
    torch.cuda.synchronize()
    assert canaries_intact(wi) and canaries_intact(wt)
    return wi, oi, wt, ot


def two_call_route(m_image, m_text, t_text, t_image, index):
    scale = torch.tensor(SCALE, dtype=torch.float32, device=DEV)
    return (scale * cosine_rows_indexed(m_image, t_text, index, EPS, None), scale * cosine_rows_indexed(m_text, t_image, index, EPS, None))


def check_edges(B, N, width):
    ins = edge_inputs(B, N, width, 1000 * width + 10 * N + B)
    before = [t.clone() for t in ins]
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    _wi, miet, _wt, mtei = run_edges(*ins, status=status)
    assert all(torch.equal(a, b) for a, b in zip(ins, before)) and status.tolist() == [0, 0, 0, 0]
    ref_i, ref_t = two_call_route(*ins)
    assert torch.equal(bits(miet), bits(ref_i)) and torch.equal(bits(mtei), bits(ref_t))           # exact: one fp32 multiply apart
    m_image, m_text, t_text, t_image, index = [t.cpu() for t in ins]
    for name, got, ref in (("miet", miet, cos64(m_image, t_text, index, SCALE, EPS)), ("mtei", mtei, cos64(m_text, t_image, index, SCALE, EPS))):
        err, top = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"cross-modal edges ({B},{N},{width}) {name}: max err {err:.2e} of max |ref| {top:.2e}")
        assert err <= KERNEL_TOL * top
    # one edge alone: the same bits, the absent output untouched (run_edges looks at the canaries around both)
    wi, only_i, wt, none_t = run_edges(*ins, mtei=False)
    assert torch.equal(bits(only_i), bits(miet)) and torch.equal(none_t, torch.full_like(none_t, CANARY))
    wi, none_i, wt, only_t = run_edges(*ins, miet=False)
    assert torch.equal(bits(only_t), bits(mtei)) and torch.equal(none_i, torch.full_like(none_i, CANARY))
    # two runs give the same bits
    _wi, again_i, _wt, again_t = run_edges(*ins)
    assert torch.equal(bits(again_i), bits(miet)) and torch.equal(bits(again_t), bits(mtei))


@pytest.mark.parametrize("B,N", GRIDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_cross_modal_edges_are_the_scaled_indexed_cosine_bits(width, B, N):
    check_edges(B, N, width)


@pytest.mark.parametrize("width", [64, 516, 1028])
def test_cross_modal_edges_over_several_trips_per_wave(width):
    check_edges(*LONG, width)


def test_cross_modal_edges_zero_rows_give_exactly_zero():
    ins = edge_inputs(3, 11, 260, 5)
    ins[2][2].zero_()                                                   # a zero table text row
    ins[3][4].zero_()                                                   # a zero table image row
    ins[1][1].zero_()                                                   # a zero mention text row
    index = ins[4]
    index[0, 0], index[2, 10], index[1, 3] = 2, 2, 4
    _wi, miet, _wt, mtei = run_edges(*ins)
    assert (miet[index == 2] == 0).all() and (index == 2).sum() >= 2 and not torch.isnan(miet).any()
    assert (mtei[index == 4] == 0).all() and (mtei[1] == 0).all() and not torch.isnan(mtei).any()
    assert torch.count_nonzero(miet[index != 2]) == (index != 2).sum()


@pytest.mark.parametrize("B,N,b,n,bad", [(3, 5, 2, 4, -1), (3, 5, 0, 0, E_ROWS), (1, 3, 0, 2, E_ROWS), (5, 33, 4, 32, -1), (2, 11, 1, 5, 1 << 40)])
def test_cross_modal_edges_clamp_and_report_a_bad_index(B, N, b, n, bad):
    ins = edge_inputs(B, N, 64, 9)
    ins[4][b, n] = bad
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    _wi, miet, _wt, mtei = run_edges(*ins, status=status)
    w = status.tolist()
    value = ((w[3] & 0xFFFFFFFF) << 32 | (w[2] & 0xFFFFFFFF))
    value -= (1 << 64) if value >= (1 << 63) else 0
    assert w[0] == 1 and w[1] == b * N + n and value == bad, w
    clamped = ins[:4] + [ins[4].clamp(0, E_ROWS - 1)]
    _wi, ref_i, _wt, ref_t = run_edges(*clamped)
    assert torch.equal(bits(miet), bits(ref_i)) and torch.equal(bits(mtei), bits(ref_t))           # the clamped row was scored
    _wi, quiet_i, _wt, _t = run_edges(*ins, status=None)                                           # NULL status: clamped silently
    assert torch.equal(bits(quiet_i), bits(ref_i))


# ---- drin_rank_rows ----------------------------------------------------------------------------------------------------------------
PATTERNS = ("equal", "nans", "zeros_infs", "dups", "descending", "ascending")
ROW_CANARY, SLOT_CANARY = -77, -55


def rank_row(pattern, n, r):
    """one mention's (scores float32 [n], rows int64 [n]); rows are distinct except for "dups", negative and past 2^33 among them"""
    rows = (r.permutation(3 * n)[:n].astype(np.int64) - n) * ((1 << 33) + 1)
    if pattern == "equal":
        scores = np.full(n, 1.5, dtype=np.float32)
    elif pattern == "nans":
        scores = np.round(r.standard_normal(n), 1).astype(np.float32)
        scores[r.random(n) < 0.3] = np.nan
        scores[r.random(n) < 0.1] = np.float32(-np.nan)
        if n > 1:
            scores.view(np.uint32)[0] = 0x7FA00001                     # a signalling payload: all NaNs are equal
    elif pattern == "zeros_infs":
        scores = r.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32), n)
    elif pattern == "dups":
        rows = r.integers(0, max(1, n // 3), n).astype(np.int64)
        scores = r.choice(np.array([0.5, 1.0], dtype=np.float32), n)
    elif pattern == "descending":
        scores = (n - np.arange(n)).astype(np.float32)
    else:
        scores = np.arange(n).astype(np.float32)
    return scores, rows


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 101, 1001, 1024, 1025, 4096])
def test_rank_rows_is_the_restated_order(n, B):
    lib, r = _lib.load(), np.random.default_rng(100 * n + B)
    for first in range(len(PATTERNS)):
        made = [rank_row(PATTERNS[(first + b) % len(PATTERNS)], n, r) for b in range(B)]
        scores, rows = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
        ds, dr = torch.from_numpy(scores).to(DEV), torch.from_numpy(rows).to(DEV)
        for k in sorted({1, min(n, 10), n}):
            want_bits, want_rows, want_slots = expected_rank(scores, rows, k)
            for with_slots in (False, True):
                ws, os_ = canaried((B, k))
                wr, or_ = canaried((B, k), torch.int64, ROW_CANARY)
                wl, ol = canaried((B, k), torch.int32, SLOT_CANARY)
                _lib.check(lib.drin_rank_rows(ptr(ds), ptr(dr), B, n, k, ptr(os_), ptr(or_), ptr(ol) if with_slots else None, stream()))
                torch.cuda.synchronize()
                assert canaries_intact(ws) and canaries_intact(wr, ROW_CANARY) and canaries_intact(wl, SLOT_CANARY)
                what = (PATTERNS[first], n, B, k, with_slots)
                assert np.array_equal(os_.cpu().numpy().view(np.uint32), want_bits), what
                assert np.array_equal(or_.cpu().numpy(), want_rows), what
                if with_slots:
                    assert np.array_equal(ol.cpu().numpy(), want_slots), what
                else:
                    assert (ol == SLOT_CANARY).all(), what
        assert np.array_equal(ds.cpu().numpy().view(np.uint32), scores.view(np.uint32)) and np.array_equal(dr.cpu().numpy(), rows)


# ---- through the model ----------------------------------------------------------------------------------------------------------
ROUTES = [(name, cached) for name in sorted(CASES) for cached in (False, True)]


def gpu_case(name, cached, precision):
    c = link_case(name)
    table = c["table"].to(DEV)
    if cached:
        table.enable_cache()
    model = Model(c["cfg"], precision=precision).to(DEV)
    model.load_state_dict(c["sd"])
    model.eval()
    model.validate_indices = True
    on = lambda k: [t.to(DEV) for t in c[k]] if isinstance(c[k], list) else c[k].to(DEV)   # noqa: E731
    return c, model, table, on("mention"), on("candidates"), on("clip_image"), on("clip_text")


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name,cached", ROUTES)
def test_from_clip_batches_score_inside_the_bars_on_every_route(name, cached, precision):
    c, model, table, mention, cand, clip_image, clip_text = gpu_case(name, cached, precision)
    assert table.clip_text is not None and table.clip_text.device.type == "cuda"                   # to() moved the CLIP rows
    batch = IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)
    assert isinstance(batch, IndexedBatch) and tuple(batch.miet_similarity.shape) == tuple(cand.shape)
    for got, ref, what in ((batch.miet_similarity, c["miet"], "miet"), (batch.mtei_similarity, c["mtei"], "mtei")):
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"{name} {what}: max err {err:.2e} of max |ref| {ref.abs().max().item():.2e}")
        assert err <= KERNEL_TOL * ref.abs().max().item()
    with torch.no_grad():
        scores = model(batch)
    worst = (scores.double().cpu() - c["ref"]).abs().max().item()
    print(f"{name} cached={cached} {precision}: max |scores - fp64 oracle| = {worst:.3e} (bar {TOL[precision]:g})")
    assert scores.dtype == torch.float32 and tuple(scores.shape) == tuple(cand.shape) and worst <= TOL[precision]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name,cached", ROUTES)
def test_link_returns_the_best_candidates_by_the_models_own_scores(name, cached, precision):
    c, model, table, mention, cand, clip_image, clip_text = gpu_case(name, cached, precision)
    ref, tol, k = c["ref"], TOL[precision], K_LINK
    assert near_threshold(ref, k, tol) <= 2                             # on the oracle's scores alone
    got = model.link(mention, table, k, clip_image, clip_text, candidates=cand)
    assert tuple(got.scores.shape) == (cand.shape[0], k) == tuple(got.rows.shape) and got.rows.dtype == torch.int64
    with torch.no_grad():
        own = model(IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)).cpu().numpy()
    rows, scores, cand_h = got.rows.cpu().numpy(), got.scores.cpu().numpy(), c["candidates"].numpy()
    for b in range(cand_h.shape[0]):
        slots = [int(np.nonzero(cand_h[b] == row)[0][0]) for row in rows[b]]          # no row repeats inside a mention
        assert len(set(slots)) == k
        t = torch.sort(ref[b], descending=True).values[k - 1].item()
        assert all(ref[b, s].item() >= t - tol for s in slots), (b, slots)
        assert set(np.nonzero(ref[b].numpy() > t + tol)[0].tolist()) <= set(slots), (b, slots)
        assert np.array_equal(scores[b].view(np.uint32), canonical(own[b, slots])), b   # the forward's own bits at those slots
        assert np.array_equal(rank_order(scores[b], rows[b]), np.arange(k)), b          # contract-ordered
        assert np.array_equal(np.array(slots), rank_order(own[b], cand_h[b])[:k]), b    # and THE first k of the forward's scores


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_link_with_a_cosine_first_stage_is_link_on_its_rows(precision):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", True, precision)
    N, E = c["cfg"].num_candidates_model, table.num_entities
    g = torch.Generator().manual_seed(4)
    queries, rows = torch.randn(3, 16, generator=g).to(DEV), torch.randn(E, 16, generator=g).to(DEV)
    got = model.link(mention, table, K_LINK, clip_image, clip_text, queries=queries, rows=rows)
    first = table_topk(queries, rows, row_inv_norms(rows, c["cfg"].cosine_eps), N, c["cfg"].cosine_eps, precision).rows
    assert tuple(first.shape) == (3, N)
    same = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=first)
    assert torch.equal(got.rows, same.rows) and torch.equal(bits(got.scores), bits(same.scores))
    inv = model._link_inv[1]
    model.link(mention, table, K_LINK, clip_image, clip_text, queries=queries, rows=rows)
    assert model._link_inv[1] is inv                                    # cached per `rows` version ...
    rows.mul_(1.0)
    model.link(mention, table, K_LINK, clip_image, clip_text, queries=queries, rows=rows)
    assert model._link_inv[1] is not inv                                # ... and rebuilt when it moves


def test_link_first_stage_norms_follow_a_strided_or_replaced_rows_tensor():
    """The inverse norms of the first stage are cached per version of the CALLER's tensor, which the entry keeps alive: a
    non-contiguous `rows` (its contiguous copy is made per entry, not per call) edited in place, and a `rows` tensor that is
    dropped and replaced by a new one of the same shape, both get fresh norms - checked on the cached norms themselves and on the
    result against `link(candidates=)` fed with `drin_table_topk`'s rows of the current values."""
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", False, "f32")
    N, E, eps = c["cfg"].num_candidates_model, table.num_entities, c["cfg"].cosine_eps
    g = torch.Generator().manual_seed(6)
    queries = torch.randn(3, 16, generator=g).to(DEV)

    def agrees(rows):
        got = model.link(mention, table, K_LINK, clip_image, clip_text, queries=queries, rows=rows)
        dense = rows.contiguous()
        fresh = row_inv_norms(dense, eps)
        assert torch.equal(bits(model._link_inv[1]), bits(fresh))
        first = table_topk(queries, dense, fresh, N, eps, "f32").rows
        want = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=first)
        assert torch.equal(got.rows, want.rows) and torch.equal(bits(got.scores), bits(want.scores))

    big = torch.randn(E, 32, generator=g).to(DEV)
    strided = big[:, :16]
    assert not strided.is_contiguous()
    agrees(strided)
    held = model._link_inv[1]
    agrees(big[:, :16])                                                 # another view object of the same storage and version
    assert model._link_inv[1] is held
    big.mul_(torch.rand(E, 1, generator=g).to(DEV) * 8 + 0.125)         # every row's norm moves, through the base tensor
    agrees(strided)
    assert model._link_inv[1] is not held
    for seed in (1, 2, 3):                                              # dropped and replaced: same shape, a fresh tensor each time
        rows = torch.randn(E, 16, generator=torch.Generator().manual_seed(seed)).to(DEV)
        agrees(rows)
        del rows
    rows = torch.randn(E, 16, generator=g).to(DEV)
    agrees(rows)
    rows.data.mul_(torch.rand(E, 1, generator=g).to(DEV) + 0.5)         # a write the version counter does not see ...
    model.invalidate()                                                  # ... needs this call, as for the weights
    agrees(rows)


def test_from_clip_slices_and_empty_batches(monkeypatch):
    c, model, table, mention, cand, clip_image, clip_text = gpu_case("wm", False, "bf16x3")
    whole = IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)
    calls, lib = [], _lib.load()
    real = lib.drin_cross_modal_edges
    monkeypatch.setattr(lib, "drin_cross_modal_edges", lambda *a: (calls.append(a[6]), real(*a))[1])
    monkeypatch.setattr(Model, "MAX_CALL_MENTIONS", 2)
    sliced = IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)
    assert calls == [2, 1]
    assert torch.equal(bits(sliced.miet_similarity), bits(whole.miet_similarity))
    assert torch.equal(bits(sliced.mtei_similarity), bits(whole.mtei_similarity))
    got, ref = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=cand), None
    monkeypatch.undo()
    ref = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=cand)
    # (a mention's scores in calls of different sizes agree to fp32 re-association, <= 5e-6 - Model.MAX_CALL_MENTIONS - and the
    #  k-th largest of a list moves by no more than its entries do)
    assert (got.scores - ref.scores).abs().max().item() <= 1e-5
    empty = IndexedBatch.from_clip([t[:0] for t in mention], table, cand[:0], clip_image[:0], clip_text[:0], model=model)
    assert tuple(empty.miet_similarity.shape) == (0, cand.shape[1]) == tuple(empty.mtei_similarity.shape)
    none = model.link([t[:0] for t in mention], table, K_LINK, clip_image[:0], clip_text[:0], candidates=cand[:0])
    assert tuple(none.scores.shape) == (0, K_LINK) == tuple(none.rows.shape)


def test_from_clip_reports_a_candidate_outside_the_table():
    c, model, table, mention, cand, clip_image, clip_text = gpu_case("wm", False, "bf16x3")
    bad = cand.clone()
    bad[1, 2] = table.num_entities
    with pytest.raises(IndexError, match=f"row {table.num_entities} at pair {1 * cand.shape[1] + 2}"):
        IndexedBatch.from_clip(mention, table, bad, clip_image, clip_text, model=model)           # validate_indices: at once
    model.check_indices()                                               # the words were zeroed by the raise
    with pytest.raises(IndexError, match="row -1 at pair 0"):
        bad[1, 2], bad[0, 0] = 0, -1
        IndexedBatch.from_clip(mention, table, bad, clip_image, clip_text)                        # without a model: checked here
    model.validate_indices = False
    IndexedBatch.from_clip(mention, table, bad, clip_image, clip_text, model=model)               # watched, not waited for
    with pytest.raises(IndexError, match="row -1 at pair 0"):
        model.check_indices()
