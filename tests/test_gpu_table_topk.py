"""-m gpu: the cosine top-k against the whole entity table (csrc/table_topk.hip).

The selection alone (`drin_topk_update`) is held to the ordering contract of include/drin_hip.h EXACTLY, against a numpy
restatement, on crafted blocks with ties, NaN, infinities and signed zeros, whatever way the columns are cut into calls.  The
whole call (`drin_table_topk`) is held to fp64 by the project's score bars (1e-4 bf16x3, 1e-5 f32; DESIGN.md sections 15, 22,
23): every returned row scores at least t - tol and every row above t + tol is returned, t the k-th largest fp64 cosine; its
scores are the bits of `drin_cosine_rows_indexed_fwd` on its rows.  Then planted answers, degenerate rows, the write footprint,
`drin_ghmfc_mention_forward` against `drin_ghmfc_forward`'s mention_repr, and `model.link` on the three GHMFC classes.
Set GHMFC_LINK_PARITY_OUT to a path to have the measured maxima written there as JSON (profiles/ghmfc_link_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc_table import GhmfcIndexedBatch, LinkResult
from drin_amd.metrics import link_recall
from drin_amd.model import EntityTable
from tests.ghmfc_inputs import ghmfc_inputs, geometry
from tests.ghmfc_table_inputs import entity_table, rng, table_case
from tests.test_ghmfc_host import as_tensors, case_model
from tests.test_gpu_ghmfc_table import make_model, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
PRECISION = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
S = _lib.TOPK_SLICE
EPS = 1e-8
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
dev = lambda a, dtype=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)   # noqa: E731
kp_of = lambda k: 64 if k <= 64 else (128 if k <= 128 else 256)   # noqa: E731


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def contract_order(keys: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """the permutation that sorts (key, row) pairs by the contract: higher key first, NaN below -inf and all NaNs equal,
    -0.0 == +0.0, the lower row between equal keys"""
    nan = np.isnan(keys)
    return np.lexsort((rows, -np.where(nan, 0.0, keys.astype(np.float64)), nan))    # the LAST key is the primary one


def is_contract_ordered(scores: np.ndarray, rows: np.ndarray) -> bool:
    return all(np.array_equal(contract_order(scores[b], rows[b]), np.arange(scores.shape[1])) for b in range(scores.shape[0]))


# ---- 1. the selection alone, exact -----------------------------------------------------------------------------------------------
def crafted_block(cols: int, with_inv: bool):
    """dots [3, cols] float32 and inv [cols] (or None).  Mention 0: values rounded to one decimal (many ties) with NaN, +-inf and
    +-0.0 planted; mention 1: one value everywhere; mention 2: random, its maximum planted again in every later slice and at the
    last column.  inv: positive, a few of them the 1e8 of an eps-clamped row - one of those under a negative dot."""
    r = rng(f"topk_{cols}_{with_inv}", 1)
    dots = r.standard_normal((3, cols), dtype=np.float32)
    dots[0] = np.round(dots[0], 1)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0, 0.0]
    for i, pos in enumerate(r.permutation(cols)[:len(special)]):
        dots[0, pos] = special[i]
    dots[1] = 1.5
    top = np.float32(dots[2].max() + 1.0)
    for pos in list(range(cols // 3, cols, S)) + [cols - 1]:
        dots[2, pos] = top
    inv = None
    if with_inv:
        inv = (0.5 + r.random(cols, dtype=np.float32)).astype(np.float32)
        big = r.permutation(cols)[:3]
        inv[big] = np.float32(1e8)
        dots[2, big[0]] = np.float32(-0.75)
        dots[0, big[-1]] = np.float32(0.0)
    return dots, inv


def expected_topk(dots, inv, k):
    keys = dots if inv is None else dots * inv[None, :]               # float32 x float32, as the kernel forms the key
    rows = np.arange(dots.shape[1], dtype=np.int64)
    order = np.stack([contract_order(keys[b], rows)[:k] for b in range(dots.shape[0])])
    return np.take_along_axis(keys, order, 1), order.astype(np.int64)


def feed(block_t, inv_t, B, cols, k, cuts, ld=4):
    """drin_topk_update over the column segments between `cuts`, in order; the finishing pass rides the last call"""
    lib, kp = _lib.load(), kp_of(k)
    keys = torch.full((B, kp), 7.0, device=DEV)
    rows = torch.full((B, kp), 7, dtype=torch.int64, device=DEV)
    longest = max(b - a for a, b in zip(cuts[:-1], cuts[1:]))
    scratch = torch.empty(-(-longest // S) * B * kp * 8, dtype=torch.uint8, device=DEV)
    out_keys = torch.full((B, k), 7.0, device=DEV)
    out_rows = torch.full((B, k), 7, dtype=torch.int64, device=DEV)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        done = b == cols
        inv_p = None if inv_t is None else C.c_void_p(inv_t.data_ptr() + 4 * a)
        _lib.check(lib.drin_topk_update(C.c_void_p(block_t.data_ptr() + 4 * ld * a), ld, B, b - a, a, inv_p, k, ptr(keys), ptr(rows),
                                        ptr(scratch), scratch.numel(), 1 if i == 0 else 0, ptr(out_keys) if done else None,
                                        ptr(out_rows) if done else None, stream()))
    return out_keys.cpu().numpy(), out_rows.cpu().numpy()


@pytest.mark.parametrize("with_inv", [False, True])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 5])
def test_selection_is_exact_however_the_columns_are_cut(cols, with_inv):
    B, ld = 3, 4
    dots, inv = crafted_block(cols, with_inv)
    padded = np.full((cols, ld), np.float32(3e38))                     # the padding column of the entity-major block is not read as a mention
    padded[:, :B] = dots.T
    block_t, inv_t = dev(padded), dev(inv)
    boundaries = [c for c in (1, 63, 64, 65, S - 1, S, S + 1) if c < cols]
    for k in (1, 5, 64, 100, 256):
        if k > cols:
            continue
        want_keys, want_rows = expected_topk(dots, inv, k)
        whole = feed(block_t, inv_t, B, cols, k, [0, cols])
        assert np.array_equal(whole[1], want_rows), f"rows, k={k}"
        assert np.array_equal(whole[0], want_keys, equal_nan=True), f"keys, k={k}"
        for what, cuts in (("one column per call", list(range(cols + 1))), ("cut at every boundary", [0] + boundaries + [cols])):
            got = feed(block_t, inv_t, B, cols, k, cuts)
            assert np.array_equal(got[1], whole[1]) and np.array_equal(got[0].view(np.int32), whole[0].view(np.int32)), f"{what}, k={k}"


def test_selection_in_any_call_order_and_on_an_all_equal_block():
    """columns fed back to front give the same list (ties still go to the lowest ROW, not to the first call), and the finishing
    call alone (cols = 0) returns what the last update would have"""
    B, ld, cols, k = 3, 4, 300, 64
    dots, inv = crafted_block(cols, True)
    dots[0] = -0.0                                                      # all equal, and equal to +0.0
    dots[0, 100:200] = 0.0
    padded = np.zeros((cols, ld), dtype=np.float32)
    padded[:, :B] = dots.T
    block_t, inv_t = dev(padded), dev(inv)
    want_keys, want_rows = expected_topk(dots, inv, k)
    assert np.array_equal(want_rows[0], np.arange(k))
    lib, kp = _lib.load(), kp_of(k)
    keys = torch.full((B, kp), 7.0, device=DEV)
    rows = torch.full((B, kp), 7, dtype=torch.int64, device=DEV)
    scratch = torch.empty(B * kp * 8, dtype=torch.uint8, device=DEV)
    segments = [(200, 300), (64, 200), (0, 64)]
    for i, (a, b) in enumerate(segments):
        _lib.check(lib.drin_topk_update(C.c_void_p(block_t.data_ptr() + 4 * ld * a), ld, B, b - a, a, C.c_void_p(inv_t.data_ptr() + 4 * a), k,
                                        ptr(keys), ptr(rows), ptr(scratch), scratch.numel(), 1 if i == 0 else 0, None, None, stream()))
    out_keys = torch.full((B, k), 7.0, device=DEV)
    out_rows = torch.full((B, k), 7, dtype=torch.int64, device=DEV)
    _lib.check(lib.drin_topk_update(None, 0, B, 0, 0, None, k, ptr(keys), ptr(rows), None, 0, 0, ptr(out_keys), ptr(out_rows), stream()))
    assert np.array_equal(out_rows.cpu().numpy(), want_rows) and np.array_equal(out_keys.cpu().numpy(), want_keys, equal_nan=True)


# ---- 2. the whole call against fp64 --------------------------------------------------------------------------------------------------
def cosine64(x, rows):
    x, rows = x.astype(np.float64), rows.astype(np.float64)
    nx, nr = np.maximum(np.sqrt((x * x).sum(1)), EPS), np.maximum(np.sqrt((rows * rows).sum(1)), EPS)
    return (x @ rows.T) / (nx[:, None] * nr[None, :])


def inv_norms(rows_t):
    out = torch.full((rows_t.shape[0],), 7.0, device=DEV)
    _lib.check(_lib.load().drin_row_inv_norms(ptr(rows_t), rows_t.shape[0], rows_t.shape[1], EPS, ptr(out), stream()))
    return out


def table_topk(x_t, rows_t, inv_t, k, precision, chunk):
    lib = _lib.load()
    (B, D), E = x_t.shape, rows_t.shape[0]
    nbytes = lib.drin_table_topk_workspace_bytes(B, E, D, k, chunk)
    assert nbytes > 0, lib.drin_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    scores = torch.full((B, k), 7.0, device=DEV)
    best = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.drin_table_topk(ptr(x_t), ptr(rows_t), ptr(inv_t), E, B, D, k, EPS, PRECISION[precision], chunk, ptr(ws), nbytes,
                                   ptr(scores), ptr(best), stream()))
    return scores, best


def indexed_cosine(x_t, rows_t, index_t):
    out = torch.full(tuple(index_t.shape), 7.0, device=DEV)
    _lib.check(_lib.load().drin_cosine_rows_indexed_fwd(ptr(x_t), ptr(rows_t), ptr(index_t), rows_t.shape[0], ptr(out), index_t.shape[0],
                                                        index_t.shape[1], x_t.shape[1], EPS, None, stream()))
    return out


def holds_rule(ref: np.ndarray, got_rows: np.ndarray, k: int, tol: float, what: str) -> None:
    """every returned row has ref >= t - tol, every row with ref > t + tol is returned; t = the k-th largest of ref.  First, so
    that the rule cannot hide a failure: at most 2 rows other than the k-th lie within tol of t."""
    for b in range(ref.shape[0]):
        t = np.sort(ref[b])[::-1][k - 1]
        assert int((np.abs(ref[b] - t) <= tol).sum()) - 1 <= 2, f"{what}: mention {b} has too many rows within {tol} of the k-th"
        assert (ref[b, got_rows[b]] >= t - tol).all(), f"{what}: mention {b} returned a row below t - tol"
        assert np.isin(np.nonzero(ref[b] > t + tol)[0], got_rows[b]).all(), f"{what}: mention {b} misses a row above t + tol"


_PARITY = {}


def record(key: str, value: float) -> None:
    _PARITY[key] = value
    out = os.environ.get("GHMFC_LINK_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(_PARITY.items())), f, indent=1)


_WHOLE = {}


def whole_case(D, E, B, seed=0):
    """x, rows from numpy's default_rng(seed).standard_normal and their fp64 cosines, computed once"""
    if (D, E, B, seed) not in _WHOLE:
        g = np.random.default_rng(seed)
        x = g.standard_normal((B, D)).astype(np.float32)
        rows = g.standard_normal((E, D)).astype(np.float32)
        _WHOLE[(D, E, B, seed)] = (x, rows, cosine64(x, rows))
    return _WHOLE[(D, E, B, seed)]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("D,E,B,k,chunk", [(16, 300, 3, 20, 64), (32, 1500, 4, 64, 256), (768, 2000, 5, 100, 0), (768, 2000, 5, 100, 512)])
def test_table_topk_against_fp64(D, E, B, k, chunk, precision):
    x, rows, ref = whole_case(D, E, B)
    x_t, rows_t = dev(x), dev(rows)
    inv_t = inv_norms(rows_t)
    want_inv = 1.0 / np.maximum(np.sqrt((rows.astype(np.float64) ** 2).sum(1)), EPS)
    # worst case of the <= 54 roundings of a lane's chain (12 dot4 of 4 terms) and the wave's tree, halved by the square root, plus
    # the root's and the reciprocal's own: (54 / 2 + 2) x 2^-24 = 1.7e-6
    assert np.abs(inv_t.cpu().numpy() / want_inv - 1.0).max() <= 2e-6
    scores, best = table_topk(x_t, rows_t, inv_t, k, precision, chunk)
    got_rows, got_scores = best.cpu().numpy(), scores.cpu().numpy()
    what = f"D{D} E{E} B{B} k{k} chunk{chunk} {precision}"
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    holds_rule(ref, got_rows, k, TOL[precision], what)
    assert same_bits(scores, indexed_cosine(x_t, rows_t, best)), what      # the bits of the cached table-form scoring
    assert is_contract_ordered(got_scores, got_rows), what
    err = float(np.abs(got_scores - np.take_along_axis(ref, got_rows, 1)).max())
    print(f"{what}: max |returned score - fp64| = {err:.3e}")
    record(f"D{D}_E{E}_B{B}_k{k}_chunk{chunk}/{precision}", err)
    again_scores, again_rows = table_topk(x_t, rows_t, inv_t, k, precision, chunk)
    assert torch.equal(again_rows, best) and same_bits(again_scores, scores), what   # the same bits every run


# ---- 3. planted answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("D,E,chunk", [(16, 300, 64), (32, 1500, 256)])
def test_planted_answers_rank_first(D, E, chunk, precision):
    x, rows, _ = whole_case(D, E, 3)
    x_t = dev(x)
    for place in (0, E - 1, chunk - 1, chunk):                          # the ends, the last row of a chunk, the first of the next
        for b in range(3):
            planted = rows.copy()
            planted[place] = np.float32(2.5) * x[b]
            copy_at = None if place == E - 1 else min(place + 1 + 37 * (b + 1), E - 1)
            if copy_at is not None:
                planted[copy_at] = planted[place]                       # the same key in another slice or chunk: the lower row first
            rows_t = dev(planted)
            scores, best = table_topk(x_t, rows_t, inv_norms(rows_t), 5, precision, chunk)
            assert best[b, 0].item() == place and abs(scores[b, 0].item() - 1.0) <= 1e-6, (place, b)
            if copy_at is not None:
                assert best[b, 1].item() == copy_at and scores[b, 1].item() == scores[b, 0].item(), (place, b)


# ---- 4. degenerate rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_degenerate_rows(precision):
    D, E, chunk, ZERO, NAN = 16, 70, 32, 7, 40
    x, rows, _ = whole_case(D, 300, 3)
    rows = rows[:E].copy()
    rows[ZERO] = 0.0
    rows[NAN, 3] = np.nan
    x = x.copy()
    x[2] = 0.0                                                          # an all-zero mention: every score is 0 (or NaN)
    x_t, rows_t = dev(x), dev(rows)
    inv_t = inv_norms(rows_t)
    assert inv_t[ZERO].item() == np.float32(1.0) / np.float32(EPS) and torch.isfinite(inv_t[ZERO])
    scores, best = table_topk(x_t, rows_t, inv_t, E, precision, chunk)   # k = E: every row appears
    for b in range(2):
        at = (best[b] == ZERO).nonzero().item()
        assert scores[b, at].item() == 0.0                               # through the eps clamp: 0 / (|x| eps), finite
        assert best[b, E - 1].item() == NAN and torch.isnan(scores[b, E - 1]) and torch.isfinite(scores[b, :E - 1]).all()
    assert best[2].tolist() == [e for e in range(E) if e != NAN] + [NAN] and bool((scores[2, :E - 1] == 0).all())
    scores, best = table_topk(x_t, rows_t, inv_t, E - 1, precision, chunk)
    assert not bool((best == NAN).any()) and torch.isfinite(scores).all()      # the NaN row appears only when k reaches it
    scores, best = table_topk(x_t, rows_t, inv_t, 10, precision, chunk)
    assert best[2].tolist() == list(range(10))


# ---- 5. nothing else is written ----------------------------------------------------------------------------------------------------
G = 4096


def canaried(nbytes: int):
    buf = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[G:G + nbytes]


def intact(buf, nbytes: int) -> bool:
    return bool((buf[:G] == 0xA5).all() and (buf[G + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("D,E,B,k,chunk", [(4, 1, 1, 1, 0), (16, 300, 3, 20, 64), (16, 300, 5, 65, 0)])
def test_table_topk_writes_only_its_outputs_and_workspace(D, E, B, k, chunk):
    lib = _lib.load()
    x, rows, _ = whole_case(D, E, B, seed=1)
    x_t, rows_t = dev(x), dev(rows)
    inv_buf, inv = canaried(E * 4)
    _lib.check(lib.drin_row_inv_norms(ptr(rows_t), E, D, EPS, ptr(inv), stream()))
    nbytes = lib.drin_table_topk_workspace_bytes(B, E, D, k, chunk)
    ws_buf, ws = canaried(nbytes)
    sc_buf, sc = canaried(B * k * 4)
    rw_buf, rw = canaried(B * k * 8)
    for precision in PRECISION.values():
        _lib.check(lib.drin_table_topk(ptr(x_t), ptr(rows_t), ptr(inv), E, B, D, k, EPS, precision, chunk, ptr(ws), nbytes, ptr(sc), ptr(rw),
                                       stream()))
    torch.cuda.synchronize()
    assert intact(inv_buf, E * 4) and intact(ws_buf, nbytes) and intact(sc_buf, B * k * 4) and intact(rw_buf, B * k * 8)
    assert torch.equal(dev(x), x_t) and torch.equal(dev(rows), rows_t)
    got = rw.view(torch.int64).reshape(B, k)
    assert got.min().item() >= 0 and got.max().item() <= E - 1
    # refusals launch nothing and write nothing
    sc.fill_(0x5A)
    assert lib.drin_table_topk(ptr(x_t), ptr(rows_t), ptr(inv), E, B, D, k, EPS, 1, chunk, ptr(ws), nbytes - 1, ptr(sc), ptr(rw), stream()) \
        == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((sc == 0x5A).all())


@pytest.mark.parametrize("B,cols,k", [(1, 1, 1), (3, S + 70, 100), (9, 200, 256)])
def test_topk_update_writes_only_its_state_scratch_and_outputs(B, cols, k):
    lib, kp, ld = _lib.load(), kp_of(k), -(-B // 4) * 4
    k = min(k, cols)
    block_t = dev(rng(f"guard_{B}_{cols}", 1).standard_normal((cols, ld), dtype=np.float32))
    sizes = dict(keys=B * kp * 4, rows=B * kp * 8, scratch=-(-cols // S) * B * kp * 8, out_keys=B * k * 4, out_rows=B * k * 8)
    bufs = {name: canaried(n) for name, n in sizes.items()}
    t = {name: bufs[name][1] for name in bufs}
    half = cols // 2
    if half:
        _lib.check(lib.drin_topk_update(ptr(block_t), ld, B, half, 0, None, k, ptr(t["keys"]), ptr(t["rows"]), ptr(t["scratch"]),
                                        sizes["scratch"], 1, None, None, stream()))
    _lib.check(lib.drin_topk_update(C.c_void_p(block_t.data_ptr() + 4 * ld * half), ld, B, cols - half, half, None, k, ptr(t["keys"]),
                                    ptr(t["rows"]), ptr(t["scratch"]), sizes["scratch"], 0 if half else 1, ptr(t["out_keys"]),
                                    ptr(t["out_rows"]), stream()))
    torch.cuda.synchronize()
    for name, n in sizes.items():
        assert intact(bufs[name][0], n), name
    dots = block_t.cpu().numpy()[:, :B].T
    want_keys, want_rows = expected_topk(np.ascontiguousarray(dots), None, k)
    assert np.array_equal(t["out_rows"].view(torch.int64).reshape(B, k).cpu().numpy(), want_rows)
    assert np.array_equal(t["out_keys"].view(torch.float32).reshape(B, k).cpu().numpy(), want_keys)


# ---- 6. the mention half alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["wd_b5", "wm_b3", "b300", "full_b4"])
def test_mention_forward_has_the_bits_of_the_forward(name, precision):
    lib, geo = _lib.load(), geometry(name)
    model = case_model(name, precision).to(DEV)
    batch = as_tensors(ghmfc_inputs(name), torch.float32, DEV)
    with torch.no_grad():
        want = model.encode_mentions(batch)                              # drin_ghmfc_forward's mention_repr
    mf, mmask, mimage = batch[0].contiguous(), batch[1].contiguous(), batch[4].contiguous()
    B, D = mf.shape[0], geo["D"]
    c = _lib.DrinGhmfcConfigC(batch=B, num_candidates=0, embed_dim=D, image_dim=geo["R"], mention_tokens=geo["L"], image_regions=geo["P"],
                              num_heads=geo["H"], entity_tokens=-5, precision=PRECISION[precision], layer_norm_eps=1e-5, cosine_eps=1e-8)
    params = [p.detach().contiguous() for p in model.param_list()]
    pc = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[p.data_ptr() for p in params]))
    bt = _lib.DrinGhmfcBatchC(ptr(mf), ptr(mmask), ptr(mimage), None, None)      # no candidate tensor at all
    nbytes = lib.drin_ghmfc_mention_forward_workspace_bytes(C.byref(c))
    assert nbytes > 0, lib.drin_last_error()
    ws_buf, ws = canaried(nbytes)
    out_buf, out = canaried(B * D * 4)
    _lib.check(lib.drin_ghmfc_mention_forward(C.byref(c), C.byref(bt), C.byref(pc), ptr(ws), nbytes, ptr(out), stream()))
    torch.cuda.synchronize()
    assert intact(ws_buf, nbytes) and intact(out_buf, B * D * 4)
    assert same_bits(out.view(torch.float32).reshape(B, D), want)
    assert same_bits(model._mention_only(batch[:5]), want)


# ---- 7. model.link ---------------------------------------------------------------------------------------------------------------
E_LINK, K_LINK = 150, 10


def link_inputs(pooled: bool):
    mention = [dev(a) for a in table_case("tiny_clean_b3")[0]]
    text, mask = entity_table("link_table", E_LINK, 0 if pooled else 6, 16)
    return mention, EntityTable(dev(text), dev(mask), None, None, None)


def table_form_scores(model, mention, table) -> torch.Tensor:
    """[B, E]: every row scored through the cached table form, in `arange` candidate blocks of N"""
    N, E, B = model.cfg.num_candidates, table.text.shape[0], mention[0].shape[0]
    model.enable_entity_cache()
    out = []
    with torch.no_grad():
        for e0 in range(0, E, N):
            cand = torch.arange(e0, e0 + N, device=DEV).clamp(max=E - 1).repeat(B, 1)
            out.append(model(GhmfcIndexedBatch(mention, table, cand)))
    return torch.cat(out, dim=1)[:, :E]


def check_link(model, mention, table, result, what):
    assert isinstance(result, LinkResult) and result.scores.shape == result.rows.shape == (3, K_LINK)
    assert result.scores.dtype == torch.float32 and result.rows.dtype == torch.int64 and not result.scores.requires_grad
    every = table_form_scores(model, mention, table)
    ref, got_rows = every.double().cpu().numpy(), result.rows.cpu().numpy()
    assert all(len(set(r)) == K_LINK for r in got_rows.tolist()) and got_rows.min() >= 0 and got_rows.max() < E_LINK, what
    holds_rule(ref, got_rows, K_LINK, TOL[model.precision], what)
    assert same_bits(result.scores, torch.gather(every, 1, result.rows)), what      # the table form's bits at the returned rows
    assert is_contract_ordered(result.scores.cpu().numpy(), got_rows), what
    # with those bits the list IS the table form's top-k by the contract unless the product mis-ranked a row at the boundary
    want_rows = np.stack([contract_order(every[b].cpu().numpy(), np.arange(E_LINK))[:K_LINK] for b in range(3)])
    print(f"{what}: {int((want_rows != got_rows).sum())} of {want_rows.size} positions differ from the table form's own top-k")


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("kind", ["model", "trainable", "variant"])
def test_link_on_the_three_models(kind, pooled):
    mention, table = link_inputs(pooled)
    model = make_model(kind, "tiny_clean_b3").eval()
    first = model.link(mention, K_LINK, table)
    assert model.entity_cache_builds == 1
    check_link(model, mention, table, first, f"{kind} pooled={pooled}")
    builds = model.entity_cache_builds
    model.attach_entity_table(table)
    zeros = torch.zeros(3, dtype=torch.int64, device=DEV)
    attached = model.link(mention + [torch.zeros(3, 4, dtype=torch.int64, device=DEV), zeros, zeros], K_LINK)   # items 5-7 are not read
    assert torch.equal(attached.rows, first.rows) and same_bits(attached.scores, first.scores)
    again = model.link(GhmfcIndexedBatch(mention, table, zeros), K_LINK)
    assert torch.equal(again.rows, first.rows) and model.entity_cache_builds == builds + 1      # attaching dropped the rows: one build
    with torch.no_grad():
        model.entity_encoder.final_layer.weight.mul_(-1.0).add_(0.05)
    moved = model.link(mention, K_LINK)
    assert model.entity_cache_builds == builds + 2 and not torch.equal(moved.rows, first.rows)
    check_link(model, mention, table, moved, f"{kind} pooled={pooled} after the weights moved")
    with pytest.raises(ValueError, match="exceeds the table's 150"):
        model.link(mention, E_LINK + 1)
    with pytest.raises(ValueError, match="k = 257"):
        model.link(mention, 257)
    with pytest.raises(RuntimeError, match="eval\\(\\) only"):
        model.train().link(mention, K_LINK)


@pytest.mark.parametrize("kind", ["model", "trainable", "variant"])
def test_link_recall_of_planted_answers(kind):
    mention, table = link_inputs(pooled=True)
    model = make_model(kind, "tiny_clean_b3", precision="f32").eval()
    with torch.no_grad():
        fl = model.entity_encoder.final_layer
        fl.weight.copy_(torch.eye(16, device=DEV))
        fl.bias.zero_()
        x = model.encode_mentions(mention + [torch.zeros(3, 4, 16, device=DEV), 0, 0])
    answers = torch.tensor([0, E_LINK - 1, 64], device=DEV)
    text = table.text.clone()
    text[answers] = 2.5 * x                                            # the entity row is the mention's direction: cosine 1
    result = model.link(mention, K_LINK, EntityTable(text, None, None, None, None))
    assert link_recall(result.rows, answers, [1, K_LINK]) == [1.0, 1.0]
    assert link_recall(result.rows.cpu(), (answers + 1) % E_LINK, [1]) == [0.0]
    assert bool(((result.scores[:, 0] - 1.0).abs() <= 1e-6).all())
