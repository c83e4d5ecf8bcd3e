"""-m gpu: the summed-cosine first stage (csrc/table_topk.hip).

`drin_table_topk_sum` with one term of weight 1 IS `drin_table_topk`, bit for bit; its scores are the fp32 chain over
`drin_cosine_rows_indexed_fwd` of every live term on its rows; its rows follow the selection rule of section 24 against the fp64
restatement (tests/table_topk_sum_restatement.py) with the bar taken once per term; `drin_topk_combine` is held to its fp64
formula and to its own roundings, and `drin_topk_update` on a combined block to the contract exactly.  Then the corners, and
`Model.link(first_stage="edges")` against `link(candidates=)` fed with `table_topk_sum`'s rows of the same three terms."""
import ctypes as C

import numpy as np
import pytest
import torch

from drin_amd import _lib, row_ops
from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk_sum
from drin_amd.metrics import link_recall
from drin_amd.model import EntityTable, Model
from tests.drin_link_restatement import K_LINK
from tests.table_topk_sum_restatement import BAR, CASES, chain32, combine32, combine64, near_threshold, sum64, sum_case, tol_of
from tests.test_gpu_drin_link import gpu_case
from tests.test_gpu_ghmfc_table import same_bits
from tests.test_gpu_table_topk import (contract_order, dev, expected_topk, feed, indexed_cosine, inv_norms, is_contract_ordered, ptr, stream,
                                       table_topk, whole_case)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-8
PRECISIONS = ["bf16x3", "f32"]


def topk_sum(xs, tables, invs, weights, k, precision, chunk=0):
    return table_topk_sum(list(zip(xs, tables, invs, weights)), k, EPS, precision, chunk)


def on_device(xs, tables):
    xs_t, tables_t = [dev(x) for x in xs], [dev(t) for t in tables]
    return xs_t, tables_t, [inv_norms(t) for t in tables_t]


# ---- 1. identity with the single-term call --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D,E,B,k,chunk", [(16, 300, 3, 20, 64), (32, 1500, 4, 64, 256)])
def test_one_term_of_weight_one_is_table_topk(D, E, B, k, chunk, precision):
    x, rows, _ = whole_case(D, E, B)
    (x_t,), (rows_t,), (inv_t,) = on_device([x], [rows])
    want_scores, want_rows = table_topk(x_t, rows_t, inv_t, k, precision, chunk)
    one = topk_sum([x_t], [rows_t], [inv_t], [1.0], k, precision, chunk)
    assert torch.equal(one.rows, want_rows) and same_bits(one.scores, want_scores)
    # the same term twice, half each: 0.5 c + 0.5 c is exact
    halves = topk_sum([x_t, x_t], [rows_t, rows_t], [inv_t, inv_t], [0.5, 0.5], k, precision, chunk)
    assert torch.equal(halves.rows, want_rows) and same_bits(halves.scores, want_scores)
    # a term of weight 0 with NULL pointers changes nothing, wherever it stands
    for terms in ([(None, None, None, 0.0), (x_t, rows_t, inv_t, 1.0)], [(x_t, rows_t, inv_t, 1.0), (None, None, None, 0.0)],
                  [(x_t, rows_t, inv_t, 0.5), (None, None, None, 0.0), (x_t, rows_t, inv_t, 0.5), (None, None, None, -0.0)]):
        got = table_topk_sum(terms, k, EPS, precision, chunk)
        assert torch.equal(got.rows, want_rows) and same_bits(got.scores, want_scores)


# ---- 2. + 3. the bit statement and the selection rule ---------------------------------------------------------------------------
def holds_rule(ref, got_rows, k, tol, cap, what):
    for b in range(ref.shape[0]):
        t = np.sort(ref[b])[::-1][k - 1]
        assert int((np.abs(ref[b] - t) <= tol).sum()) - 1 <= cap, f"{what}: mention {b} has too many rows within {tol} of the k-th"
        assert (ref[b, got_rows[b]] >= t - tol).all(), f"{what}: mention {b} returned a row below t - tol"
        assert np.isin(np.nonzero(ref[b] > t + tol)[0], got_rows[b]).all(), f"{what}: mention {b} misses a row above t + tol"


SWEEP = [(name, chunk) for name in CASES for chunk in CASES[name][5]]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,chunk", SWEEP)
def test_sum_against_fp64_and_the_chain_of_indexed_cosines(name, chunk, precision):
    c = sum_case(name)
    k, weights, ref, E = c["k"], c["weights"], c["ref"], c["E"]
    xs_t, tables_t, invs_t = on_device(c["xs"], c["tables"])
    got = topk_sum(xs_t, tables_t, invs_t, weights, k, precision, chunk)
    got_rows, got_scores = got.rows.cpu().numpy(), got.scores.cpu().numpy()
    what = f"{name} chunk{chunk} {precision}"
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    # the bit statement: the fp32 chain over the indexed cosines of every term on the returned rows
    cosines = [indexed_cosine(x_t, rows_t, got.rows).cpu().numpy() for x_t, rows_t in zip(xs_t, tables_t)]
    assert np.array_equal(got_scores.view(np.uint32), chain32(cosines, weights).view(np.uint32)), what
    err = float(np.abs(got_scores - np.take_along_axis(ref, got_rows, 1)).max())
    print(f"{what}: max |returned score - fp64| = {err:.3e} (bar {tol_of(weights, 'f32'):.1e}), "
          f"rows within tol of the k-th: {near_threshold(ref, k, tol_of(weights, precision))}")
    assert err <= tol_of(weights, "f32"), what                          # drin_cosine_rows_fwd's bar, once per term
    holds_rule(ref, got_rows, k, tol_of(weights, precision), c["cap"], what)
    assert is_contract_ordered(got_scores, got_rows), what
    again = topk_sum(xs_t, tables_t, invs_t, weights, k, precision, chunk)
    assert torch.equal(again.rows, got.rows) and same_bits(again.scores, got.scores), what   # the same bits every run


def run_combine(blocks_t, invs_t, scales_t, weights, ld, B, cols, out_t):
    S = len(blocks_t)
    arrays = [(C.c_void_p * S)(*[t.data_ptr() for t in ts]) for ts in (blocks_t, invs_t, scales_t)]
    _lib.check(_lib.load().drin_topk_combine(*arrays, (C.c_float * S)(*weights), S, ld, B, cols, ptr(out_t), stream()))


def combine_inputs(Ec, B, S, seed):
    g = np.random.default_rng(seed)
    ld = -(-B // 4) * 4
    blocks = [g.standard_normal((Ec, ld)).astype(np.float32) * np.float32(10.0) for _ in range(S)]
    invs = [(0.05 + g.random(Ec)).astype(np.float32) for _ in range(S)]
    scales = [(0.05 + g.random(ld)).astype(np.float32) for _ in range(S)]
    weights = [1.0, -0.5, 2.0, 0.25][:S]
    return ld, blocks, invs, scales, weights


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("Ec,B", [(1, 1), (63, 5), (64, 4), (257, 9), (2100, 1030)])
def test_combine_against_its_formula_with_the_output_on_block_zero(Ec, B, S):
    """(2100, 1030): more quads than one workgroup is wide and more rows than one pass of the grid"""
    ld, blocks, invs, scales, weights = combine_inputs(Ec, B, S, 100 * Ec + 10 * B + S)
    ref = combine64(blocks, invs, scales, weights)
    blocks_t, invs_t, scales_t = [dev(b) for b in blocks], [dev(i) for i in invs], [dev(s) for s in scales]
    G = 64
    guarded = torch.full((G + Ec * ld + G,), 777.0, device=DEV)
    apart = guarded[G:G + Ec * ld].view(Ec, ld)
    run_combine(blocks_t, invs_t, scales_t, weights, ld, B, Ec, apart)
    torch.cuda.synchronize()
    assert bool((guarded[:G] == 777.0).all()) and bool((guarded[-G:] == 777.0).all())
    assert all(torch.equal(t, dev(b)) for t, b in zip(blocks_t, blocks))              # the inputs are left alone
    got = apart.cpu().numpy()
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"combine Ec={Ec} B={B} S={S}: max err {err:.2e} of max |ref| {top:.2e}")
    assert err <= 1e-6 * top
    assert np.array_equal(got.view(np.uint32), combine32(blocks, invs, scales, weights).view(np.uint32))   # its own roundings, no contraction
    run_combine(blocks_t, invs_t, scales_t, weights, ld, B, Ec, blocks_t[0])          # the output ON block 0
    assert torch.equal(blocks_t[0].view(torch.int32), apart.view(torch.int32))
    assert all(torch.equal(t, dev(b)) for t, b in zip(blocks_t[1:], blocks[1:]))


@pytest.mark.parametrize("cols,k", [(300, 20), (4096 + 70, 100)])
def test_selection_on_a_combined_block_is_exact(cols, k):
    """the selection the whole call makes, on a block combined by hand: drin_topk_update (no inverse norms left) returns THE
    first k of the combined keys by the contract - ties (two terms that cancel), a NaN and an infinity among them"""
    B, S = 3, 3
    ld, blocks, invs, scales, weights = combine_inputs(cols, B, S, 5)
    blocks[1][10:40] = blocks[0][10:40] * 2                             # with weight -0.5 and equal factors: exact zeros, many ties
    invs[1][10:40], invs[0][10:40] = 1.0, 1.0
    scales[1][:], scales[0][:] = 1.0, 1.0
    blocks[2][10:40] = 0.0
    blocks[0][50, 0], blocks[1][60, 1] = np.nan, np.inf
    by_hand = combine32(blocks, invs, scales, weights)
    assert (by_hand[10:40, :B] == 0).all()
    out_t = torch.empty(cols, ld, device=DEV)
    run_combine([dev(b) for b in blocks], [dev(i) for i in invs], [dev(s) for s in scales], weights, ld, B, cols, out_t)
    assert np.array_equal(out_t.cpu().numpy().view(np.uint32), by_hand.view(np.uint32))
    dots = np.ascontiguousarray(by_hand[:, :B].T)
    want_keys, want_rows = expected_topk(dots, None, k)
    for cuts in ([0, cols], [0, 64, cols]):
        got_keys, got_rows = feed(out_t, None, B, cols, k, cuts, ld=ld)
        assert np.array_equal(got_rows, want_rows) and np.array_equal(got_keys, np.where(want_keys == 0, 0.0, want_keys), equal_nan=True)


# ---- 4. corners ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_corners(precision):
    E, B, chunk, ZERO, NAN = 70, 4, 32, 7, 40
    g = np.random.default_rng(3)
    xs = [g.standard_normal((B, d)).astype(np.float32) for d in (16, 8)]
    tables = [g.standard_normal((E, d)).astype(np.float32) for d in (16, 8)]
    tables[0][ZERO] = 0.0                                               # a zero table row in term 0 only
    tables[1][NAN, 3] = np.nan                                          # a NaN in one table row of term 1
    xs[0][2] = 0.0                                                      # mention 2: a zero query row in term 0
    xs[1][3, 1] = np.nan                                                # mention 3: a NaN query row in term 1
    tables[0][51], tables[1][51] = tables[0][50], tables[1][50]         # rows 50 and 51: equal scores for every mention
    xs_t, tables_t, invs_t = on_device(xs, tables)
    weights = (1.0, 2.0)
    ref = sum64(xs, tables, weights)
    got = topk_sum(xs_t, tables_t, invs_t, weights, E, precision, chunk)               # k = E: every row appears
    scores, rows = got.scores.cpu().numpy(), got.rows.cpu().numpy()
    only1 = cosine_rows_indexed(xs_t[1], tables_t[1], got.rows, EPS, None).cpu().numpy()
    only0 = cosine_rows_indexed(xs_t[0], tables_t[0], got.rows, EPS, None).cpu().numpy()
    for b in range(3):
        assert sorted(rows[b].tolist()) == list(range(E))
        at = int(np.nonzero(rows[b] == ZERO)[0][0])
        assert only0[b, at] == 0.0 and scores[b, at] == np.float32(2.0) * only1[b, at] and at < E - 1     # term 1 still ranks it
        assert rows[b, E - 1] == NAN and np.isnan(scores[b, E - 1]) and np.isfinite(scores[b, :E - 1]).all()   # the NaN row ranks last
        at50 = int(np.nonzero(rows[b] == 50)[0][0])
        assert rows[b, at50 + 1] == 51 and scores[b, at50] == scores[b, at50 + 1]      # equal scores: the lower row first
        assert np.abs(scores[b, :E - 1] - ref[b, rows[b, :E - 1]]).max() <= tol_of(weights, "f32")
    assert (only0[2] == 0).all() and np.array_equal(scores[2, :E - 1], (np.float32(2.0) * only1[2, :E - 1]).astype(np.float32))   # the zero query row
    assert np.isnan(scores[3]).all() and rows[3].tolist() == list(range(E))            # a NaN query row: the whole list is NaN
    short = topk_sum(xs_t, tables_t, invs_t, weights, 10, precision, chunk)
    assert short.rows[3].tolist() == list(range(10)) and not bool((short.rows[:3] == NAN).any())
    again = topk_sum(xs_t, tables_t, invs_t, weights, E, precision, chunk)
    assert torch.equal(again.rows, got.rows) and same_bits(again.scores, got.scores)


def test_the_wrapper_refuses_what_the_library_would_trust():
    x, rows = torch.randn(3, 16, device=DEV), torch.randn(50, 16, device=DEV)
    inv = row_inv_norms(rows, EPS)
    with pytest.raises(ValueError, match="term 1"):
        table_topk_sum([(x, rows, inv, 1.0), (x[:2], rows, inv, 1.0)], 5, EPS, "f32")
    with pytest.raises(ValueError, match="term 0"):
        table_topk_sum([(x, rows[:, :8], inv, 1.0)], 5, EPS, "f32")
    with pytest.raises(ValueError, match="contiguous float32"):
        table_topk_sum([(x.double(), rows, inv, 1.0)], 5, EPS, "f32")
    with pytest.raises(ValueError, match="term 0"):
        table_topk_sum([(x, rows, inv[:-1], 1.0)], 5, EPS, "f32")
    with pytest.raises(_lib.DrinError, match="no live term"):
        table_topk_sum([(x, rows, inv, 0.0)], 5, EPS, "f32")
    with pytest.raises(_lib.DrinError, match="num_terms = 5"):
        table_topk_sum([(x, rows, inv, 1.0)] * 5, 5, EPS, "f32")


# ---- 5. through the model ---------------------------------------------------------------------------------------------------------
def edge_terms(model, table, mention, clip_image, clip_text, weights):
    """the three terms of first_stage="edges", built here from the public pieces"""
    eps = model.cfg.cosine_eps
    tt_rows = table.pooled_text(model.cfg)[1] if table.text.dim() == 3 else table.text.contiguous()
    pairs = ((row_ops.span_mean(mention[0], mention[2], mention[3]), tt_rows), (clip_text, table.clip_image), (clip_image, table.clip_text))
    return [(x.contiguous(), r, row_inv_norms(r, eps), w) if w != 0 else (None, None, None, 0.0) for (x, r), w in zip(pairs, weights)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("name", ["wm", "wd"])                            # token-level and pooled tables
def test_link_edges_is_link_on_the_rows_of_the_three_terms(name, cached, precision):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case(name, cached, precision)
    cfg, N = c["cfg"], c["cfg"].num_candidates_model
    assert (table.text.dim() == 3) == (name == "wm")
    first = table_topk_sum(edge_terms(model, table, mention, clip_image, clip_text, (1.0, 1.0, 1.0)), N, cfg.cosine_eps, precision)
    assert tuple(first.rows.shape) == (3, N)
    got = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges")
    want = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=first.rows)
    assert torch.equal(got.rows, want.rows) and same_bits(got.scores, want.scores)
    assert tuple(got.rows.shape) == (3, K_LINK) and got.rows.dtype == torch.int64 and got.scores.dtype == torch.float32
    # which rows and which pairing each term uses: the layer-0 edges of the forward on the gathered batch of those rows
    from drin_amd.model import IndexedBatch
    batch = IndexedBatch.from_clip(mention, table, first.rows, clip_image, clip_text, model=model)
    traced = model.forward_traced(mention + table.gather(first.rows) + [batch.miet_similarity, batch.mtei_similarity])
    e0 = traced["edges0"]
    err = (first.scores - (e0[0] + e0[1] + e0[2])).abs().max().item()
    print(f"{name} cached={cached} {precision}: max |first-stage score - (tt + ti + it of the forward)| = {err:.2e}")
    assert err <= 3 * 1e-5
    # the norms of the three tables are cached per tensor version, and dropped by invalidate()
    held = {s: e[1] for s, e in model._link_edges_inv.items()}
    assert sorted(held) == [0, 1, 2]
    model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges")
    assert all(model._link_edges_inv[s][1] is held[s] for s in held)
    table.clip_image.mul_(1.0)
    model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges")
    assert model._link_edges_inv[1][1] is not held[1] and model._link_edges_inv[0][1] is held[0] and model._link_edges_inv[2][1] is held[2]
    model.invalidate()
    assert "_link_edges_inv" not in model.__dict__


@pytest.mark.parametrize("name", ["wm", "wd"])
def test_planted_entities_are_found_and_a_swapped_clip_pairing_is_not(name):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case(name, False, "f32")
    E, N = table.num_entities, c["cfg"].num_candidates_model
    gold = torch.tensor([E - 1, 0, 17], device=DEV)
    g = torch.Generator().manual_seed(12)
    noisy = lambda t: t + 0.05 * torch.randn(t.shape, generator=g).to(DEV)   # noqa: E731
    text = table.text.clone()
    span = row_ops.span_mean(mention[0], mention[2], mention[3])
    if text.dim() == 3:
        text[gold, 0, :] = noisy(span)                                  # the token-0 row
    else:
        text[gold] = noisy(span)
    planted = EntityTable(text, table.mask, table.image, table.object, table.object_score)
    t_text, t_image = table.clip_text.clone(), table.clip_image.clone()
    t_image[gold], t_text[gold] = noisy(clip_text), noisy(clip_image)   # ti: clip_text x clip_image rows; it: clip_image x clip_text rows
    planted.set_clip(t_text, t_image)
    for weights in (None, (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        rows = model._edge_candidates(mention, planted, clip_image, clip_text, weights)
        assert link_recall(rows, gold, [1]) == [1.0], weights
        through = model.link(mention, planted, N, clip_image, clip_text, first_stage="edges", edge_weights=weights)
        assert link_recall(through.rows, gold, [N]) == [1.0], weights
    swapped = model._edge_candidates(mention, planted, clip_text, clip_image, (0, 1, 1))    # the mentions' two CLIP rows are independent draws
    assert link_recall(swapped, gold, [1]) != [1.0]


def test_edge_weights_drop_terms_and_follow_the_configuration(monkeypatch):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", False, "bf16x3")
    cfg, N = c["cfg"], c["cfg"].num_candidates_model
    two = table_topk_sum(edge_terms(model, table, mention, clip_image, clip_text, (0, 1.0, 1.0))[1:], N, cfg.cosine_eps, "bf16x3").rows

    def never(*a, **k):
        raise AssertionError("the tensors of a dropped term were read")

    with monkeypatch.context() as m:                                    # tt's tensors are never read
        m.setattr(row_ops, "span_mean", never)
        m.setattr(EntityTable, "pooled_text", never)
        assert torch.equal(model._edge_candidates(mention, table, clip_image, clip_text, (0, 1, 1)), two)
    got = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=(0, 1, 1))
    want = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=two)
    assert torch.equal(got.rows, want.rows) and same_bits(got.scores, want.scores)
    half = table_topk_sum(edge_terms(model, table, mention, clip_image, clip_text, (1.0, 0.5, 2.0)), N, cfg.cosine_eps, "bf16x3").rows
    assert torch.equal(model._edge_candidates(mention, table, clip_image, clip_text, (1.0, 0.5, 2.0)), half)
    # the default weights are cfg.gcn_edge_enabled[0:3]
    off = Model(cfg.with_(gcn_edge_enabled=(1, 0, 1, 1)), precision="bf16x3").to(DEV).eval()
    one_off = table_topk_sum(edge_terms(off, table, mention, clip_image, clip_text, (1.0, 0, 1.0)), N, cfg.cosine_eps, "bf16x3").rows
    assert torch.equal(off._edge_candidates(mention, table, clip_image, clip_text, None), one_off)
    assert not torch.equal(one_off, model._edge_candidates(mention, table, clip_image, clip_text, None))


def test_link_edges_empty_and_sliced_batches(monkeypatch):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", False, "bf16x3")
    none = model.link([t[:0] for t in mention], table, K_LINK, clip_image[:0], clip_text[:0], first_stage="edges")
    assert tuple(none.scores.shape) == (0, K_LINK) == tuple(none.rows.shape) and none.rows.dtype == torch.int64
    halves = [model.link([t[sl] for t in mention], table, K_LINK, clip_image[sl], clip_text[sl], first_stage="edges")
              for sl in (slice(0, 2), slice(2, 3))]
    calls, lib = [], _lib.load()
    real = lib.drin_table_topk_sum
    monkeypatch.setattr(lib, "drin_table_topk_sum", lambda *a: (calls.append(a[3]), real(*a))[1])
    monkeypatch.setattr(Model, "MAX_CALL_MENTIONS", 2)
    sliced = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges")
    assert calls == [2, 1]                                              # a batch above MAX_CALL_MENTIONS runs in slices
    assert torch.equal(sliced.rows, torch.cat([h.rows for h in halves])) and same_bits(sliced.scores, torch.cat([h.scores for h in halves]))


def test_an_empty_span_lists_the_first_rows():
    """documented, not special-cased: an empty span gives a NaN tt row, every first-stage score of that mention is NaN and its
    candidates are rows 0 .. N-1 by the contract"""
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wd", False, "f32")
    N = c["cfg"].num_candidates_model
    mention = [t.clone() for t in mention]
    mention[3][1] = mention[2][1]                                       # end = start
    rows = model._edge_candidates(mention, table, clip_image, clip_text, None)
    assert rows[1].tolist() == list(range(N)) and rows[0].tolist() != list(range(N))
