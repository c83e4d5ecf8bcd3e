"""-m gpu: the image-image edge as a term of the summed top-k (csrc/table_topk.hip).

`drin_object_rows` against fp64 with its masses bit for bit; `drin_topk_combine_forms` against its fp64 formula and against its own
roundings restated in numpy float32; `drin_ratio_rows_indexed_fwd` against fp64; the whole call `drin_table_topk_sum_forms` on the
shared cases - its scores ARE the fp32 chain over the indexed cosines and the indexed ratio, its rows follow the selection rule of
section 24 against the fp64 DOUBLE LOOP of `model.py:84-92` (tests/table_topk_ratio_restatement.py), not against the factored form;
and `Model.link(first_stage="edges")` with four weights.  Every test prints its maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.model import EntityTable
from drin_amd.table_ops import RatioTerm, object_rows, ratio_rows_indexed, table_topk_sum
from tests.drin_link_restatement import K_LINK
from tests.table_topk_ratio_restatement import (CASES, COS_EPS, MIEI_EPS, chain32, combine_forms32, combine_forms64, mass32, near_threshold,
                                                object_rows64, ratio64, ratio_case, tol_of)
from tests.test_gpu_drin_link import gpu_case
from tests.test_gpu_ghmfc_table import same_bits
from tests.test_gpu_table_topk import dev, indexed_cosine, inv_norms, is_contract_ordered, ptr, stream
from tests.test_gpu_table_topk_sum import edge_terms, holds_rule

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ["bf16x3", "f32"]
PREC = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
GUARD, CANARY = 64, 777.0


def guarded(shape):
    """`(whole, view)`: a float32 buffer with GUARD canary words on either side of the `shape` view"""
    n = int(np.prod(shape))
    whole = torch.full((GUARD + n + GUARD,), CANARY, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guards_intact(whole) -> bool:
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


# ---- 1. drin_object_rows ---------------------------------------------------------------------------------------------------------
def run_object_rows(obj_t, score_t, dtype):
    n, K, R = obj_t.shape
    w_out, out = guarded((n, R))
    w_mass, mass = guarded((n,))
    _lib.check(_lib.load().drin_object_rows(ptr(obj_t), ptr(score_t), dtype, n, K, R, COS_EPS, ptr(out), ptr(mass), stream()))
    torch.cuda.synchronize()
    assert guards_intact(w_out) and guards_intact(w_mass)
    return out, mass


def object_inputs(n, K, R, seed):
    g = np.random.default_rng(seed)
    obj = g.standard_normal((n, K, R)).astype(np.float32)
    score = (0.05 + 0.95 * g.random((n, K))).astype(np.float32)
    if n > 1:
        obj[n // 2, K - 1] = 0.0                                        # a zero object row: its norm is clamped, it adds nothing
    if n > 1 or K > 1:
        score[0, 0] = 0.0                                               # a zero score
    if n > 2:
        score[n - 2, :] = 0.0                                           # a row whose scores are all zero: a zero row of mass 0
    return obj, score


@pytest.mark.parametrize("n,K,R", [(1, 1, 8), (5, 3, 260), (7, 4, 2048), (3, 2, 2056), (65541, 1, 8)])
def test_object_rows_against_fp64_and_its_masses_bit_for_bit(n, K, R):
    """260: a tail of the lane loop; 2048: every register slot full; 2056: past the register form (each row read twice);
    65 541 rows: more workgroups than a 65 535 grid dimension holds, the last row checked"""
    obj, score = object_inputs(n, K, R, 1000 * n + 10 * K + R)
    ref, _ = object_rows64(obj, score)
    obj_t, score_t = dev(obj), dev(score)
    out, mass = run_object_rows(obj_t, score_t, _lib.FEAT_F32)
    assert torch.equal(obj_t, dev(obj)) and torch.equal(score_t, dev(score))          # the inputs are left alone
    got = out.cpu().numpy()
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"object rows n={n} K={K} R={R}: max err {err:.2e} of max |ref| {top:.2e}, last row err {float(np.abs(got[-1] - ref[-1]).max()):.2e}")
    assert err <= 1e-6 * top and float(np.abs(got[-1] - ref[-1]).max()) <= 1e-6 * top
    assert np.array_equal(mass.cpu().numpy().view(np.uint32), mass32(score).view(np.uint32))   # the ascending fp32 sum
    if n > 2:
        assert (got[n - 2] == 0).all() and float(mass[n - 2]) == 0.0
    if n > 1 and K == 1:
        assert (got[n // 2] == 0).all()                                 # the zero object row alone: a zero output row
    again, mass_again = run_object_rows(obj_t, score_t, _lib.FEAT_F32)
    assert same_bits(again, out) and same_bits(mass_again, mass)                         # the same bits every run
    via = object_rows(obj_t, score_t, COS_EPS)                                           # the wrapper makes the same call
    assert same_bits(via[0], out) and same_bits(via[1], mass)


@pytest.mark.parametrize("n,K,R", [(5, 3, 264), (7, 4, 2048), (3, 2, 2056), (4, 1, 8)])
def test_object_rows_on_bf16_storage_are_the_fp32_call_on_the_widened_values(n, K, R):
    obj, score = object_inputs(n, K, R, 7 * n + K + R)
    obj_b, score_b = dev(obj).bfloat16(), dev(score).bfloat16()
    out_b, mass_b = run_object_rows(obj_b, score_b, _lib.FEAT_BF16)
    out_f, mass_f = run_object_rows(obj_b.float(), score_b.float(), _lib.FEAT_F32)
    assert same_bits(out_b, out_f) and same_bits(mass_b, mass_f)
    via = object_rows(obj_b, score_b, COS_EPS)
    assert same_bits(via[0], out_b) and same_bits(via[1], mass_b) and via[0].dtype == torch.float32


# ---- 2. drin_topk_combine_forms --------------------------------------------------------------------------------------------------
def forms_array(forms_t, S):
    arr = (_lib.DrinTopkFormC * S)()
    for s, f in enumerate(forms_t):
        if f is not None:
            arr[s].form, arr[s].x_mass, arr[s].row_mass, arr[s].eps = _lib.TOPK_RATIO, f[0].data_ptr(), f[1].data_ptr(), f[2]
    return arr


def run_combine_forms(blocks_t, invs_t, scales_t, weights, forms_t, ld, B, cols, out_t, plain=False):
    S = len(blocks_t)
    arrays = [(C.c_void_p * S)(*[0 if t is None else t.data_ptr() for t in ts]) for ts in (blocks_t, invs_t, scales_t)]
    w = (C.c_float * S)(*weights)
    lib = _lib.load()
    if plain:
        _lib.check(lib.drin_topk_combine(*arrays, w, S, ld, B, cols, ptr(out_t), stream()))
    else:
        _lib.check(lib.drin_topk_combine_forms(*arrays, w, None if forms_t is None else forms_array(forms_t, S), S, ld, B, cols, ptr(out_t),
                                               stream()))


def combine_inputs(Ec, B, S, ratio_at, seed):
    g = np.random.default_rng(seed)
    ld = -(-B // 4) * 4
    blocks = [g.standard_normal((Ec, ld)).astype(np.float32) * np.float32(10.0) for _ in range(S)]
    invs = [(0.05 + g.random(Ec)).astype(np.float32) for _ in range(S)]
    scales = [(0.05 + g.random(ld)).astype(np.float32) for _ in range(S)]
    weights = [1.0, -0.5, 2.0, 0.25][:S]
    forms = [None] * S
    forms[ratio_at] = ((0.05 + g.random(ld)).astype(np.float32), (0.05 + g.random(Ec)).astype(np.float32), MIEI_EPS)
    return ld, blocks, invs, scales, weights, forms


@pytest.mark.parametrize("S,ratio_at", [(4, 0), (4, 3), (1, 0), (2, 1)])
@pytest.mark.parametrize("Ec,B", [(1, 1), (63, 5), (257, 9), (2100, 1030)])
def test_combine_forms_against_its_formula_and_its_own_roundings(Ec, B, S, ratio_at):
    """the RATIO term in slot 0 - the output ON block 0 - and in the last slot; (2100, 1030): more quads than one workgroup is wide
    and more rows than one pass of the grid"""
    ld, blocks, invs, scales, weights, forms = combine_inputs(Ec, B, S, ratio_at, 100 * Ec + 10 * B + S + ratio_at)
    ref = combine_forms64(blocks, invs, scales, weights, forms)
    blocks_t = [dev(b) for b in blocks]
    invs_t = [None if f is not None else dev(i) for i, f in zip(invs, forms)]          # a RATIO term's inverse norms and factors: NULL
    scales_t = [None if f is not None else dev(s) for s, f in zip(scales, forms)]
    forms_t = [None if f is None else (dev(f[0]), dev(f[1]), f[2]) for f in forms]
    whole, apart = guarded((Ec, ld))
    run_combine_forms(blocks_t, invs_t, scales_t, weights, forms_t, ld, B, Ec, apart)
    torch.cuda.synchronize()
    assert guards_intact(whole) and all(torch.equal(t, dev(b)) for t, b in zip(blocks_t, blocks))
    got = apart.cpu().numpy()
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"combine forms Ec={Ec} B={B} S={S} ratio at {ratio_at}: max err {err:.2e} of max |ref| {top:.2e}")
    assert err <= 1e-6 * top
    assert np.array_equal(got.view(np.uint32), combine_forms32(blocks, invs, scales, weights, forms).view(np.uint32))   # no contraction
    run_combine_forms(blocks_t, invs_t, scales_t, weights, forms_t, ld, B, Ec, blocks_t[0])                              # the output ON block 0
    assert torch.equal(blocks_t[0].view(torch.int32), apart.view(torch.int32))
    assert all(torch.equal(t, dev(b)) for t, b in zip(blocks_t[1:], blocks[1:]))


def test_a_zero_mass_product_gives_block_over_eps_exactly():
    Ec, B = 70, 6
    ld, blocks, invs, scales, _w, forms = combine_inputs(Ec, B, 1, 0, 3)
    x_mass, row_mass, eps = forms[0]
    x_mass[2], row_mass[5] = 0.0, 0.0                                   # a mention and an entity of mass 0
    out_t = torch.empty(Ec, ld, device=DEV)
    run_combine_forms([dev(blocks[0])], [None], [None], [1.0], [(dev(x_mass), dev(row_mass), eps)], ld, B, Ec, out_t)
    got = out_t.cpu().numpy()
    over_eps = (blocks[0] / np.float32(eps)).astype(np.float32)
    assert np.array_equal(got[5].view(np.uint32), over_eps[5].view(np.uint32)) and np.array_equal(got[:, 2].view(np.uint32), over_eps[:, 2].view(np.uint32))
    blocks[0][5] = 0.0                                                  # what the whole call sees there: a zero row u, a zero dot product
    run_combine_forms([dev(blocks[0])], [None], [None], [1.0], [(dev(x_mass), dev(row_mass), eps)], ld, B, Ec, out_t)
    assert bool((out_t[5] == 0).all())


@pytest.mark.parametrize("S", [1, 3, 4])
@pytest.mark.parametrize("Ec,B", [(63, 5), (2100, 1030)])
def test_all_cosine_forms_are_the_plain_combine_bit_for_bit(Ec, B, S):
    ld, blocks, invs, scales, weights, _f = combine_inputs(Ec, B, S, 0, 9 * Ec + B + S)
    blocks_t, invs_t, scales_t = [dev(b) for b in blocks], [dev(i) for i in invs], [dev(s) for s in scales]
    want, none, zeros = (torch.empty(Ec, ld, device=DEV) for _ in range(3))
    run_combine_forms(blocks_t, invs_t, scales_t, weights, None, ld, B, Ec, want, plain=True)
    run_combine_forms(blocks_t, invs_t, scales_t, weights, None, ld, B, Ec, none)
    run_combine_forms(blocks_t, invs_t, scales_t, weights, [None] * S, ld, B, Ec, zeros)
    assert torch.equal(want.view(torch.int32), none.view(torch.int32)) and torch.equal(want.view(torch.int32), zeros.view(torch.int32))


# ---- 3. drin_ratio_rows_indexed_fwd ----------------------------------------------------------------------------------------------
def ratio_inputs(B, E, R, Km, Ke, seed):
    g = np.random.default_rng(seed)
    mobj, eobj = g.standard_normal((B, Km, R)).astype(np.float32), g.standard_normal((E, Ke, R)).astype(np.float32)
    ms, es = (0.05 + 0.95 * g.random((B, Km))).astype(np.float32), (0.05 + 0.95 * g.random((E, Ke))).astype(np.float32)
    es[1, :] = 0.0
    q, S = object_rows64(mobj, ms)
    u, T = object_rows64(eobj, es)
    return [a.astype(np.float32) for a in (q, S, u, T)]


@pytest.mark.parametrize("B,N,E,R", [(1, 5, 7, 8), (3, 11, 7, 260), (5, 33, 40, 2048), (2, 3, 9, 2056)])
def test_ratio_rows_indexed_against_fp64(B, N, E, R):
    q, S, u, T = ratio_inputs(B, E, R, 3, 2, 10 * B + N + R)
    g = torch.Generator().manual_seed(B + N)
    index = torch.randint(0, E, (B, N), generator=g)
    index[0, 0] = 1                                                     # the entity of mass 0: exactly 0
    ref = np.take_along_axis(ratio64(q, S, u, T), index.numpy(), 1)
    q_t, S_t, u_t, T_t, index_t = dev(q), dev(S), dev(u), dev(T), index.to(DEV)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    got = ratio_rows_indexed(q_t, S_t, u_t, T_t, index_t, MIEI_EPS, status)
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"ratio rows ({B},{N},{E},{R}): max err {err:.2e} of max |ref| {float(np.abs(ref).max()):.2e}")
    assert err <= 1e-5 and float(got[0, 0]) == 0.0 and status.tolist() == [0, 0, 0, 0]
    assert same_bits(ratio_rows_indexed(q_t, S_t, u_t, T_t, index_t, MIEI_EPS, None), got)          # two runs: the same bits


@pytest.mark.parametrize("b,n,bad,clamped", [(2, 4, -1, 0), (0, 0, 7, 6), (1, 3, 1 << 40, 6)])
def test_ratio_rows_indexed_clamps_and_reports_a_bad_index(b, n, bad, clamped):
    B, N, E, R = 3, 5, 7, 16
    q, S, u, T = ratio_inputs(B, E, R, 2, 1, 4)
    index = torch.randint(0, E, (B, N), generator=torch.Generator().manual_seed(1))
    fixed = index.clone()
    index[b, n], fixed[b, n] = bad, clamped
    q_t, S_t, u_t, T_t = dev(q), dev(S), dev(u), dev(T)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    got = ratio_rows_indexed(q_t, S_t, u_t, T_t, index.to(DEV), MIEI_EPS, status)
    assert same_bits(got, ratio_rows_indexed(q_t, S_t, u_t, T_t, fixed.to(DEV), MIEI_EPS, None))
    w = status.tolist()
    assert w[0] == 1 and w[1] == b * N + n and ((w[3] & 0xFFFFFFFF) << 32 | (w[2] & 0xFFFFFFFF)) == bad & 0xFFFFFFFFFFFFFFFF
    assert same_bits(ratio_rows_indexed(q_t, S_t, u_t, T_t, index.to(DEV), MIEI_EPS, None), got)     # NULL status: clamped silently


# ---- 4. the whole call ---------------------------------------------------------------------------------------------------------------
def on_device(c):
    """the terms of a case on the device: the cosine 4-tuples (a weight 0: a dropped term) and the RatioTerm from drin_object_rows"""
    xs_t, tables_t = [dev(x) for x in c["xs"]], [dev(t) for t in c["tables"]]
    q, S = object_rows(dev(c["mobj"]), dev(c["ms"]), COS_EPS)
    u, T = object_rows(dev(c["eobj"]), dev(c["es"]), COS_EPS)
    w = c["weights"]
    cosines = [(x, t, inv_norms(t), wt) for x, t, wt in zip(xs_t, tables_t, w)] if xs_t else [(None, None, None, 0.0)] * 3
    return cosines, RatioTerm(q, S, u, T, w[3], MIEI_EPS)


SWEEP = [(name, chunk) for name in CASES for chunk in CASES[name][8]]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,chunk", SWEEP)
def test_four_terms_against_the_double_loop_and_the_chain_of_indexed_scores(name, chunk, precision):
    c = ratio_case(name)
    k, weights, ref, E = c["k"], c["weights"], c["ref"], c["E"]
    cosines, ratio = on_device(c)
    got = table_topk_sum(cosines + [ratio], k, COS_EPS, precision, chunk)
    got_rows, got_scores = got.rows.cpu().numpy(), got.scores.cpu().numpy()
    what = f"{name} chunk{chunk} {precision}"
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    # the rows drin_object_rows made are the fp64 ones to the kernel's bar
    for made, want in ((ratio.x, c["q"]), (ratio.rows, c["u"])):
        assert float(np.abs(made.cpu().numpy() - want).max()) <= 1e-6 * float(np.abs(want).max()), what
    # the bit statement: the fp32 chain over the indexed cosines of the live cosine terms and the indexed ratio of the RATIO term
    parts = [None if w == 0 else indexed_cosine(x, t, got.rows).cpu().numpy() for (x, t, _i, w) in cosines]
    parts.append(ratio_rows_indexed(ratio.x, ratio.x_mass, ratio.rows, ratio.row_mass, got.rows, MIEI_EPS, None).cpu().numpy())
    assert np.array_equal(got_scores.view(np.uint32), chain32(parts, weights).view(np.uint32)), what
    err = float(np.abs(got_scores - np.take_along_axis(ref, got_rows, 1)).max())
    print(f"{what}: max |returned score - fp64 double loop| = {err:.3e} (bar {tol_of(weights, 'f32'):.1e}), "
          f"rows within tol of the k-th: {near_threshold(ref, k, tol_of(weights, precision))}")
    assert err <= tol_of(weights, "f32"), what
    holds_rule(ref, got_rows, k, tol_of(weights, precision), c["cap"], what)
    assert is_contract_ordered(got_scores, got_rows), what
    again = table_topk_sum(cosines + [ratio], k, COS_EPS, precision, chunk)
    assert torch.equal(again.rows, got.rows) and same_bits(again.scores, got.scores), what          # the same bits every run


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["ii_e300", "ii_e1500"])
def test_null_forms_are_the_ex_entry_point_bit_for_bit(name, precision):
    c = ratio_case(name)
    lib, k, chunk, B, E = _lib.load(), c["k"], c["chunks"][0], c["B"], c["E"]
    cosines, _ratio = on_device(c)
    S = len(cosines)
    arr, dtypes = (_lib.DrinTopkTermC * S)(), (C.c_int32 * S)(*[_lib.FEAT_F32] * S)
    for s, (x, t, inv, w) in enumerate(cosines):
        arr[s].x, arr[s].rows, arr[s].row_inv_norms, arr[s].width, arr[s].weight = x.data_ptr(), t.data_ptr(), inv.data_ptr(), x.shape[1], w
    nbytes = lib.drin_table_topk_sum_workspace_bytes_ex(arr, dtypes, S, B, E, k, chunk, PREC[precision])
    assert nbytes == lib.drin_table_topk_sum_forms_workspace_bytes(arr, dtypes, None, S, B, E, k, chunk, PREC[precision]) > 0
    outs = []
    for call, head in ((lib.drin_table_topk_sum_ex, (arr, dtypes)), (lib.drin_table_topk_sum_forms, (arr, dtypes, None)),
                       (lib.drin_table_topk_sum_forms, (arr, None, (_lib.DrinTopkFormC * S)()))):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        scores, rows = torch.empty(B, k, device=DEV), torch.empty(B, k, dtype=torch.int64, device=DEV)
        _lib.check(call(*head, S, E, B, k, COS_EPS, PREC[precision], chunk, ptr(ws), nbytes, ptr(scores), ptr(rows), stream()))
        outs.append((scores, rows))
    for scores, rows in outs[1:]:
        assert torch.equal(rows, outs[0][1]) and same_bits(scores, outs[0][0])


# ---- 5. through the model --------------------------------------------------------------------------------------------------------
def ii_term(model, table, mention, weight):
    q, S = object_rows(mention[5][:, :, 0, :].contiguous(), mention[6].contiguous(), model.cfg.cosine_eps)
    u, T = table.object_rows(model.cfg)
    return RatioTerm(q, S, u, T, weight, model.cfg.miei_eps)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["wm", "wd"])                            # token-level and pooled tables
def test_link_with_four_weights_is_link_on_the_rows_of_the_four_terms(name, precision):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case(name, False, precision)
    cfg, N = c["cfg"], c["cfg"].num_candidates_model
    weights = (1.0, 1.0, 1.0, 1.0)
    terms = edge_terms(model, table, mention, clip_image, clip_text, weights[:3]) + [ii_term(model, table, mention, weights[3])]
    first = table_topk_sum(terms, N, cfg.cosine_eps, precision)
    got = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=weights)
    want = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=first.rows)
    assert torch.equal(got.rows, want.rows) and same_bits(got.scores, want.scores)
    assert tuple(got.rows.shape) == (3, K_LINK) and got.rows.dtype == torch.int64 and got.scores.dtype == torch.float32
    # the first stage ranks by the evidence the model reads: the four layer-0 edges of the forward on the gathered batch of those rows
    from drin_amd.model import IndexedBatch
    batch = IndexedBatch.from_clip(mention, table, first.rows, clip_image, clip_text, model=model)
    e0 = model.forward_traced(mention + table.gather(first.rows) + [batch.miet_similarity, batch.mtei_similarity])["edges0"]
    err = (first.scores - (e0[0] + e0[1] + e0[2] + e0[3])).abs().max().item()
    print(f"{name} {precision}: max |first-stage score - (tt + ti + it + ii of the forward)| = {err:.2e} (bar {tol_of(weights, 'f32'):.1e})")
    assert err <= tol_of(weights, "f32")
    # the table's u rows are built once across calls, and again after an in-place edit of object_score
    held = table._object_rows[1]
    model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=weights)
    assert table._object_rows[1] is held
    table.object_score.mul_(1.0)
    model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=weights)
    assert table._object_rows[1] is not held and same_bits(table._object_rows[1], held)
    assert table.invalidate()._object_rows is None


def test_ii_alone_links_without_reading_text_or_clip_rows():
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", False, "f32")
    cfg, N = c["cfg"], c["cfg"].num_candidates_model
    want = table_topk_sum([ii_term(model, table, mention, 1.0)], N, cfg.cosine_eps, "f32")
    nan = lambda t: torch.full_like(t, float("nan"))   # noqa: E731
    poisoned = EntityTable(nan(table.text), table.mask, table.image, table.object, table.object_score).set_clip(nan(table.clip_text),
                                                                                                                nan(table.clip_image))
    bad_mention = [nan(mention[0])] + list(mention[1:])
    rows = model._edge_candidates(bad_mention, poisoned, nan(clip_image), nan(clip_text), (0, 0, 0, 1))
    assert torch.equal(rows, want.rows) and bool(torch.isfinite(want.scores).all())
    assert rows[0].tolist() != list(range(N))                           # (a NaN score would list the first rows)
    through = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=(0, 0, 0, 1))
    assert torch.equal(through.rows, model.link(mention, table, K_LINK, clip_image, clip_text, candidates=want.rows).rows)


def test_four_weights_tell_apart_entities_that_differ_only_in_their_object_rows():
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wd", False, "f32")
    cfg, E = c["cfg"], table.num_entities
    twin = EntityTable(table.text.clone(), table.mask, table.image.clone(), table.object.clone(), table.object_score.clone())
    t_text, t_image = table.clip_text.clone(), table.clip_image.clone()
    for t in (twin.text, twin.image, t_text, t_image):
        t[1] = t[0]                                                     # entities 0 and 1: equal text, image and CLIP rows ...
    twin.object[1, 0] = mention[5][0, 1].reshape(twin.object[1, 0].shape)   # ... and entity 1 shows what mention 0 shows
    twin.set_clip(t_text, t_image)
    three = table_topk_sum(edge_terms(model, twin, mention, clip_image, clip_text, (1.0, 1.0, 1.0)), E, cfg.cosine_eps, "f32")
    four = table_topk_sum(edge_terms(model, twin, mention, clip_image, clip_text, (1.0, 1.0, 1.0)) + [ii_term(model, twin, mention, 1.0)],
                          E, cfg.cosine_eps, "f32")
    place = lambda res, row: int((res.rows[0] == row).nonzero()[0])   # noqa: E731
    assert place(three, 1) == place(three, 0) + 1 and three.scores[0, place(three, 0)] == three.scores[0, place(three, 1)]   # a tie: the lower row first
    assert place(four, 1) < place(four, 0) and four.scores[0, place(four, 1)] > four.scores[0, place(four, 0)]
    assert not torch.equal(model._edge_candidates(mention, twin, clip_image, clip_text, (1, 1, 1, 1)),
                           model._edge_candidates(mention, twin, clip_image, clip_text, (1, 1, 1)))


def test_three_weights_and_a_zero_fourth_give_todays_call_and_bits(monkeypatch):
    c, model, table, mention, _cand, clip_image, clip_text = gpu_case("wm", False, "bf16x3")
    cfg, N = c["cfg"], c["cfg"].num_candidates_model
    first = table_topk_sum(edge_terms(model, table, mention, clip_image, clip_text, (1.0, 0.5, 2.0)), N, cfg.cosine_eps, "bf16x3")
    want = model.link(mention, table, K_LINK, clip_image, clip_text, candidates=first.rows)
    lib, calls = _lib.load(), []
    real_sum, real_forms = lib.drin_table_topk_sum, lib.drin_table_topk_sum_forms
    monkeypatch.setattr(lib, "drin_table_topk_sum", lambda *a: (calls.append("sum"), real_sum(*a))[1])
    monkeypatch.setattr(lib, "drin_table_topk_sum_forms", lambda *a: (calls.append("forms"), real_forms(*a))[1])
    for weights in ((1.0, 0.5, 2.0), (1.0, 0.5, 2.0, 0.0)):
        got = model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=weights)
        assert torch.equal(got.rows, want.rows) and same_bits(got.scores, want.scores)
    assert calls == ["sum", "sum"] and table._object_rows is None       # the old entry point; the object rows were never built
    model.link(mention, table, K_LINK, clip_image, clip_text, first_stage="edges", edge_weights=(1.0, 0.5, 2.0, 1.0))
    assert calls == ["sum", "sum", "forms"]
