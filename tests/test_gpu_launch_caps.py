"""-m gpu: every launcher that stops growing its grid, run past that point (DESIGN.md section 29 holds the inventory).

Two mechanisms: a grid-stride kernel with a capped grid (beyond the cap a wave walks several rows and carries its column sums
across them) and a launch loop that cuts the batch into slices of 65 535 mentions - the grid.y limit - and re-bases every pointer
by the slice's first mention b0.  Every case takes its reference from a plain fp64 (or exact) restatement of the operation on the
same inputs, never from a second call of the library at another size, and every case shows that it did cross the cap: the
workgroup count read back from the scratch query, or two counted launches where a small call counts one.  Widths are the
narrowest at which a wrong multiplier shows (D = 8: b0 and b0 * D differ).

Bars are those of the sibling tests: fp32-FMA kernels 1e-5 of max|ref|, span means 1e-6, maxima, positions,
gathers and zero patterns exact.  A column sum over thousands of rows that misses 1e-5 while dh meets it is held to
eps32 * depth * sum|term| per column instead (column_sum_ok says how depth is counted) - the bound of the summation order, never
a looser constant.  Every test prints its measured maxima; profiles/launch_caps_parity.txt records them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from drin_amd import _lib
from tests.helpers import KERNEL_TOL, check_cosine, cos_case, ln_bwd, lowest_argmax, mention_rows_bwd, mention_rows_fwd, rel_err
from tests.step_restatement import cosine_rows64_grads

pytestmark = pytest.mark.gpu

DEV = "cuda"
AVG, MAX = _lib.REPR_AVG_EXTRACT, _lib.REPR_MAX_POOL
SPAN_TOL = 1e-6                                                       # tests/test_gpu_ghmfc_variants.py, tests/test_gpu_mention_rows.py
EPS32 = 2.0 ** -24                                                    # unit roundoff of fp32
SLICE = 65535                                                         # grid.y limit: mentions per launch of the sliced loops
B2 = SLICE + 6                                                        # a second slice of six mentions
ROW_CAP = 4 * SLICE * 16                                              # rows of one trip of the one-wave-per-row forward kernels
NAN = float("nan")
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)                      # noqa: E731
cdiv = lambda a, b: -(-a // b)                                         # noqa: E731


def launches(fn):
    """{kernel class: launches} of one call of fn, and what fn returned"""
    torch.cuda.synchronize()
    _lib.profile_begin()
    out = fn()
    torch.cuda.synchronize()
    return {k: n for k, (_ms, n) in _lib.profile_end().items() if n}, out


def column_sum_ok(got, ref, abs_terms, depth, what):
    """A column sum over rows: 1e-5 of max|ref|, or - only where that misses - |err| <= eps32 * depth * sum_rows |term| per column,
    sum|term| from the fp64 terms.  depth counts the roundings between a term and the stored sum: the serial additions of a
    wave's trips, two levels for the four waves, the serial additions of a lane over its share of the partial rows, two levels
    for the four lanes, and the roundings inside one term (the caller adds those)."""
    ratio = rel_err(got, ref, what)
    if ratio <= KERNEL_TOL:
        return True
    err = (got.double() - ref.double()).abs()
    bound = EPS32 * depth * abs_terms
    print(f"{what}: misses {KERNEL_TOL:g}; against eps32 * {depth} * sum|term| the worst column stands at {(err / bound).max().item():.3f} of its bound")
    return bool((err <= bound).all())


def sum_depth(rows, blocks):
    return cdiv(rows, 4 * blocks) + 2 + cdiv(blocks, 4) + 2


# ---- the GHMFC row backward beyond kRowBwdBlocks * 4 = 1024 rows ------------------------------------------------------------
def ln_case(rows, E, with_res, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(rows * 7 + E + seed)
    x = torch.randn(rows, E, device=DEV, generator=gen) * 1.5 + 0.3
    res = torch.randn(rows, E, device=DEV, generator=gen) if with_res else None
    gamma = torch.randn(E, device=DEV, generator=gen)
    gamma[::5] = 0.0
    beta = torch.randn(E, device=DEV, generator=gen)
    dy = torch.randn(rows, E, device=DEV, generator=gen)
    return x, res, gamma, beta, dy


def ln_fwd(x, res, gamma, beta, y=None, eps=1e-5):
    rows, E = x.shape
    y = torch.full_like(x, NAN) if y is None else y
    mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    _lib.check(_lib.load().drin_layernorm_res_train_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, E, eps,
                                                        stream()))
    return y, mean, rstd


def ln_fp64(x, res, gamma, beta, dy, eps=1e-5):
    h64 = (x.double() + (res.double() if res is not None else 0.0)).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu = h64.mean(-1, keepdim=True)
    var = ((h64 - mu) ** 2).mean(-1, keepdim=True)
    xhat = (h64 - mu) / torch.sqrt(var + eps)
    y64 = xhat * g64 + b64
    dh, dg, db = torch.autograd.grad((y64 * dy.double()).sum(), [h64, g64, b64])
    return y64.detach(), mu.detach()[:, 0], (1.0 / torch.sqrt(var + eps)).detach()[:, 0], dh, dg, db, xhat.detach()


LN_ROWS_WIDTHS = [(1025, 16), (1025, 260), (1025, 768), (1025, 2048),   # one wave takes two rows, the rest one; DV = 1, 2, 4, 8
                  (2051, 16), (2051, 260), (2051, 768),
                  (5003, 16), (5003, 260), (5003, 768)]                 # waves with 4 and with 5 rows in one launch; 256 partial rows


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,E", LN_ROWS_WIDTHS)
def test_layernorm_backward_past_the_grid_cap(rows, E, with_res):
    lib = _lib.load()
    blocks = lib.drin_layernorm_res_bwd_scratch_floats(rows, E) // (2 * E)
    assert 0 < blocks < cdiv(rows, 4), "the launch no longer strides: this case is back to one trip"
    x, res, gamma, beta, dy = ln_case(rows, E, with_res)
    y, mean, rstd = ln_fwd(x, res, gamma, beta)
    y64, mu64, rs64, ref_dh, ref_dg, ref_db, xhat64 = ln_fp64(x, res, gamma, beta, dy)
    tag = f"layernorm ({rows},{E}) res={with_res} blocks={blocks}"
    assert rel_err(y, y64, tag + " y") <= KERNEL_TOL
    assert rel_err(mean, mu64, tag + " mean", max(mu64.abs().max().item(), 1.0)) <= KERNEL_TOL
    assert rel_err(rstd, rs64, tag + " rstd") <= KERNEL_TOL
    dh, dgamma, dbeta = ln_bwd(x, res, mean, rstd, gamma, dy)
    assert rel_err(dh, ref_dh, tag + " dh") <= KERNEL_TOL
    depth = sum_depth(rows, blocks) + 6                               # a term dy * xhat: xhat = (h - mean) rstd from rounded h, mean, rstd
    assert column_sum_ok(dgamma, ref_dg, (dy.double() * xhat64).abs().sum(0), depth, tag + " dgamma")
    assert column_sum_ok(dbeta, ref_db, dy.double().abs().sum(0), depth, tag + " dbeta")
    frozen, none_g, none_b = ln_bwd(x, res, mean, rstd, gamma, dy, sums=False)
    assert none_g is None and none_b is None and torch.equal(bits(frozen), bits(dh))   # a frozen LayerNorm: the same dh bits
    again = ln_bwd(x, res, mean, rstd, gamma, dy)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (dh, dgamma, dbeta)))


@pytest.mark.parametrize("rows,E", [(37, 260), (1025, 768)])
def test_layernorm_aliased_outputs_give_the_same_bits(rows, E):
    """"y may be x or res" and "dh may be dy" (csrc/ghmfc_rows.hip): a wave holds its whole row before it stores."""
    x, res, gamma, beta, dy = ln_case(rows, E, True, seed=3)
    y, mean, rstd = ln_fwd(x, res, gamma, beta)
    ref = ln_fp64(x, res, gamma, beta, dy)
    assert rel_err(y, ref[0], f"layernorm alias ({rows},{E}) y") <= KERNEL_TOL
    xa = x.clone()
    ya, ma, ra = ln_fwd(xa, res, gamma, beta, y=xa)
    assert ya.data_ptr() == xa.data_ptr() and torch.equal(bits(ya), bits(y)) and torch.equal(bits(ma), bits(mean)) and torch.equal(bits(ra), bits(rstd))
    rb = res.clone()
    yb, mb, _ = ln_fwd(x, rb, gamma, beta, y=rb)
    assert torch.equal(bits(yb), bits(y)) and torch.equal(bits(mb), bits(mean))
    dh, dgamma, dbeta = ln_bwd(x, res, mean, rstd, gamma, dy)
    assert rel_err(dh, ref[3], f"layernorm alias ({rows},{E}) dh") <= KERNEL_TOL
    lib = _lib.load()
    floats = lib.drin_layernorm_res_bwd_scratch_floats(rows, E)
    dya = dy.clone()
    dg, db = torch.full((E,), NAN, device=DEV), torch.full((E,), NAN, device=DEV)
    scratch = torch.full((floats,), NAN, device=DEV)
    _lib.check(lib.drin_layernorm_res_bwd(ptr(x), ptr(res), ptr(mean), ptr(rstd), ptr(gamma), ptr(dya), ptr(dya), ptr(dg), ptr(db), ptr(scratch),
                                          floats, rows, E, stream()))
    assert torch.equal(bits(dya), bits(dh)) and torch.equal(bits(dg), bits(dgamma)) and torch.equal(bits(db), bits(dbeta))


GATE_SHAPES = [(5, 260), (5, 2048),                                   # DV = 2 and DV = 8 of k_gate_mix_bwd, inside one trip
               (1025, 16), (1025, 260), (1025, 768), (1025, 2048), (4099, 16), (4099, 260), (4099, 768)]


@pytest.mark.parametrize("B,D", GATE_SHAPES)
def test_gate_backward_past_the_grid_cap(B, D):
    lib = _lib.load()
    floats = lib.drin_gate_mix_bwd_scratch_floats(B, D)
    blocks = floats // (2 * D + 4)
    if B > 1024:
        assert 0 < blocks < cdiv(B, 4), "the launch no longer strides: this case is back to one trip"
    else:
        assert blocks == cdiv(B, 4)
    gen = torch.Generator(device=DEV).manual_seed(B * 31 + D)
    tl, vl, dout = (torch.randn(B, D, device=DEV, generator=gen) for _ in range(3))
    ws = torch.randn(2, 2 * D, device=DEV, generator=gen) / math.sqrt(2 * D)
    bs = torch.randn(2, device=DEV, generator=gen)
    ws[1], bs[1] = ws[0], bs[0]
    ws[1, 1:] += 0.05 * torch.randn(2 * D - 1, device=DEV, generator=gen)
    tl[B - 1], vl[B - 1] = 0.0, 0.0                                   # gelu(0) = 0: the last mention's two logits are both bs[0]
    out = torch.full((B, D), NAN, device=DEV)
    _lib.check(lib.drin_gate_mix_fwd(ptr(tl), ptr(vl), ptr(ws), ptr(bs), ptr(out), B, D, stream()))
    leaves = [t.double().requires_grad_(True) for t in (tl, vl, ws, bs)]
    gelu = lambda a: 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))   # noqa: E731
    t, v = gelu(leaves[0]), gelu(leaves[1])
    z = torch.cat([t, v], 1) @ leaves[2].T + leaves[3]
    assert z[B - 1, 0].item() == z[B - 1, 1].item()
    s = torch.softmax(z, 1)
    out64 = s[:, :1] * t + s[:, 1:] * v
    refs = torch.autograd.grad((out64 * dout.double()).sum(), leaves)
    tag = f"gate ({B},{D}) blocks={blocks}"
    assert rel_err(out, out64.detach(), tag + " out") <= KERNEL_TOL

    def run(sums=True):
        dtl, dvl = torch.full_like(tl, NAN), torch.full_like(vl, NAN)
        dws, dbs = (torch.full_like(ws, NAN), torch.full_like(bs, NAN)) if sums else (None, None)
        scratch = torch.full((floats,), NAN, device=DEV) if sums else None
        _lib.check(lib.drin_gate_mix_bwd(ptr(tl), ptr(vl), ptr(ws), ptr(bs), ptr(dout), ptr(dtl), ptr(dvl), ptr(dws), ptr(dbs), ptr(scratch),
                                         floats if sums else 0, B, D, stream()))
        return dtl, dvl, dws, dbs

    got = run()
    assert rel_err(got[0], refs[0], tag + " dtl") <= KERNEL_TOL and rel_err(got[1], refs[1], tag + " dvl") <= KERNEL_TOL
    # a term of the sums is dz0 * [t | v | 1], dz0 = s0 s1 sum_c dout_c (t_c - v_c): its size is bounded with the absolute sum (no
    # cancellation assumed); its roundings: a 2 D-term dot product per logit in lane order (D / 256 + 6 levels), gelu, exp, the
    # quotient and the products (10)
    with torch.no_grad():
        dz_abs = (s[:, 0] * s[:, 1] * (dout.double() * (t - v)).abs().sum(1))[:, None]
        abs_w = torch.cat([(dz_abs * t.abs()).sum(0), (dz_abs * v.abs()).sum(0)])
        abs_terms_w = torch.stack([abs_w, abs_w])
        abs_terms_b = dz_abs.sum().expand(2)
    depth = sum_depth(B, blocks) + cdiv(D, 256) + 6 + 10
    assert column_sum_ok(got[2], refs[2], abs_terms_w, depth, tag + " dws")
    assert column_sum_ok(got[3], refs[3], abs_terms_b, depth, tag + " dbs")
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(run(), got))
    frozen = run(sums=False)
    assert torch.equal(bits(frozen[0]), bits(got[0])) and torch.equal(bits(frozen[1]), bits(got[1])) and frozen[2] is None


# ---- past 65 535 mentions through the per-operation entry points --------------------------------------------------------------
SPAN_FORMS = [(1, 2), (3, 9), (0, 12), (8, 20), (4, 4), (-3, -1), (-20, 3), (2, 9), (0, 1)]   # test_span_mean_forward_and_backward's, and two more


def span_bounds(B, L, empty_at=()):
    """(start, end int64 [B] on the device, lo, hi: the bounds as a Python slice of L positions clips them)"""
    forms = torch.tensor(SPAN_FORMS, dtype=torch.int64)
    rows = forms[torch.arange(B) % len(SPAN_FORMS)]
    for b in empty_at:
        rows[b] = torch.tensor([4, 4])
    start, end = rows[:, 0].contiguous(), rows[:, 1].contiguous()
    clip = lambda p: torch.where(p < 0, (p + L).clamp(min=0), p.clamp(max=L))   # noqa: E731
    lo, hi = clip(start), clip(end)
    for b in (0, 1, 5, B // 2, B - 2, B - 1):
        s, e = slice(int(start[b]), int(end[b])).indices(L)[:2]
        assert (int(lo[b]), int(hi[b])) == (s, e) or (e <= s and int(hi[b]) <= int(lo[b]))
    return start.to(DEV), end.to(DEV), lo.to(DEV), hi.to(DEV)                 # (the loop: the restatement against Python's own slice)


def span_mean64(x, lo, hi):
    """[B, D] fp64: mean of x[b, lo:hi]; NaN rows where the span is empty"""
    L = x.shape[1]
    pos = torch.arange(L, device=x.device)[None, :]
    inside = ((pos >= lo[:, None]) & (pos < hi[:, None])).double()
    cnt = (hi - lo).clamp(min=0).double()
    return (x.double() * inside[:, :, None]).sum(1) / cnt[:, None]   # 0 / 0 = NaN


def span_scatter64(g, lo, hi, L):
    """[B, L, D] fp64: g[b] / (hi - lo) inside the span, 0 elsewhere (and everywhere for an empty span)"""
    pos = torch.arange(L, device=g.device)[None, :]
    inside = ((pos >= lo[:, None]) & (pos < hi[:, None])).double()
    cnt = (hi - lo).clamp(min=1).double()
    return inside[:, :, None] * (g.double() / cnt[:, None])[:, None, :]


def test_span_mean_second_slice():
    lib, B, L, D = _lib.load(), B2, 3, 8
    start, end, lo, hi = span_bounds(B, L, empty_at=(SLICE + 2,))
    empty = hi <= lo
    assert bool(empty[SLICE + 2]) and not bool(empty[SLICE:].all()) and bool(empty[:SLICE].any())
    gen = torch.Generator(device=DEV).manual_seed(11)
    seq, dout = torch.randn(B, L, D, device=DEV, generator=gen), torch.randn(B, D, device=DEV, generator=gen)

    def run(n):
        out, dseq = torch.full((n, D), 7.0, device=DEV), torch.full((n, L, D), NAN, device=DEV)
        _lib.check(lib.drin_span_mean_fwd(ptr(seq), ptr(start), ptr(end), ptr(out), n, L, D, stream()))
        _lib.check(lib.drin_span_mean_bwd(ptr(dout), ptr(start), ptr(end), ptr(dseq), n, L, D, stream()))
        return out, dseq

    small, _ = launches(lambda: run(5))
    counted, (out, dseq) = launches(lambda: run(B))
    assert small == {"pool": 2} and counted == {"pool": 4}, (small, counted)   # forward and backward: one launch each, two past 65 535
    ref_out, ref_dseq = span_mean64(seq, lo, hi), span_scatter64(dout, lo, hi, L)
    assert torch.equal(torch.isnan(out), empty[:, None].expand(B, D)) and torch.equal(torch.isnan(ref_out), torch.isnan(out))
    assert not torch.isnan(dseq).any() and not dseq[empty].any()      # every element written; the empty span: a block of zeros
    for name, part in (("first slice", slice(0, SLICE)), ("second slice", slice(SLICE, B))):
        live = ~empty[part]
        assert rel_err(out[part][live], ref_out[part][live], f"span_mean B={B} {name} out") <= SPAN_TOL
        assert rel_err(dseq[part], ref_dseq[part], f"span_mean B={B} {name} dseq") <= SPAN_TOL
    assert torch.equal(dseq != 0, ref_dseq != 0)                      # exact zeros outside the span


def planted_rows(B, L, D, seed):
    """[B, L, D] normal deviates with NaNs, ties and signed zeros in the first mentions AND past mention 65 535"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, L, D, device=DEV, generator=g)
    for b in (0, SLICE + 2):
        x[b, L - 1, 0] = NAN                                          # a NaN wins, at the last position
        x[b, :, 2] = -0.0                                             # signed zeros: every position ties
        x[b, L // 2, 2] = 0.0
    for b in (1, B - 1):
        x[b, :, 1] = 2.0                                              # a tie over the whole column: position 0
        x[b, :, 3] = -1.0
        x[b, L - 2:, 3] = 5.0                                         # a tie of the last two positions: the lower one
    return x, g


@pytest.mark.parametrize("with_encoded", [False, True])
def test_mention_rows_max_second_slice(with_encoded):
    B, L, D = B2, 5, 8
    raw, g = planted_rows(B, L, D, 21)
    enc = None
    if with_encoded:
        enc = torch.randn(B, L, D, device=DEV, generator=g)
        enc[SLICE + 1, 0, 0] = NAN
        enc[B - 1, :, 1] = -3.0
    small, _ = launches(lambda: mention_rows_fwd(raw[:5].contiguous(), None if enc is None else enc[:5].contiguous(), None, None, MAX))
    counted, (edge, vert, idx) = launches(lambda: mention_rows_fwd(raw, enc, None, None, MAX))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    for x, row, at, name in ((raw, edge, idx[0], "edge"), (enc if with_encoded else raw, vert, idx[1], "vertex")):
        ref, _ = torch.max(x, dim=1)
        assert torch.equal(row.nan_to_num(7.5), ref.nan_to_num(7.5)), name
        assert torch.equal(torch.isnan(row), torch.isnan(x).any(1)), name
        assert torch.equal(at.long(), lowest_argmax(x)), name         # both planes of max_index, the second at batch * width
    assert int(idx[0][SLICE + 2, 0]) == L - 1 and int(idx[0][B - 1, 1]) == 0 and int(idx[0][SLICE + 2, 2]) == 0 and int(idx[0][B - 1, 3]) == L - 2
    # backward: exact scatter of the rows' gradients to the positions of the two planes
    ge, gv = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, D, device=DEV, generator=g)
    shape = (B, L, D)
    small, _ = launches(lambda: mention_rows_bwd(ge, gv, None, None, idx[:, :5].contiguous(), MAX, int(with_encoded), (5, L, D),
                                                 want_enc=with_encoded))
    counted, (d_raw, d_enc) = launches(lambda: mention_rows_bwd(ge, gv, None, None, idx, MAX, int(with_encoded), shape, want_enc=with_encoded))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    zeros = torch.zeros(shape, device=DEV)
    s_edge = zeros.clone().scatter_(1, idx[0][:, None, :].long(), ge[:, None, :])
    s_vert = zeros.clone().scatter_(1, idx[1][:, None, :].long(), gv[:, None, :])
    if with_encoded:
        assert torch.equal(bits(d_raw), bits(s_edge)) and torch.equal(bits(d_enc), bits(s_vert))
    else:
        assert d_enc is None
        want = s_edge.double() + s_vert.double()                      # both rows are functions of the raw block: one write of the sum
        assert rel_err(d_raw, want, f"mention_rows_bwd max B={B} both-in-one") <= SPAN_TOL
        assert torch.equal(d_raw != 0, want != 0)


@pytest.mark.parametrize("with_encoded,raw_dtype", [(False, torch.float32), (True, torch.float32), (True, torch.bfloat16)])
def test_mention_rows_avg_second_slice(with_encoded, raw_dtype):
    B, L, D = B2, 5, 8
    raw, g = planted_rows(B, L, D, 31)
    raw = raw.nan_to_num(0.25).to(raw_dtype)
    enc = torch.randn(B, L, D, device=DEV, generator=g) if with_encoded else None
    start, end, lo, hi = span_bounds(B, L, empty_at=(SLICE + 2,))
    empty = hi <= lo
    five = lambda t: None if t is None else t[:5].contiguous()       # noqa: E731
    small, _ = launches(lambda: mention_rows_fwd(five(raw), five(enc), five(start), five(end), AVG))
    counted, (edge, vert, idx) = launches(lambda: mention_rows_fwd(raw, enc, start, end, AVG))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    assert (idx == -5).all()
    tag = f"mention_rows avg B={B} enc={with_encoded} {str(raw_dtype).split('.')[-1]}"
    for x, row, name in ((raw, edge, "edge"), (enc if with_encoded else raw, vert, "vertex")):
        ref = span_mean64(x.float(), lo, hi)                          # bf16 widens exactly
        assert torch.equal(torch.isnan(row), empty[:, None].expand(B, D)), name
        for part_name, part in (("first slice", slice(0, SLICE)), ("second slice", slice(SLICE, B))):
            live = ~empty[part]
            assert rel_err(row[part][live], ref[part][live], f"{tag} {name} {part_name}") <= SPAN_TOL
    ge, gv = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, D, device=DEV, generator=g)
    small, _ = launches(lambda: mention_rows_bwd(five(ge), five(gv), five(start), five(end), None, AVG, int(with_encoded), (5, L, D),
                                                 want_enc=with_encoded))
    counted, (d_raw, d_enc) = launches(lambda: mention_rows_bwd(ge, gv, start, end, None, AVG, int(with_encoded), (B, L, D),
                                                                want_enc=with_encoded))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    r_edge, r_vert = span_scatter64(ge, lo, hi, L), span_scatter64(gv, lo, hi, L)
    want_raw = r_edge if with_encoded else r_edge + r_vert
    assert not torch.isnan(d_raw).any()
    for part_name, part in (("first slice", slice(0, SLICE)), ("second slice", slice(SLICE, B))):
        assert rel_err(d_raw[part], want_raw[part], f"{tag} d_raw {part_name}") <= SPAN_TOL
        if with_encoded:
            assert rel_err(d_enc[part], r_vert[part], f"{tag} d_enc {part_name}") <= SPAN_TOL
    inside = span_scatter64(torch.ones(B, D, device=DEV), lo, hi, L) != 0
    assert not d_raw[~inside].any() and (not with_encoded or not d_enc[~inside].any())   # exact zeros outside the span


def test_cosine_rows_flat_pair_grid_and_sliced_mention_kernel():
    """B > 65 535: k_cosine_rows and k_cosine_bwd_entity take the flat pair grid (b = p / N with b > 0: at B = 1 it is always 0),
    k_cosine_bwd_mention runs in two slices whose pointers move by b0 * D, b0 * N * D and b0 * N."""
    B, N, D = B2, 3, 8
    x, y, dout = cos_case(B, N, D, 97)
    small, _ = launches(lambda: check_cosine(x[:5], y[:5], dout[:5], 1e-8, "cosine (5,3,8)"))
    counted, (out, dx, dy) = launches(lambda: check_cosine(x, y, dout, 1e-8, f"cosine ({B},{N},{D})"))
    # check_cosine: forward twice, backward twice directly, forward and backward once through row_ops, a refused backward
    assert small == {"edge": 3, "gcn": 3 * 2} and counted == {"edge": 3, "gcn": 3 * 3}, (small, counted)
    out64, dx64, dy64 = cosine_rows64_grads(x[SLICE:], y[SLICE:], dout[SLICE:], 1e-8)
    assert (out[SLICE:].double().cpu() - out64).abs().max().item() <= KERNEL_TOL * out64.abs().max().item()
    for got, ref, name in ((dx[SLICE:], dx64, "dx"), (dy[SLICE:], dy64, "dy")):   # the six mentions of the second slice, by themselves
        assert rel_err(got.cpu(), ref, f"cosine ({B},{N},{D}) second slice {name}") <= KERNEL_TOL


def test_cosine_rows_indexed_flat_pair_grid_reports_a_clamped_index():
    lib, B, N, D, E = _lib.load(), B2, 3, 8, 9
    g = torch.Generator().manual_seed(5)
    x, rows = torch.randn(B, D, generator=g), torch.randn(E, D, generator=g)
    index = torch.randint(0, E, (B, N), generator=g)
    bad = (SLICE + 3, 1)
    index[bad] = 12                                                   # clamped to row 8, reported with its pair
    xd, rd, idx = x.to(DEV), rows.to(DEV), index.to(DEV)
    out = torch.full((B, N), NAN, device=DEV)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    counted, _ = launches(lambda: _lib.check(lib.drin_cosine_rows_indexed_fwd(ptr(xd), ptr(rd), ptr(idx), E, ptr(out), B, N, D, 1e-8, ptr(status),
                                                                          stream())))
    assert counted == {"edge": 1}
    yy = rows.double()[index.clamp(0, E - 1)]
    ref = (x.double()[:, None, :] * yy).sum(-1) / (x.double().norm(dim=-1)[:, None].clamp(min=1e-8) * yy.norm(dim=-1).clamp(min=1e-8))
    assert rel_err(out.cpu(), ref, f"indexed cosine ({B},{N},{D})") <= KERNEL_TOL
    assert rel_err(out[SLICE:].cpu(), ref[SLICE:], f"indexed cosine ({B},{N},{D}) mentions past 65535") <= KERNEL_TOL
    assert status.cpu().tolist() == [1, bad[0] * N + bad[1], 12, 0]
    assert lib.drin_index_status(status.data_ptr(), stream()) == _lib.E_INDEX
    msg = lib.drin_last_error().decode()
    assert "row 12" in msg and f"pair {bad[0] * N + bad[1]}" in msg, msg


def test_seq_max_at_the_largest_admitted_batch():
    lib, B, S, E = _lib.load(), SLICE, 2, 8
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, S, E)).astype(np.float32)
    for b in (0, B - 1):
        x[b, 1, 0] = x[b, 0, 0]                                       # a tie: the first position
        x[b, 1, 1] = np.nan                                           # a NaN wins
        x[b, :, 2] = np.nan                                           # two NaNs: the lowest position
        x[b, :, 3] = [0.0, -0.0]                                      # signed zeros are equal
        x[b, :, 4] = -np.inf
    xt = torch.from_numpy(x).to(DEV)
    out, idx = torch.full((B, E), 7.0, device=DEV), torch.full((B, E), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.drin_seq_max_train_fwd(ptr(xt), ptr(out), ptr(idx), B, S, E, stream()))
    want_idx = np.argmax(x, axis=1)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    want = np.take_along_axis(x, want_idx[:, None, :], 1)[:, 0, :]
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    dout = torch.randn(B, E, device=DEV)
    dx = torch.full((B, S, E), NAN, device=DEV)
    _lib.check(lib.drin_seq_max_bwd(ptr(dout), ptr(idx), ptr(dx), B, S, E, stream()))
    want_dx = torch.zeros(B, S, E, device=DEV).scatter_(1, idx.long()[:, None, :], dout[:, None, :])
    assert torch.equal(bits(dx), bits(want_dx))
    assert lib.drin_seq_max_train_fwd(ptr(xt), ptr(out), ptr(idx), B + 1, S, E, stream()) == _lib.E_SHAPE   # one more: refused


# ---- the 4 * 65535 * 16-row cap of the one-wave-per-row forward kernels ---------------------------------------------------------
BIG_ROWS = ROW_CAP + 5                                                # 4 194 245: five waves take a second row


def sample_rows(rows):
    """the last 8 rows, the 5 past the cap with the 3 before it, and a strided sample"""
    return torch.cat([torch.arange(rows - 8, rows), torch.arange(ROW_CAP - 3, ROW_CAP + 5), torch.arange(0, rows, 4099)]).to(DEV)


def test_layernorm_forward_past_the_row_cap():
    """Width 4, rows of spread >= 1 (alternating signs around a row offset): a row of four nearly equal deviates, of which four million
    draws hold some, would measure the cancellation in x - mean, not the kernel."""
    rows, E = BIG_ROWS, 4
    assert rows > ROW_CAP
    gen = torch.Generator(device=DEV).manual_seed(9)
    sign = torch.tensor([-1.0, 1.0, -1.0, 1.0], device=DEV)
    x = sign * (1.0 + 0.5 * torch.rand(rows, E, device=DEV, generator=gen)) + 0.3 * torch.randn(rows, 1, device=DEV, generator=gen)
    gamma, beta = torch.tensor([1.5, -0.5, 0.0, 2.0], device=DEV), torch.tensor([0.1, 0.2, -0.3, 0.4], device=DEV)
    y, mean, rstd = ln_fwd(x, None, gamma, beta)
    h = x.double()
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + 1e-5)
    y64 = (h - mu) * rs * gamma.double() + beta.double()
    at = sample_rows(rows)
    tag = f"layernorm forward ({rows},{E})"
    assert rel_err(y[at], y64[at], tag + " y, sampled rows") <= KERNEL_TOL
    assert rel_err(y[ROW_CAP:], y64[ROW_CAP:], tag + " y, rows past the cap") <= KERNEL_TOL
    assert rel_err(y, y64, tag + " y") <= KERNEL_TOL
    assert rel_err(mean, mu[:, 0], tag + " mean", max(mu.abs().max().item(), 1.0)) <= KERNEL_TOL
    assert rel_err(rstd, rs[:, 0], tag + " rstd") <= KERNEL_TOL
    assert rel_err(rstd[ROW_CAP:], rs[ROW_CAP:, 0], tag + " rstd, rows past the cap") <= KERNEL_TOL


def test_gather_rows_past_the_row_cap():
    lib, count, E, W = _lib.load(), BIG_ROWS, 9, 4
    table = torch.randn(E, W, device=DEV)
    index = (torch.arange(count, device=DEV) * 7 + torch.arange(count, device=DEV) // 5) % E
    out = torch.full((count, W), NAN, device=DEV)
    counted, _ = launches(lambda: _lib.check(lib.drin_gather_rows(ptr(table), ptr(index), E, ptr(out), count, W, None, stream())))
    assert counted == {"pool": 1}
    at = sample_rows(count)
    assert torch.equal(bits(out[at]), bits(table[index[at]]))
    assert torch.equal(bits(out), bits(table[index]))


def test_row_inv_norms_past_the_row_cap():
    lib, rows, D, eps = _lib.load(), BIG_ROWS, 4, 1e-8
    x = torch.randn(rows, D, device=DEV)
    x[rows - 1] = 0.0                                                 # a clamped norm past the cap: 1 / eps
    out = torch.full((rows,), NAN, device=DEV)
    _lib.check(lib.drin_row_inv_norms(ptr(x), rows, D, eps, ptr(out), stream()))
    ref = 1.0 / x.double().norm(dim=-1).clamp(min=eps)
    at = sample_rows(rows)
    err = ((out.double() - ref).abs() / ref).max().item()            # each element against its own value: they span 1e8
    print(f"row_inv_norms ({rows},{D}): worst relative error {err:.2e}; sampled rows {((out[at].double() - ref[at]).abs() / ref[at]).max().item():.2e}")
    assert err <= KERNEL_TOL and out[rows - 1].item() > 9e7


# ---- drin_pool_fwd: the image means past 65 535 groups -------------------------------------------------------------------------
def pool_config(B, N, R, regions, inner):
    c = _lib.DrinConfigC()
    _lib.check(_lib.load().drin_default_config(C.byref(c)))
    c.batch, c.num_candidates, c.embed_dim, c.image_dim = B, N, 8, R
    c.mention_tokens, c.image_regions, c.entity_image_inner, c.entity_tokens = 1, regions, inner, 0
    return c


def pool_fwd(c, mention_image=None, entity_image=None):
    lib, b = _lib.load(), _lib.DrinBatchC()
    R = c.image_dim
    out_m = torch.full((c.batch, R), NAN, device=DEV) if mention_image is not None else None
    out_e = torch.full((c.batch, c.num_candidates, R), NAN, device=DEV) if entity_image is not None else None
    b.mention_image = mention_image.data_ptr() if mention_image is not None else None
    b.entity_image = entity_image.data_ptr() if entity_image is not None else None
    _lib.check(lib.drin_pool_fwd(C.byref(c), C.byref(b), None, ptr(out_m), ptr(out_e), stream()))
    return out_m, out_e


def test_pool_fwd_image_means_past_65535_groups():
    """launch_axis_mean_t folds its groups in chunks of 65 535 (input moves by g0 * inner * cols, output by g0 * cols): the entity
    image mean over B N = 72 094 pairs and the mention image mean over 65 541 mentions.  Bar: the span mean's 1e-6 of max|ref| -
    one fp32 addition and one division per element here."""
    R = 8
    gen = torch.Generator(device=DEV).manual_seed(4)
    B, N = 6554, 11
    assert B * N > SLICE
    eimg = torch.randn(B, N, 2, R, device=DEV, generator=gen)
    small, _ = launches(lambda: pool_fwd(pool_config(5, N, R, 2, 2), entity_image=eimg))
    counted, (_, out_e) = launches(lambda: pool_fwd(pool_config(B, N, R, 2, 2), entity_image=eimg))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    ref = eimg.double().mean(2)
    assert rel_err(out_e, ref, f"entity image mean ({B},{N},2,{R})") <= SPAN_TOL
    flat_o, flat_r = out_e.view(-1, R), ref.view(-1, R)
    assert rel_err(flat_o[SLICE:], flat_r[SLICE:], f"entity image mean ({B},{N},2,{R}) pairs past 65535") <= SPAN_TOL
    mimg = torch.randn(B2, 2, R, device=DEV, generator=gen)
    small, _ = launches(lambda: pool_fwd(pool_config(5, 1, R, 2, 0), mention_image=mimg))
    counted, (out_m, _) = launches(lambda: pool_fwd(pool_config(B2, 1, R, 2, 0), mention_image=mimg))
    assert small == {"pool": 1} and counted == {"pool": 2}, (small, counted)
    ref = mimg.double().mean(1)
    assert rel_err(out_m, ref, f"mention image mean ({B2},2,{R})") <= SPAN_TOL
    assert rel_err(out_m[SLICE:], ref[SLICE:], f"mention image mean ({B2},2,{R}) mentions past 65535") <= SPAN_TOL


# ---- drin_table_topk: k_pad_rows past 4096 workgroups ----------------------------------------------------------------------------
def test_table_topk_pad_rows_stride():
    """B D = 5505 x 768 > 4 194 304 floats: k_pad_rows (4096 workgroups of 256 float4) takes a second trip, and B = 5505 leaves three
    zero rows behind it.  The ranking against fp64 as test_table_topk_against_fp64 holds it (f32: 1e-5)."""
    from tests.test_gpu_ghmfc_table import same_bits
    from tests.test_gpu_table_topk import TOL, dev, holds_rule, indexed_cosine, inv_norms, is_contract_ordered, table_topk, whole_case
    D, E, B, k = 768, 64, 5505, 5
    assert B * D > 4096 * 256 * 4 and B % 4
    x, rows, ref = whole_case(D, E, B, seed=2)
    x_t, rows_t = dev(x), dev(rows)
    inv_t = inv_norms(rows_t)
    scores, best = table_topk(x_t, rows_t, inv_t, k, "f32", 0)
    got_rows, got_scores = best.cpu().numpy(), scores.cpu().numpy()
    what = f"D{D} E{E} B{B} k{k} f32"
    assert got_rows.min() >= 0 and got_rows.max() <= E - 1 and all(len(set(r)) == k for r in got_rows.tolist()), what
    holds_rule(ref, got_rows, k, TOL["f32"], what)
    assert same_bits(scores, indexed_cosine(x_t, rows_t, best)), what
    assert is_contract_ordered(got_scores, got_rows), what
    err = np.abs(got_scores - np.take_along_axis(ref, got_rows, 1))
    print(f"{what}: max |returned score - fp64| = {err.max():.3e}; mentions of the second trip {err[4096 * 256 * 4 // D:].max():.3e}")
    assert err.max() <= TOL["f32"]


# ---- drin_forward_cached: k_check_entity_index past 2048 workgroups ----------------------------------------------------------------
def test_cached_forward_reports_a_bad_row_past_524288_pairs():
    """k_check_entity_index walks the B N candidate rows with at most 2048 workgroups of 256 threads: pair 524 288 is the first of
    the second trip.  One row outside the table behind it must be reported with its pair and value; without it, nothing is."""
    from drin_amd import synth
    from drin_amd.config import DrinConfig
    from drin_amd.model import EntityTable, IndexedBatch, Model
    from oracle.cases import TINY
    E, B = 30, 4100
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=127, max_entity_attr_token_len=6, **TINY)
    N = cfg.num_candidates_model
    assert B * N > 2048 * 256
    tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1), 1, 5)
    table = EntityTable(tab[7][0], tab[8][0], tab[9][0], tab[10][0], tab[11][0]).to(DEV)
    table.enable_cache()
    men = [t.to(DEV) for t in synth.make_batch(cfg.with_(num_candidates_data=1), B, 6)[:7]]
    g = torch.Generator().manual_seed(1)
    cand = torch.randint(0, E, (B, N), generator=g)
    miet, mtei = torch.randn(B, N, generator=g).to(DEV), torch.randn(B, N, generator=g).to(DEV)
    model = Model(cfg, precision="bf16x3_all").to(DEV).eval()
    model.load_state_dict(synth.make_state_dict(cfg, 8))
    model.validate_indices = False
    bad_pair = 2048 * 256 + 77
    bad = cand.clone()
    bad.view(-1)[bad_pair] = E + 9
    with torch.no_grad():
        counted, s_good = launches(lambda: model(IndexedBatch(men, table, cand.to(DEV), miet, mtei)))
        model.check_indices()                                         # nothing to report
        s_bad = model(IndexedBatch(men, table, bad.to(DEV), miet, mtei))
        with pytest.raises(IndexError, match=rf"row {E + 9} at pair {bad_pair} "):
            model.check_indices()
    assert tuple(s_good.shape) == (B, N) and torch.isfinite(s_good).all()
    same = torch.ones(B, dtype=torch.bool, device=DEV)
    same[bad_pair // N] = False                                       # (a mention's candidates meet in its sums: that mention's row differs)
    assert torch.equal(s_bad[same], s_good[same])                     # every other mention: the same bits


# ---- drin_forward / drin_backward above 65 535 mentions, through the C ABI ----------------------------------------------------------
# api.hip makes the calls it makes below the cap; the launchers differ there (launch_layer_aggregate and
# launch_mention_reduce2[_pair] move their pointers to a second slice, the text / image and edge-type strides those of the whole
# batch; the one-wave-per-pair kernels on the flat grid; every per-mention launch in two slices).  Reference: the fp64 oracle on the same batch, at the bars of tests/test_gpu_parity.py (scores 1e-4, every
# parameter gradient 2e-4 of its norm); second, the same batch sent as slices of Model.MAX_CALL_MENTIONS mentions - scores to the
# 5e-6 re-association bound documented there, the summed gradients to the gradient bar.
ABI_VARIANTS = {"dynamic": {}, "static": dict(gcn_edge_type="static"), "vector": dict(gcn_edge_feature="vector"),
                "vector_static": dict(gcn_edge_feature="vector", gcn_edge_type="static"),
                "tokens3": dict(dataset_name="wikimel", max_entity_attr_token_len=3)}
ABI_SCORE_TOL, ABI_GRAD_TOL, ABI_SLICE_TOL = 1e-4, 2e-4, 5e-6
SENTINEL = -7.25


class AbiCase:
    """One configuration at B2 mentions: batch, parameters, the fp64 oracle's scores and gradients of sum(scores * G)."""

    def __init__(self, kind, mention_objects=1):
        from drin_amd import synth
        from drin_amd.config import DrinConfig
        from drin_amd.model import Model, _param_list
        from oracle import drin_oracle as O
        self.kind = kind
        self.cfg = DrinConfig(num_candidates_data=1, bert_embed_dim=8, gcn_embed_dim=8, resnet_embed_dim=8, max_mention_sentence_len=2,
                              resnet_num_region=1, object_topk_mention=mention_objects, object_topk_entity=1, num_gcn_layers=2,
                              **ABI_VARIANTS[kind])
        sd = synth.make_state_dict(self.cfg, 3)
        batch = synth.make_batch(self.cfg, B2, 9)[:14]
        g = torch.Generator().manual_seed(2)
        batch[2] = torch.randint(0, 2, (B2,), generator=g)             # the span: position 0 or 1, so that mentions differ in it
        batch[3] = batch[2] + 1
        batch[6], batch[11] = 0.25 + 0.75 * batch[6], 0.25 + 0.75 * batch[11]   # object scores in [0.25, 1]: see the input-gradient test
        self.G = torch.randn(B2, self.cfg.num_candidates_model, generator=g)
        p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        scores = O.forward(p, batch, dtype=torch.float64, **O.config_kwargs(self.cfg))
        grads = torch.autograd.grad((scores * self.G.double()).sum(), list(p.values()), allow_unused=True)
        self.ref_scores, self.ref_grads = scores.detach(), dict(zip(p, grads))
        self.sd, self.cpu_batch = sd, batch
        self.model = Model(self.cfg, precision="f32").to(DEV)
        self.model.load_state_dict(sd)
        self.names = {id(q): k for k, q in self.model.named_parameters()}
        self.params = tuple(q.detach().contiguous() for q in _param_list(self.model))
        self.keys = [self.names[id(q)] for q in _param_list(self.model)]
        self.batch = [t.to(DEV) for t in batch]

    def call(self, lo=0, hi=B2, grads=None, backward=True):
        """drin_forward (keep_for_backward) and drin_backward on mentions [lo, hi); the gradients are ADDED to `grads`.
        -> (scores, grads, status of the backward, workspace, its copy before the backward)"""
        from drin_amd.model import _Call, _fill_params
        lib = _lib.load()
        xs = [t[lo:hi].contiguous() for t in self.batch]
        call = _Call(self.model.cfg, xs, _lib.PREC_F32)
        pc, gc = _lib.DrinParamsC(), _lib.DrinParamGradsC()
        _fill_params(pc, self.params, call.per_layer)
        ws = call.workspace(True)
        scores = torch.full((call.B, call.N), NAN, device=DEV)
        _lib.check(lib.drin_forward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), scores.data_ptr(), 1, None,
                                    stream()))
        grads = [torch.zeros_like(q) for q in self.params] if grads is None else grads
        _fill_params(gc, grads, call.per_layer)
        g = self.G[lo:hi].contiguous().to(DEV)
        if not backward:
            return scores, grads, None, ws, None
        torch.cuda.synchronize()
        before = ws.clone()
        status = lib.drin_backward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), g.data_ptr(), C.byref(gc),
                                   stream())
        torch.cuda.synchronize()
        return scores, grads, status, ws, before

    def check_grads(self, grads, tag):
        worst = 0.0
        for k, got in zip(self.keys, grads):
            ref = self.ref_grads[k]
            if ref is None:
                assert not got.any(), f"{k}: no gradient in the oracle, not zero here"
                continue
            rel = (got.double().cpu() - ref).norm().item() / (ref.norm().item() + 1e-300)
            worst = max(worst, rel)
            assert rel <= ABI_GRAD_TOL, (k, rel)
        print(f"{tag}: worst parameter gradient {worst:.2e} of its norm against the fp64 oracle")

    def input_grads(self):
        """{field: gradient} of every float batch tensor through drin_backward_ex (no parameter gradients), outputs NaN-poisoned"""
        from drin_amd.model import _Call, _fill_params
        from tests.test_gpu_input_grads import FLOAT_INPUTS
        lib = _lib.load()
        call = _Call(self.model.cfg, self.batch, _lib.PREC_F32)
        pc = _lib.DrinParamsC()
        _fill_params(pc, self.params, call.per_layer)
        ws = call.workspace(True)
        scores = torch.full((call.B, call.N), NAN, device=DEV)
        _lib.check(lib.drin_forward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), scores.data_ptr(), 1, None,
                                    stream()))
        outs = {f: torch.full(tuple(self.batch[i].shape), NAN, device=DEV) for i, f in FLOAT_INPUTS.items()}
        ig = _lib.DrinInputGradsC()
        for f, t in outs.items():
            setattr(ig, f, t.data_ptr())
        n = lib.drin_input_grad_scratch_bytes(C.byref(call.cfg))
        scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
        ig.scratch, ig.scratch_bytes = scratch.data_ptr(), n
        g = self.G.contiguous().to(DEV)
        _lib.check(lib.drin_backward_ex(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), g.data_ptr(), None,
                                        C.byref(ig), None, stream()))
        torch.cuda.synchronize()
        return outs


@pytest.mark.parametrize("kind", ["dynamic", "tokens3"])
def test_c_abi_input_gradients_above_65535_mentions(kind):
    """drin_backward_ex's batch-tensor gradients at B2 mentions (the sliced k_span_mean_bwd, k_cosine_bwd_mention and
    k_miei_bwd_mention launches; the token block's backward): every tensor against fp64 autograd through the oracle at the bar of
    tests/test_gpu_input_grads.py (2e-4 of its norm), every element written, and the six mentions past 65 535 by themselves.
    Three mention objects here: with one object on each side the image-image edge is cos * w / (w + 1e-9), w = ms * es, whose
    derivative in either score is cos * 1e-9 * (...) / (w + 1e-9)^2 - nothing but the few of 131 082 pairs with a tiny w, where fp32
    resolves w + 1e-9 to a per cent (measured so: 1.7e-3 of the norm).  entity_object_score keeps that form, so the object scores
    are drawn from [0.25, 1]: its gradient is then below 1e-6 everywhere and test_gpu_input_grads' rule for it applies (ke1: an
    absolute 1e-6)."""
    from tests.test_gpu_input_grads import BAR, FLOAT_INPUTS, check, oracle_grads, rel_err as frob
    case = AbiCase(kind, mention_objects=3)
    counted, outs = launches(case.input_grads)
    ref = oracle_grads(case.cfg, case.sd, case.cpu_batch, case.G)
    worst = 0.0
    for field in FLOAT_INPUTS.values():
        assert torch.isfinite(outs[field]).all(), field
        check(field, outs[field], ref[field], ke1=True)
        check(field, outs[field][SLICE:], ref[field][SLICE:], ke1=True)
        if ref[field].abs().max().item() > 1e-6:
            worst = max(worst, frob(outs[field], ref[field]), frob(outs[field][SLICE:], ref[field][SLICE:]))
    print(f"drin_backward_ex {kind} B={B2}: worst input gradient {worst:.2e} of its norm (bar {BAR:g}), launches {counted}")


@pytest.mark.parametrize("kind", ["dynamic", "static", "vector_static", "tokens3"])
def test_c_abi_forward_and_backward_above_65535_mentions(kind):
    case = AbiCase(kind)
    tag = f"drin_forward/backward {kind} B={B2}"
    small, _ = launches(lambda: case.call(0, 5))
    counted, (scores, grads, status, _ws, _before) = launches(lambda: case.call())
    _lib.check(status)
    assert counted["gcn"] > small["gcn"], (small, counted)            # the sliced per-mention launches
    err = (scores.double().cpu() - case.ref_scores).abs()
    print(f"{tag}: max |score - fp64 oracle| {err.max().item():.2e}, mentions past 65535 {err[SLICE:].max().item():.2e}")
    assert err.max().item() <= ABI_SCORE_TOL
    case.check_grads(grads, tag)
    # the same batch as slices of Model.MAX_CALL_MENTIONS mentions
    from drin_amd.model import Model
    step, parts, summed = Model.MAX_CALL_MENTIONS, [], None
    for lo in range(0, B2, step):
        s, summed, status, _ws, _before = case.call(lo, min(B2, lo + step), grads=summed)
        _lib.check(status)
        parts.append(s)
    gap = (torch.cat(parts) - scores).abs().max().item()
    print(f"{tag}: one call against slices of {step}: scores {gap:.2e}")
    assert gap <= ABI_SLICE_TOL
    for k, one, cut in zip(case.keys, grads, summed):
        rel = (one.double() - cut.double()).norm().item() / (cut.double().norm().item() + 1e-300)
        assert rel <= ABI_GRAD_TOL or not (cut.any() or one.any()), (k, rel)


def test_c_abi_vector_edge_update_backward_is_refused_before_any_launch():
    """Vector edges with a live edge update (dynamic, two layers) above 65 535 mentions: the forward runs and matches the oracle; the
    backward - whose k_edge_pre_vec_bwd_fu is one unsliced (column quads, mention) grid - refuses among its argument checks:
    gradients and workspace keep every bit, nothing was counted as launched."""
    case = AbiCase("vector")
    scores, _grads, _status, _ws, _before = case.call(backward=False)
    err = (scores.double().cpu() - case.ref_scores).abs().max().item()
    print(f"drin_forward vector B={B2}: max |score - fp64 oracle| {err:.2e}")
    assert err <= ABI_SCORE_TOL
    poisoned = [torch.full_like(q, SENTINEL) for q in case.params]
    counted, (scores2, grads, status, ws, before) = launches(lambda: case.call(grads=poisoned))
    assert status == _lib.E_SHAPE and "vector-edge update" in _lib.load().drin_last_error().decode()
    assert torch.equal(ws, before) and all(bool((g == SENTINEL).all()) for g in grads) and torch.equal(bits(scores2), bits(scores))
    small, _ = launches(lambda: case.call(0, 5, backward=False))
    forward_only, _ = launches(lambda: case.call(backward=False))
    assert counted == forward_only and sum(counted.values()) > sum(small.values())   # the refused backward launched nothing
    # below the limit the same configuration trains
    s, g, status, _ws, _before = case.call(0, 4096)
    _lib.check(status)
    assert any(bool(t.any()) for t in g)


# ---- k_attention_bwd_delta past 2^20 workgroups ----------------------------------------------------------------------------------------
def test_attention_backward_delta_past_its_grid_cap():
    """B H Lq = 65535 x 1 x 65 = 4 259 775 rows > 4 x 2^20: waves of k_attention_bwd_delta take a second row.  With one key (Lk = 1)
    and dh = 1 everything has a closed form: p = 1, out = v, delta = out * dout (one fp32 product: exact), dq = dk = 0 up to the
    rounding of p and of dout * v - delta, dv[b] = sum_i dout[b, i]."""
    lib, B, H, Lq, Lk, dh = _lib.load(), SLICE, 1, 65, 1, 1
    rows = B * H * Lq
    assert rows > 4 * (1 << 20)
    gen = torch.Generator(device=DEV).manual_seed(13)
    q, dout = torch.randn(B * Lq, 1, device=DEV, generator=gen), torch.randn(B * Lq, 1, device=DEV, generator=gen)
    k, v = torch.randn(B * Lk, 1, device=DEV, generator=gen), torch.randn(B * Lk, 1, device=DEV, generator=gen)
    out, lse = torch.full((B * Lq, 1), NAN, device=DEV), torch.full((B, H, Lq), NAN, device=DEV)
    dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
    delta = torch.full((B, H, Lq), NAN, device=DEV)
    geo = (B, H, Lq, Lk, dh)
    _lib.check(lib.drin_attention_train_fwd(ptr(q), 1, ptr(k), 1, ptr(v), 1, None, ptr(out), 1, ptr(lse), *geo, stream()))
    _lib.check(lib.drin_attention_bwd(ptr(q), 1, ptr(k), 1, ptr(v), 1, None, ptr(out), 1, ptr(lse), ptr(dout), 1, ptr(dq), 1, ptr(dk), 1, ptr(dv), 1,
                                      ptr(delta), *geo, stream()))
    v_rows = v.view(B, 1).expand(B, Lq).reshape(B * Lq, 1)
    tag = f"attention ({B},{H},{Lq},{Lk},{dh})"
    assert rel_err(out, v_rows, tag + " out") <= KERNEL_TOL
    assert torch.equal(bits(delta.view(-1)), bits((out * dout).view(-1)))          # every row, those of the second trip included
    assert rel_err(delta.view(-1)[4 * (1 << 20):], (v_rows.double() * dout.double()).view(-1)[4 * (1 << 20):], tag + " delta, second trip") <= KERNEL_TOL
    assert rel_err(dv, dout.double().view(B, Lq).sum(1, keepdim=True), tag + " dv") <= KERNEL_TOL
    scale = (dout.abs().max() * v.abs().max() * max(k.abs().max().item(), q.abs().max().item())).item()   # the size of dq's and dk's terms
    assert rel_err(dq, torch.zeros_like(dq), tag + " dq (true value 0)", scale) <= KERNEL_TOL
    assert rel_err(dk, torch.zeros_like(dk), tag + " dk (true value 0)", scale * Lq) <= KERNEL_TOL


# ---- MELHI: k_scale_rows past 65 535 rows ----------------------------------------------------------------------------------------------
def test_melhi_image_mask_past_65535_entity_rows():
    """B N = 6554 x 11 = 72 094 entity-image rows: k_scale_rows' grid.y stops at 65 535 and the rows behind it are strided, forward
    (the mapped entity images) and backward (their gradient).  Against the fp64 restatement at the bars of DESIGN.md section 14."""
    from drin_amd.melhi import Model
    from tests.melhi_inputs import KEYS
    from tests.melhi_restatement import melhi_scores
    from tests.test_gpu_melhi import TOL, big_batch, cfg_for, max_err, sd64
    g = dict(D=8, R=8, L=6, P=2, N=11)
    B = 6554
    assert B * g["N"] > SLICE
    torch.manual_seed(17)
    model = Model(cfg_for(g), precision="f32").to(DEV)
    batch = big_batch(B, g, 23)
    scores = model(batch)
    sd = sd64(model)
    ref, mask = melhi_scores([x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x for x in batch], sd, 0.3, 0.3,
                             return_mask=True)
    kept = mask.reshape(-1).bool()
    assert kept[SLICE // g["N"]:].any() and not kept[SLICE // g["N"]:].all()       # both values of the mask behind row 65 535
    err = max_err(scores, ref)
    print(f"melhi B={B} N={g['N']}: scores max err {err:.2e}; mentions of the rows past 65535: {max_err(scores[SLICE // g['N']:], ref[SLICE // g['N']:]):.2e}")
    assert err < TOL["f32"]
    G = torch.randn(B, g["N"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    (scores * G).sum().backward()
    (ref * G.double()).sum().backward()
    params = dict(model.named_parameters())
    worst = 0.0
    for name in KEYS:
        want = sd[name].grad if sd[name].grad is not None else torch.zeros_like(sd[name])
        scale = want.abs().max().item()
        diff = (params[name].grad.double() - want).abs().max().item()
        assert (diff == 0.0) if scale == 0.0 else (diff / scale < 2e-4), (name, diff, scale)
        worst = max(worst, diff / scale if scale else 0.0)
    print(f"melhi B={B} N={g['N']}: worst gradient tensor {worst:.2e} of its max|ref|")


# ---- k_split_planes_batch past 2048 workgroups --------------------------------------------------------------------------------------
def test_weight_planes_of_a_matrix_past_the_split_grid_cap():
    """The layer-by-layer path splits every weight into bf16 (hi, lo) planes in one batched launch of at most 2048 x 256 float4 per
    matrix: D x R = 1024 x 2080 = 2 129 920 floats is the narrowest admitted image width (a multiple of 32) past it at D = 1024.
    A wrong stride leaves the last rows of W_ei's planes unwritten; scores against the oracle at test_gpu_parity's bar."""
    from drin_amd import synth
    from drin_amd.config import DrinConfig
    from drin_amd.model import Model
    from oracle import drin_oracle as O
    cfg = DrinConfig(bert_embed_dim=1024, gcn_embed_dim=1024, resnet_embed_dim=2080, num_candidates_data=15, max_mention_sentence_len=4,
                     resnet_num_region=1)
    B = 16
    assert 1024 * 2080 > 2048 * 256 * 4 and B * cfg.num_candidates_model >= 256     # pair-sized products: the weights run as planes
    sd = synth.make_state_dict(cfg, 8)
    batch = synth.make_batch(cfg, B, 61)
    ref = O.forward({k: v.double() for k, v in sd.items()}, batch, dtype=torch.float64, **O.config_kwargs(cfg))
    model = Model(cfg, precision="bf16x3", fused=False).to(DEV).eval()
    model.load_state_dict(sd)
    with torch.no_grad():
        counted, got = launches(lambda: model([t.to(DEV) for t in batch[:14]]))
    assert counted.get("stream", 0) == 0 and counted.get("gemm_x3", 0) + counted.get("gemm_planes", 0) > 0, counted
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"weight planes D=1024 R=2080 B={B}: max |score - fp64 oracle| {err:.2e}")
    assert err <= 1e-4
