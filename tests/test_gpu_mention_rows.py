"""-m gpu: k_mention_rows / k_mention_rows_bwd through drin_mention_rows_fwd / _bwd (csrc/mention_rows.hip).
Shapes: L below the kernel's four row groups, L not a multiple of them, D past one 64-lane row of float4s, the reference's width.
Bars: span-mean rows 1e-6 of max|ref| against fp64 (the project's span-mean bar: L <= 130 fp32 additions of O(1) values and one
division, ~1e-7 relative); max rows and positions exact; the backward's fp64 scatter 1e-6 of max|ref| (one division, 6e-8).
Every test prints its measured maxima."""
import ctypes as C

import pytest
import torch

from drin_amd import _lib
from tests.helpers import lowest_argmax, mention_rows_bwd, mention_rows_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 4), (3, 5, 20), (2, 33, 260), (5, 130, 768)]
AVG, MAX = _lib.REPR_AVG_EXTRACT, _lib.REPR_MAX_POOL
TOL = 1e-6
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731


def bits(t):
    return t.contiguous().view(torch.int32)


def planted(B, L, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, L, D, device=DEV, generator=g)
    x[0, L - 1, 0] = float("nan")                  # a NaN wins, at the last position
    x[-1, :, 1] = 2.0                              # a tie over the whole column: position 0
    x[0, :, 2] = -0.0                              # signed zeros: every position ties
    x[0, L // 2, 2] = 0.0
    if L > 2:
        x[-1, :, 3] = -1.0
        x[-1, L - 2:, 3] = 5.0                     # a tie of the last two positions: the lower one
    return x, g


def spans(B, L):
    """Slice forms of Avg.avg: inside, empty, start > end, end past L, negative positions, the whole block."""
    forms = [(0, 1), (2, 2), (4, 1), (1, L + 7), (-3, -1), (0, L), (-2 * L, 2), (L - 1, L)]
    rows = [forms[(b + 7 * L) % len(forms)] for b in range(B)]
    start = torch.tensor([r[0] for r in rows], dtype=torch.int64, device=DEV)
    end = torch.tensor([r[1] for r in rows], dtype=torch.int64, device=DEV)
    clipped = [slice(s, e).indices(L)[:2] for s, e in rows]
    return start, end, clipped


def span_mean_fp64(x, clipped):
    out = torch.empty(x.shape[0], x.shape[2], dtype=torch.float64, device=x.device)
    for b, (s, e) in enumerate(clipped):
        out[b] = x[b, s:e].double().mean(0) if e > s else float("nan")
    return out


def rel(got, ref, tag):
    e = float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))
    print(f"{tag}: max err / max|ref| = {e:.3g}")
    return e


@pytest.mark.parametrize("with_encoded", [False, True])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_mention_rows_forward_max(B, L, D, with_encoded):
    raw, g = planted(B, L, D, 100 + L)
    enc = None
    if with_encoded:
        enc = torch.randn(B, L, D, device=DEV, generator=g)
        enc[0, 0, 0] = float("nan")
        enc[-1, :, 1] = -3.0
    edge, vert, idx = mention_rows_fwd(raw, enc, None, None, MAX)
    for x, row, at, name in ((raw, edge, idx[0], "edge"), (enc if with_encoded else raw, vert, idx[1], "vertex")):
        ref, _ = torch.max(x, dim=1)
        assert torch.equal(row.nan_to_num(7.5), ref.nan_to_num(7.5)), name            # torch.max: NaN wins
        assert torch.equal(torch.isnan(row), torch.isnan(x).any(1)), name
        assert torch.equal(at.long(), lowest_argmax(x)), name
        out, pos = torch.empty(B, D, device=DEV), torch.empty(B, D, dtype=torch.int32, device=DEV)
        _lib.check(_lib.load().drin_seq_max_train_fwd(ptr(x), ptr(out), ptr(pos), B, L, D, stream()))
        assert torch.equal(bits(row), bits(out)) and torch.equal(at, pos), name       # drin_seq_max_train_fwd's bits and positions
    if not with_encoded:
        assert torch.equal(bits(vert), bits(edge)) and torch.equal(idx[0], idx[1])
    assert int(idx[0][0, 0]) == L - 1 and int(idx[0][-1, 1]) == 0
    assert int(idx[0][0, 2]) == 0                                                    # -0.0 == 0.0: a tie, the lowest position
    if L > 2:
        assert int(idx[0][-1, 3]) == L - 2


@pytest.mark.parametrize("with_encoded", [False, True])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_mention_rows_forward_avg(B, L, D, with_encoded):
    raw, g = planted(B, L, D, 200 + L)
    raw = raw.nan_to_num(0.25)
    enc = torch.randn(B, L, D, device=DEV, generator=g) if with_encoded else None
    start, end, clipped = spans(B, L)
    edge, vert, idx = mention_rows_fwd(raw, enc, start, end, AVG)
    assert (idx == -5).all()                                                         # positions belong to the max alone
    empty = torch.tensor([e <= s for s, e in clipped], device=DEV)
    for x, row, name in ((raw, edge, "edge"), (enc if with_encoded else raw, vert, "vertex")):
        ref = span_mean_fp64(x, clipped)
        assert torch.equal(torch.isnan(row), empty[:, None].expand(B, D)), name       # an empty span: a NaN row, as the reference
        if (~empty).any():
            assert rel(row[~empty], ref[~empty], f"mention_rows avg {name} B={B} L={L} D={D}") <= TOL
    if not with_encoded:
        assert torch.equal(bits(vert), bits(edge))


@pytest.mark.parametrize("representation", [AVG, MAX])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_mention_rows_bf16_raw_equals_fp32_kernel_on_widened_values(B, L, D, representation):
    raw, g = planted(B, L, D, 300 + L)
    raw16 = raw.to(torch.bfloat16)
    enc = torch.randn(B, L, D, device=DEV, generator=g)
    start, end, _ = spans(B, L)
    for e in (None, enc):
        a = mention_rows_fwd(raw16, e, start, end, representation)
        b = mention_rows_fwd(raw16.float(), e, start, end, representation)
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)


def scatter_fp64(g, shape, representation, clipped, at):
    B, L, D = shape
    out = torch.zeros(shape, dtype=torch.float64, device=DEV)
    if g is None:
        return out
    if representation == MAX:
        return out.scatter_(1, at[:, None, :].long(), g.double()[:, None, :])
    for b, (s, e) in enumerate(clipped):
        if e > s:
            out[b, s:e] = g[b].double() / (e - s)
    return out


@pytest.mark.parametrize("representation", [AVG, MAX])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_mention_rows_backward(B, L, D, representation):
    shape = (B, L, D)
    raw, g = planted(B, L, D, 400 + L)
    enc = torch.randn(B, L, D, device=DEV, generator=g)
    start, end, clipped = spans(B, L)
    ge, gv = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, D, device=DEV, generator=g)
    tag = f"mention_rows_bwd repr={representation} B={B} L={L} D={D}"
    # an encoded block: the edge row's term to the raw block, the vertex row's to the encoded one
    _, _, idx = mention_rows_fwd(raw, enc, start, end, representation)
    d_raw, d_enc = mention_rows_bwd(ge, gv, start, end, idx, representation, 1, shape)
    assert not torch.isnan(d_raw).any() and not torch.isnan(d_enc).any()            # every element written
    ref_raw, ref_enc = (scatter_fp64(x, shape, representation, clipped, at) for x, at in ((ge, idx[0]), (gv, idx[1])))
    assert rel(d_raw, ref_raw, tag + " d_raw") <= TOL and rel(d_enc, ref_enc, tag + " d_enc") <= TOL
    assert torch.equal(d_raw != 0, ref_raw != 0) and torch.equal(d_enc != 0, ref_enc != 0)   # exactly 0 elsewhere
    again = mention_rows_bwd(ge, gv, start, end, idx, representation, 1, shape)
    assert torch.equal(bits(again[0]), bits(d_raw)) and torch.equal(bits(again[1]), bits(d_enc))   # two runs: the same bits
    # NULL destinations, NULL rows
    only_enc = mention_rows_bwd(ge, gv, start, end, idx, representation, 1, shape, want_raw=False)
    only_raw = mention_rows_bwd(ge, gv, start, end, idx, representation, 1, shape, want_enc=False)
    assert only_enc[0] is None and torch.equal(bits(only_enc[1]), bits(d_enc))
    assert only_raw[1] is None and torch.equal(bits(only_raw[0]), bits(d_raw))
    assert mention_rows_bwd(ge, gv, start, end, idx, representation, 1, shape, want_raw=False, want_enc=False) == (None, None)
    no_edge = mention_rows_bwd(None, gv, start, end, idx, representation, 1, shape)
    assert not no_edge[0].any() and torch.equal(bits(no_edge[1]), bits(d_enc))      # no gradient through the edge row: zeros
    # no encoded block: both terms land in the raw block in one write = the sum of the two single forms, to fp32 rounding
    _, _, idx1 = mention_rows_fwd(raw, None, start, end, representation)
    both, none = mention_rows_bwd(ge, gv, start, end, idx1, representation, 0, shape, want_enc=False)
    e_only, _ = mention_rows_bwd(ge, None, start, end, idx1, representation, 0, shape, want_enc=False)
    v_only, _ = mention_rows_bwd(None, gv, start, end, idx1, representation, 0, shape, want_enc=False)
    assert none is None and not torch.isnan(both).any()
    two = e_only.double() + v_only.double()
    err = float((both.double() - two).abs().max() / two.abs().max().clamp_min(1e-30))
    print(f"{tag} both-in-one vs sum of the single forms: {err:.3g}")
    assert err <= 2.0 ** -23
    assert rel(both, scatter_fp64(ge, shape, representation, clipped, idx1[0]) + scatter_fp64(gv, shape, representation, clipped, idx1[1]),
               tag + " both") <= TOL


def test_mention_rows_count_as_pool_one_launch_each():
    raw, enc = torch.randn(3, 9, 20, device=DEV), torch.randn(3, 9, 20, device=DEV)
    ge = torch.randn(3, 20, device=DEV)
    _lib.profile_begin()
    _, _, idx = mention_rows_fwd(raw, enc, None, None, MAX)
    mention_rows_bwd(ge, ge, None, None, idx, MAX, 1, (3, 9, 20))
    torch.cuda.synchronize()
    classes = _lib.profile_end()
    assert classes["pool"][1] == 2 and sum(n for _ms, n in classes.values()) == 2


def test_mention_rows_at_the_reference_shape_profile_record():
    """B = 64, L = 128, D = 768 (25 MB read forward): what drin_profile_* reports, printed for the record - no rate is promised."""
    B, L, D = 64, 128, 768
    raw, enc = torch.randn(B, L, D, device=DEV), torch.randn(B, L, D, device=DEV)
    ge = torch.randn(B, D, device=DEV)
    for representation, name in ((AVG, "avg"), (MAX, "max")):
        start = torch.full((B,), 3, dtype=torch.int64, device=DEV)
        end = torch.full((B,), 9, dtype=torch.int64, device=DEV)
        mention_rows_fwd(raw, enc, start, end, representation)                       # warm
        _lib.profile_begin()
        _, _, idx = mention_rows_fwd(raw, enc, start, end, representation)
        torch.cuda.synchronize()
        fwd = _lib.profile_end()["pool"]
        _lib.profile_begin()
        mention_rows_bwd(ge, ge, start, end, idx, representation, 1, (B, L, D))
        torch.cuda.synchronize()
        bwd = _lib.profile_end()["pool"]
        print(f"k_mention_rows {name} B={B} L={L} D={D}: forward {fwd[0] * 1e3:.1f} us ({fwd[1]} launch), backward {bwd[0] * 1e3:.1f} us ({bwd[1]} launch)")
        assert fwd[1] == 1 and bwd[1] == 1
