"""-m gpu: the max form of the WikiMEL entity token pool alone, through its C entry points:
`drin_entity_token_pool` against `torch.max` over the slice bit for bit (a maximum rounds nothing), planted NaN / inf values,
DRIN_POOL_AVG against `drin_entity_token_mean`, the indexed form against the plain form on the clamped gather, and
`drin_ghmfc_entity_rows_ex` with and without the entity Linear.  Outputs are filled with NaN (or 7) first."""
import ctypes as C

import pytest
import torch

from drin_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
TOL = {"bf16x3": 1e-4, "f32": 1e-5}                                      # the project's bars for a product against fp64
PRECISION = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
GRID = [(T, D) for T in (9, 10, 11, 20) for D in (4, 260, 768, 1024)]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal bit for bit, NaN compared as NaN"""
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.nan_to_num(nan=0.0).contiguous().view(torch.int32), b.nan_to_num(nan=0.0).contiguous().view(torch.int32))


def slice_of(mask_row: torch.Tensor, T: int) -> slice:
    """tokens 1 : ntok - 1 with Python's rules (ntok == 0: the stop -1 counts from the end)"""
    return slice(1, int(mask_row.sum()) - 1)


def max_reference(feat: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """torch.max over each pair's slice on the CPU in fp32; an empty slice (where torch raises) is a NaN row"""
    out = torch.full((feat.shape[0], feat.shape[2]), NAN)
    for p in range(feat.shape[0]):
        rows = feat[p, slice_of(mask[p], feat.shape[1])]
        if rows.shape[0]:
            out[p] = rows.max(0)[0]
    return out


_CASES = {}


def grid_case(T: int, D: int):
    """(feat, mask, expected) on the host, pair p has ntok = p: computed once and shared"""
    if (T, D) not in _CASES:
        pairs = T + 1
        g = torch.Generator().manual_seed(100 * T + D)
        feat = torch.randn(pairs, T, D, generator=g)
        assert (feat != 0).all()                                        # no zeros: the order of +0 / -0 ties does not arise
        mask = (torch.arange(T)[None, :] < torch.arange(pairs)[:, None]).to(torch.int64)
        _CASES[(T, D)] = (feat, mask, max_reference(feat, mask))
    return _CASES[(T, D)]


def pool(feat_d, mask_d, pooling, fill=NAN):
    pairs, T, D = feat_d.shape
    out = torch.full((pairs, D), fill, device=DEV)
    _lib.check(_lib.load().drin_entity_token_pool(ptr(feat_d), ptr(mask_d), ptr(out), pairs, T, D, pooling, stream()))
    return out


@pytest.mark.parametrize("T,D", GRID)
def test_max_pool_is_torch_max_over_the_slice_bit_for_bit(T, D):
    """One pair per ntok = 0 ... T: the 8-row unrolled trip runs from ntok = 10 on, with every remainder behind it up to T = 20;
    D = 1024 is 256 float4 columns on a 192-thread block, a second trip of the column loop."""
    feat, mask, want = grid_case(T, D)
    got = pool(feat.to(DEV), mask.to(DEV), _lib.POOL_MAX).cpu()
    empty = torch.isnan(got).all(1)
    assert empty.tolist() == [p in (1, 2) for p in range(T + 1)] and int(empty.sum()) == 2      # 2 of T + 1 pairs, no more
    assert not torch.isnan(got[~empty]).any()
    assert same_bits(got, want)


def test_planted_nan_and_inf_follow_torch_max():
    T, D, pairs = 12, 260, 6
    g = torch.Generator().manual_seed(7)
    feat = torch.randn(pairs, T, D, generator=g)
    ntok = torch.tensor([12, 7, 7, 9, 5, 6])
    mask = (torch.arange(T)[None, :] < ntok[:, None]).to(torch.int64)
    mask[5] = torch.tensor([1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0])        # not a prefix: only its sum (6) counts
    feat[0, 4, 17] = NAN                                                # inside 1 : 11: that column is NaN
    feat[0, 10, 18] = NAN                                               # the last row of the slice
    feat[1, 0, :] = NAN                                                 # row 0 is never read
    feat[1, 6:, :] = NAN                                                # rows >= ntok - 1 are never read
    feat[2, 3, 5], feat[2, 2, 6] = INF, -INF
    feat[3, 1:8, 9] = -INF                                              # a whole column of -inf
    feat[4, 1, 3], feat[4, 2, 3] = NAN, INF                             # NaN beats +inf, in either order
    feat[4, 1, 4], feat[4, 2, 4] = INF, NAN
    feat[5, 5:, :] = NAN                                                # outside 1 : 5
    want = max_reference(feat, mask)
    got = pool(feat.to(DEV), mask.to(DEV), _lib.POOL_MAX).cpu()
    assert same_bits(got, want)
    assert torch.isnan(got[0, 17]) and torch.isnan(got[0, 18]) and int(torch.isnan(got[0]).sum()) == 2
    assert not torch.isnan(got[1]).any() and not torch.isnan(got[5]).any()
    assert got[2, 5] == INF and got[3, 9] == -INF and got[2, 6] == want[2, 6] and torch.isfinite(got[2, 6])
    assert torch.isnan(got[4, 3]) and torch.isnan(got[4, 4]) and int(torch.isnan(got[4]).sum()) == 2


@pytest.mark.parametrize("T,D", [(9, 4), (11, 260), (20, 768), (20, 1024)])
def test_avg_through_the_pool_entry_is_the_token_mean(T, D):
    feat, mask, _ = grid_case(T, D)
    feat_d, mask_d = feat.to(DEV), mask.to(DEV)
    want = torch.full((T + 1, D), NAN, device=DEV)
    _lib.check(_lib.load().drin_entity_token_mean(ptr(feat_d), ptr(mask_d), ptr(want), T + 1, T, D, stream()))
    assert same_bits(pool(feat_d, mask_d, _lib.POOL_AVG), want)


@pytest.mark.parametrize("pooling", [_lib.POOL_MAX, _lib.POOL_AVG])
@pytest.mark.parametrize("T,D", [(9, 4), (11, 260), (20, 768), (20, 1024)])
def test_indexed_pool_has_the_bits_of_the_plain_form_on_the_clamped_gather(T, D, pooling):
    """The table is the E = T + 1 rows of the grid; the index repeats rows and holds one -1 and one E: clamped before any address
    is formed (rows 0 and E - 1 are what is read) and reported."""
    lib = _lib.load()
    feat, mask, _ = grid_case(T, D)
    E, pairs = T + 1, 3 * T + 2
    index = torch.randint(0, E, (pairs,), generator=torch.Generator().manual_seed(T * D))
    index[:E] = torch.arange(E).flip(0)                                 # every token count is met
    index[E + 1], index[E + 3] = -1, E
    text, m, i = feat.to(DEV), mask.to(DEV), index.to(DEV)
    words = torch.zeros(4, dtype=torch.int32, device=DEV)
    got = torch.full((pairs, D), 7.0, device=DEV)
    _lib.check(lib.drin_entity_token_pool_indexed(ptr(text), ptr(m), ptr(i), E, ptr(got), pairs, T, D, pooling, ptr(words), stream()))
    clamped = i.clamp(0, E - 1)
    want = pool(text[clamped].contiguous(), m[clamped].contiguous(), pooling, fill=7.0)
    assert same_bits(got, want)
    assert words.tolist() in ([1, E + 1, -1, -1], [1, E + 3, E, 0])     # {1, the first reporter's position, value low, high}
    if pooling == _lib.POOL_AVG:
        words.zero_()
        mean = torch.full((pairs, D), 7.0, device=DEV)
        _lib.check(lib.drin_entity_token_mean_indexed(ptr(text), ptr(m), ptr(i), E, ptr(mean), pairs, T, D, ptr(words), stream()))
        assert same_bits(got, mean)


def entity_rows_ex(text, mask, pooling, w, b, precision):
    lib = _lib.load()
    E, T, D = text.shape
    nbytes = lib.drin_ghmfc_entity_rows_workspace_bytes(E, T, D)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rows = torch.full((E, D), 7.0, device=DEV)
    _lib.check(lib.drin_ghmfc_entity_rows_ex(ptr(text), ptr(mask), E, T, D, pooling, ptr(w), ptr(b), PRECISION[precision], ptr(rows),
                                             ptr(ws), nbytes, stream()))
    return rows


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_entity_rows_ex(precision):
    """E = 300 entities (past the 256-row gate of the product) with 0, 3 ... T tokens each."""
    lib = _lib.load()
    E, T, D = 300, 11, 260
    g = torch.Generator().manual_seed(11)
    feat = torch.randn(E, T, D, generator=g)
    ntok = torch.tensor([(0, 3, 4, 5, 6, 7, 8, 9, 10, 11)[e % 10] for e in range(E)])
    mask = (torch.arange(T)[None, :] < ntok[:, None]).to(torch.int64)
    w, b = torch.randn(D, D, generator=g) / D ** 0.5, torch.randn(D, generator=g)
    text, m, wd, bd = feat.to(DEV), mask.to(DEV), w.to(DEV), b.to(DEV)
    # AVG with weights: drin_ghmfc_entity_rows' bits
    nbytes = lib.drin_ghmfc_entity_rows_workspace_bytes(E, T, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    want = torch.full((E, D), 7.0, device=DEV)
    _lib.check(lib.drin_ghmfc_entity_rows(ptr(text), ptr(m), E, T, D, ptr(wd), ptr(bd), PRECISION[precision], ptr(want), ptr(ws), nbytes,
                                          stream()))
    assert same_bits(entity_rows_ex(text, m, _lib.POOL_AVG, wd, bd, precision), want)
    # MAX without weights (final_layer = Identity): the plain max pool, straight into rows
    pooled = pool(text, m, _lib.POOL_MAX)
    assert same_bits(entity_rows_ex(text, m, _lib.POOL_MAX, None, None, precision), pooled)
    assert same_bits(pooled.cpu(), max_reference(feat, mask)) and not torch.isnan(pooled).any()
    # MAX with weights against fp64
    ref = max_reference(feat, mask).double() @ w.double().T + b.double()
    got = entity_rows_ex(text, m, _lib.POOL_MAX, wd, bd, precision).double().cpu()
    err = (got - ref).abs().max().item()
    print(f"entity rows max + linear {precision}: max err {err:.3e} (max |ref| {ref.abs().max().item():.3e})")
    assert err <= TOL[precision] * ref.abs().max().item()
    # exactly one weight pointer: refused before any launch
    assert lib.drin_ghmfc_entity_rows_ex(ptr(text), ptr(m), E, T, D, _lib.POOL_MAX, ptr(wd), None, PRECISION[precision], ptr(want),
                                         ptr(ws), nbytes, stream()) == _lib.E_NULL
