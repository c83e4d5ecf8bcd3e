"""Every backward GEMM form - dW (+)= dY^T X, db (+)= column sums of dY, dX (+)= dY W - against fp64, through `drin_wgrad_probe`.

A case is a list of products handed to ONE launcher of the GEMM module (or to a whole `WeightGradPass`).  The test first asserts
the ROUTE RECORD that the dispatch code wrote next to its launches - kernel, slices, rows per slice, in place or stored, whether
the bias gradient rode in the split-bf16 kernel, the grid of every GEMM launch, the slice sum's destinations and segments - never
a restatement of a gate: a gate that moves turns the case red with "move the shape".  Then every destination is compared with the
fp64 result of the same operands on the CPU.

Contracts of every case: each dW sits in a [n_out + 1][k + 4] buffer and each db in a [n_out + 4] one, holding a random dw0 / db0
(every form accumulates) with NaN in the pad columns and the spare row; no pad and no float of the guard band behind the scratch
changes.  Strided operands carry NaN in their pad columns.  Indexed rows go through a permutation with repeats into a larger
table whose unnamed rows are NaN.

Input families (the reduction now running over the ROWS of both operands):
  a  randn (x / sqrt(rows))
  b  same-sign operands with exact planes in dy AND x: v = h + l, h a bf16 in [1, 2), l = 2^-9 (a bf16 in [0.5, 1))
  c  family a with column n of dy multiplied by 2^e[n] and column k of x by 2^f[k], e, f in [-20, 20]; dw0[n, k] and db0[n] scaled alike
  d  family a with dy drawn as bf16 values

Bars, per element (none tuned on a kernel; `test_emulation_stays_inside_the_bars_and_mutants_do_not` holds a torch emulation of
the recorded algorithm inside each of them on the CPU, and prints the fraction of the bar it uses):
  split-bf16 dW, families a, c, d   2e-5 sum|dy||x|
  split-bf16 dW, family b           sum|dy_lo||x_lo| + 4 err32 + 1e-6, err32 = the largest error of torch's CPU fp32 evaluation
  exact-fp32 dW and dX              5e-6 sum|dy||x|
  db, riding or through the batch   5e-6 sum|dy|
  a reduction of ONE row (dw and db), and no other shape: + 2^-24 (|dw0| + sum|dy||x|) (2^-24 (|db0| + sum|dy|) for db), half an
    ulp of the one fp32 addition that lands the product on dw0.  There the "sum" is a single product p, fl(dw0 + p) is off by
    up to 2^-24 |dw0 + p| whatever computes it, and 5e-6 |p| is below that wherever |p| < 0.012 |dw0|: a bar relative to
    sum|dy||x| alone cannot be met by any fp32 result.  `test_a_one_row_reduction_needs_the_rounding_of_its_landing` shows the
    emulation outside the plain bar there; at every other shape the emulation is held inside the plain bar.
  a destination that takes several products (two segments): the sum of its products' bars.

Measured maxima: DESIGN.md section 19.
"""
import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Optional

import pytest
import torch

from drin_amd import _lib

DEV = "cuda"
BF16X3_BAR, F32_BAR, DB_BAR, HALF_ULP = 2e-5, 5e-6, 5e-6, 2.0 ** -24
GUARD = 1024               # floats behind the scratch that nothing may touch
NAN = float("nan")
BIG = 1 << 23              # "a large scratch": more than any split of the direct cases needs (the largest stores 5.6 M floats)
PASS_SCRATCH = 28 << 20    # the three parts of a WeightGradPass (its split-bf16 part alone is a round of 256 x 256 tiles)
X3, FS, FL = "tn_bf16x3", "tn_f32_small", "tn_f32_large"
COEF = {X3: BF16X3_BAR, FS: F32_BAR, FL: F32_BAR}


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class P:
    """one product and what the dispatch code is expected to record for it"""
    shape: tuple                 # (rows, n_out, k)
    kernel: Optional[str]        # X3 | FS | FL | None (column sums only)
    slices: int = 0
    rows_per_slice: int = 0
    in_place: int = 0
    launch: int = 0              # which GEMM launch of the call carries it
    db: str = ""                 # "" | "rides" | "batch"
    db_slices: int = 0           # "batch": the column-sum kernel's row slices
    strided: str = ""            # "dy", "x", "dyx": lddy = n_out + 8, ldx = k + 16
    indexed: bool = False
    dst: int = -1                # >= 0: adds to the dw of that product of the case


@dataclass(frozen=True)
class Case:
    name: str
    form: str
    op: int
    products: tuple
    call: dict                   # expected per-call record
    scratch: Optional[int] = BIG
    precision: int = _lib.PREC_BF16X3
    families: tuple = ("a", "b", "c")
    staged: bool = False
    layers_done_after: int = -1
    reduce: bool = False         # the slices land through launch_gemm_tn's split-K reduction, not the slice sum


def call(gemm=1, grid=(), sums=1, dsts=0, segs=0, colsum=0, reduce=0):
    return dict(gemm_launches=gemm, grid=tuple(grid), sum_launches=sums, sum_dsts=dsts, sum_segs=segs, colsum_launches=colsum,
                reduce_launches=reduce)


G, FG, TN, CS, PASS = _lib.WGRAD_TN_GROUP, _lib.WGRAD_TN_F32_GROUP, _lib.WGRAD_TN, _lib.WGRAD_COLSUM_BATCH, _lib.WGRAD_PASS
ABCD = ("a", "b", "c", "d")
# the eight pair-sized shapes of the group cases: every M of {1024, 1055, 2080}, every N and K of {128, 132, 260, 516}
POOL = ((1024, 128, 128), (1055, 132, 260), (2080, 260, 516), (1055, 516, 132), (2080, 128, 260), (1024, 516, 516), (1055, 260, 260),
        (2080, 132, 128))
POOL_OPTS = (dict(db="rides"), dict(strided="dyx"), dict(db="rides"), dict(indexed=True), dict(db="rides", strided="x"), dict(),
             dict(db="rides", strided="dy"), dict())


def pool(n, slices, with_db=True, first=0):
    out = []
    for i, (s, rps) in enumerate(slices):
        opts = dict(POOL_OPTS[first + i])
        if not with_db:
            opts.pop("db", None)
        out.append(P(POOL[first + i], X3, s, rps, **opts))
    assert len(out) == n
    return tuple(out)


def dsts_of(products):
    return len({(p.dst if p.dst >= 0 else i) for i, p in enumerate(products)}) + sum(1 for p in products if p.db == "rides")


def group(name, form, products, grid, scratch=BIG, families=("a", "b", "c")):
    return Case(name, form, G, products, call(1, (grid,), 1, dsts_of(products), len(products) + sum(1 for p in products if p.db == "rides")),
                scratch=scratch, families=families)


PASS16 = (
    # (slice sums - plain: the instalment's 8 dW + 4 riding db, then 3 column sums + 2 stored mention-sized dW + 3 dW + 3 db;
    #  staged: 12, then 3 + 2 + 1 + 1 for the layers, then 2 + 2 for the encoders)
    # layer 0 (k = 128): dW_h takes the mention rows (mention-sized, exact fp32) and the entity rows (split-bf16) on ONE destination
    P((40, 132, 128), FS, 1, 64, 1, launch=1), P((1055, 132, 128), X3, 9, 128, dst=0), P((2080, 132, 128), X3, 17, 128, db="rides"),
    P((96, 132, 128), FS, 1, 96, 1, launch=1, db="batch", db_slices=2), P((1024, 132, 128), X3, 8, 128, db="rides"),
    # layer 1 (k = 260); its last product has lddy != n_out: the bias gradient must NOT ride
    P((129, 132, 260), FS, 2, 96, 0, launch=1), P((1055, 132, 260), X3, 9, 128, dst=5, strided="x"), P((2080, 132, 260), X3, 17, 128, db="rides"),
    P((96, 132, 260), FS, 1, 96, 1, launch=1, db="batch", db_slices=2), P((1024, 132, 260), X3, 8, 128, db="batch", db_slices=16, strided="dy"),
    # layer 2 (k = 132): the ninth split-bf16 product sends the first eight off as an instalment
    P((300, 132, 132), FS, 3, 128, 0, launch=1), P((1055, 132, 132), X3, 9, 128, dst=10), P((2080, 132, 132), X3, 17, 128, db="rides"),
    P((1024, 132, 132), X3, 8, 128, launch=2, db="rides"),
    # the two entity encoders of table-form training: indexed rows
    P((1055, 132, 260), X3, 9, 128, launch=2, db="rides", indexed=True), P((1055, 132, 516), X3, 9, 128, launch=2, db="rides", indexed=True),
)
PASS16_STAGED = tuple(P(**{**p.__dict__, "launch": 3}) if i >= 14 else p for i, p in enumerate(PASS16))
SMALL9 = tuple(P(s, FS, sl, rps, ip, launch=0 if i < 8 else 1, strided=("dy" if i == 3 else "x" if i == 4 else ""))
               for i, (s, (sl, rps, ip)) in enumerate(zip(
                   ((1, 68, 100), (127, 100, 68), (129, 68, 68), (300, 100, 100), (512, 68, 100), (96, 100, 68), (40, 68, 68), (2048, 68, 100),
                    (129, 100, 100)),
                   ((1, 32, 1), (1, 128, 1), (2, 96, 0), (3, 128, 0), (4, 128, 0), (1, 96, 1), (1, 64, 1), (4, 512, 0), (2, 96, 0)))))
# eight pair-sized products heavy enough to lift the slice length off its 128-row floor: the plain pass deals the chip over all
# eight (544-row slices), the staged one over each half (288 and 192), so the two differ by their summation split
SPLIT8_SHAPES = ((2080, 516, 516), (2080, 516, 260), (2080, 260, 516), (2080, 516, 516), (1055, 516, 516), (2080, 260, 260), (2080, 516, 516),
                 (1024, 516, 516))
SPLIT8 = tuple(P(s, X3, sl, rps, db="rides") for s, (sl, rps) in zip(
    SPLIT8_SHAPES, ((4, 544), (4, 544), (4, 544), (4, 544), (2, 544), (4, 544), (4, 544), (2, 512))))
SPLIT8_STAGED = tuple(P(s, X3, sl, rps, launch=int(i >= 4), db="rides") for i, (s, (sl, rps)) in enumerate(zip(
    SPLIT8_SHAPES, ((8, 288), (8, 288), (8, 288), (8, 288), (6, 192), (11, 192), (11, 192), (6, 192)))))

CASES = [
    # launch_gemm_tn in a split-bf16 precision with scratch: the split-bf16 kernel, one product
    Case("tn_x3_1024_128_128", "tn_bf16x3 alone", TN, (P((1024, 128, 128), X3, 8, 128),), call(1, (8,), 1, 1, 1), families=ABCD),
    Case("tn_x3_1055_132_260", "tn_bf16x3 alone", TN, (P((1055, 132, 260), X3, 9, 128, strided="dyx"),), call(1, (18,), 1, 1, 1), families=ABCD),
    Case("tn_x3_2080_260_516", "tn_bf16x3 alone", TN, (P((2080, 260, 516), X3, 17, 128),), call(1, (102,), 1, 1, 1), families=ABCD),
    Case("tn_x3_1055_516_132", "tn_bf16x3 alone", TN, (P((1055, 516, 132), X3, 9, 128, strided="dy"),), call(1, (27,), 1, 1, 1), families=ABCD),
    Case("tn_x3_2080_516_516", "tn_bf16x3 alone", TN, (P((2080, 516, 516), X3, 17, 128),), call(1, (153,), 1, 1, 1), families=ABCD),
    Case("tn_x3_1024_260_132", "tn_bf16x3 alone", TN, (P((1024, 260, 132), X3, 8, 128, strided="x"),), call(1, (16,), 1, 1, 1), families=ABCD),
    # launch_gemm_tn_group
    group("group_lone_indexed_db", "tn_bf16x3 group, indexed rows, bias gradient riding",
          (P((1055, 260, 260), X3, 9, 128, db="rides", indexed=True),), 36),
    group("group2", "tn_bf16x3 group of 2", pool(2, ((9, 128), (17, 128)), with_db=False, first=1), 120, families=ABCD),
    group("group2_cut", "tn_bf16x3 group of 2, scratch cut", pool(2, ((5, 224), (10, 224)), with_db=False, first=1), 70, scratch=1553760),
    group("group5_db", "tn_bf16x3 group of 5 with bias gradients", pool(5, ((8, 128), (9, 128), (17, 128), (9, 128), (17, 128))), 189),
    group("group5_db_cut", "tn_bf16x3 group of 5 with bias gradients, scratch cut", pool(5, ((3, 352), (3, 352), (6, 352), (3, 352), (6, 352))),
          66, scratch=1562824),
    group("group8_db", "tn_bf16x3 group of 8", pool(8, ((7, 160), (7, 160), (13, 160), (7, 160), (13, 160), (7, 160), (7, 160), (13, 160))), 250),
    group("group8_db_cut", "tn_bf16x3 group of 8, scratch cut",
          pool(8, ((4, 256), (4, 288), (8, 288), (4, 288), (8, 288), (4, 256), (4, 288), (8, 288))), 148, scratch=3343696),
    group("group_shared_dw", "tn_bf16x3 group, two products on one destination",
          (P((1055, 132, 260), X3, 9, 128), P((1024, 132, 260), X3, 8, 128, dst=0, strided="dy"), P((1024, 128, 128), X3, 8, 128)), 42),
    # launch_gemm_tn_f32_group
    Case("f32_lone_in_place", "tn_f32_small group, one slice in place", FG, (P((127, 68, 100), FS, 1, 128, 1),), call(1, (4,), 0, 0, 0)),
    Case("f32_shared_dw", "tn_f32_small group, two products on one destination", FG,
         (P((127, 68, 100), FS, 1, 128, 0), P((129, 68, 100), FS, 2, 96, 0, dst=0, strided="dyx")), call(1, (12,), 1, 1, 2)),
    Case("f32_group8", "tn_f32_small group of 8", FG,
         (P((1, 4, 4), FS, 1, 32, 1), P((127, 68, 100), FS, 1, 128, 1, strided="dy"), P((129, 100, 68), FS, 2, 96, 0), P((512, 192, 4), FS, 4, 128, 0),
          P((2048, 4, 192), FS, 4, 512, 0, strided="x"), P((2048, 192, 192), FS, 4, 512, 0), P((512, 68, 68), FS, 4, 128, 0, strided="dyx"),
          P((129, 4, 100), FS, 2, 96, 0)), call(1, (93,), 1, 6, 6)),
    # launch_gemm_tn on the large exact kernel (2049 reduction rows: one past the mention-sized limit)
    Case("tn_f32_large_scratch", "tn_f32_large, 17 slices", TN, (P((2049, 132, 132), FL, 17, 128, 0),), call(1, (68,), 0, 0, 0, reduce=1),
         precision=_lib.PREC_F32, reduce=True),
    Case("tn_f32_large_two_slices", "tn_f32_large, scratch for 2 slices", TN, (P((2049, 132, 132), FL, 2, 1056, 0, strided="dyx"),),
         call(1, (8,), 0, 0, 0, reduce=1), scratch=2 * 132 * 132, precision=_lib.PREC_F32, reduce=True),
    Case("tn_f32_large_in_place", "tn_f32_large, no scratch", TN, (P((2049, 132, 132), FL, 1, 2049, 1),), call(1, (4,), 0, 0, 0),
         scratch=None, precision=_lib.PREC_F32),
    # launch_colsum_batch: rows {1, 255, 257, 5000} x C {4, 260, 768}, the scratch exactly what the eight sums store
    Case("colsum8", "column-sum batch of 8", CS,
         (P((1, 4, 4), None, db="batch", db_slices=1), P((255, 260, 4), None, db="batch", db_slices=4),
          P((257, 768, 4), None, db="batch", db_slices=5, strided="dy"), P((5000, 4, 4), None, db="batch", db_slices=64),
          P((5000, 260, 4), None, db="batch", db_slices=64), P((1, 768, 4), None, db="batch", db_slices=1),
          P((257, 4, 4), None, db="batch", db_slices=5, strided="dy"), P((255, 768, 4), None, db="batch", db_slices=4)),
         call(0, (), 1, 8, 8, colsum=1), scratch=25640),
    # WeightGradPass
    Case("pass16", "pass: instalment of 8, mixed destinations, plain", PASS, PASS16, call(3, (128, 84, 53), 2, 12 + 11, 12 + 11, colsum=1),
         scratch=PASS_SCRATCH, layers_done_after=13),
    Case("pass16_staged", "pass: instalment of 8, mixed destinations, staged", PASS, PASS16_STAGED,
         call(4, (128, 84, 8, 45), 3, 12 + 7 + 4, 12 + 7 + 4, colsum=1), scratch=PASS_SCRATCH, staged=True, layers_done_after=13),
    Case("pass_split8", "pass: eight heavy products, plain", PASS, SPLIT8, call(1, (208,), 1, 16, 16), scratch=PASS_SCRATCH, layers_done_after=3),
    Case("pass_split8_staged", "pass: eight heavy products, staged parts with their own slice lengths", PASS, SPLIT8_STAGED,
         call(2, (240, 251), 2, 16, 16), scratch=PASS_SCRATCH, staged=True, layers_done_after=3),
    Case("pass_strided_dy", "pass: lddy != n_out keeps the bias gradient off the split-bf16 kernel", PASS,
         (P((1055, 132, 260), X3, 9, 128, db="batch", db_slices=17, strided="dy"), P((1024, 132, 128), X3, 8, 128, db="rides")),
         call(1, (26,), 1, 4, 4, colsum=1), scratch=PASS_SCRATCH),
    Case("pass_small_instalment", "pass: instalment of the exact-fp32 group", PASS,
         (P((1024, 128, 128), X3, 8, 128, launch=2, db="rides"),) + SMALL9, call(3, (68, 8, 8), 2, 4 + 1 + 2, 4 + 1 + 2), scratch=PASS_SCRATCH),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, f) for c in CASES for f in c.families]
# the forms the backward pass has: each must be named by the route record of at least one case
FORMS_WANTED = ("group of 2", "group of 5", "group of 8", "scratch cut", "bias gradient riding", "indexed rows", "two products on one destination",
                "tn_f32_small group", "one slice in place", "tn_f32_large", "column-sum batch", "pass: instalment of 8", "staged",
                "lddy != n_out", "instalment of the exact-fp32 group")


# ---- operands and references (CPU, computed once per product and shared: never written to) ---------------------------------------
def split_planes(v):
    hi = v.bfloat16()
    return hi.float(), (v - hi.float()).bfloat16().float()


def exact_plane_values(shape, gen):
    h = 1 + torch.randint(0, 128, shape, generator=gen).float() / 128            # bf16 in [1, 2)
    l = 2.0 ** -9 * (0.5 + torch.randint(0, 128, shape, generator=gen).float() / 256)   # 2^-9 x (bf16 in [0.5, 1))
    return h + l, h, l


@dataclass
class Operands:
    dy: torch.Tensor
    x: torch.Tensor            # the EFFECTIVE rows (an indexed product: row m is the table row its index names)
    dw0: torch.Tensor
    db0: torch.Tensor
    with_gemm: bool
    cache: dict = field(default_factory=dict)

    def get(self, name):
        if name not in self.cache:
            dy, x = self.dy, self.x
            self.cache[name] = {
                "ref": lambda: dy.double().t() @ x.double(), "scale": lambda: (dy.abs().t() @ x.abs()).double(),
                "prod32": lambda: dy.t() @ x, "colref": lambda: dy.double().sum(0), "colscale": lambda: dy.abs().double().sum(0),
                "lolo": lambda: split_planes(dy)[1].double().t() @ split_planes(x)[1].double()}[name]()
        return self.cache[name]


@functools.lru_cache(maxsize=48)
def operands(shape, family, salt, repeats, with_gemm=True):
    """Family c: element (n, k) of the product lives at 2^(e[n] + f[k]), so dw0 is scaled by that and db0[n] by 2^e[n]: an fp32 sum
    with a term 2^40 times larger than sum|dy||x| could not meet a bar relative to sum|dy||x|, whatever the kernel."""
    M, N, K = shape
    gen = torch.Generator().manual_seed(M * 31 + N * 7 + K + ord(family) + 1009 * salt)
    dw0, db0 = torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)
    if family == "b":
        (dy, dyh, dyl), (x, xh, xl) = exact_plane_values((M, N), gen), exact_plane_values((M, K), gen)
        assert torch.equal(split_planes(dy)[0], dyh) and torch.equal(split_planes(dy)[1], dyl)   # the planes are the drawn (h, l) exactly
        assert torch.equal(split_planes(x)[0], xh) and torch.equal(split_planes(x)[1], xl)
    else:
        dy, x = torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen) / M ** 0.5
        if family == "c":
            e = torch.randint(-20, 21, (N,), generator=gen).float()
            f = torch.randint(-20, 21, (K,), generator=gen).float()
            dy, x = dy * torch.exp2(e)[None, :], x * torch.exp2(f)[None, :]
            dw0, db0 = dw0 * torch.exp2(e[:, None] + f[None, :]), db0 * torch.exp2(e)
        if family == "d":
            dy = dy.bfloat16().float()
    if repeats:            # the index names every 7th row twice
        x = x.clone()
        x[1::7] = x[0::7][:len(x[1::7])]
    return Operands(dy, x, dw0, db0, with_gemm)


def case_operands(case, family):
    return [operands(p.shape, family, i, p.indexed, p.kernel is not None) for i, p in enumerate(case.products)]


def destinations(case):
    """{owner product: [products that add to its dw]}, in the order the case lists them"""
    out = {}
    for i, p in enumerate(case.products):
        if p.kernel is not None:
            out.setdefault(p.dst if p.dst >= 0 else i, []).append(i)
    return out


def dw_bar(case, ops, members, family, dw0):
    """(fp64 reference, bar per element, text) of one destination"""
    ref = dw0.double() + sum(ops[i].get("ref") for i in members)
    scale = sum(ops[i].get("scale") for i in members)
    kernels = [case.products[i].kernel for i in members]
    if family == "b" and X3 in kernels:
        f32 = dw0.clone()
        for i in members:
            f32 = f32 + ops[i].get("prod32")
        err32 = (f32.double() - ref).abs().max().item()
        bar = sum(ops[i].get("lolo") if k == X3 else F32_BAR * ops[i].get("scale") for i, k in zip(members, kernels)) + (4 * err32 + 1e-6)
        return ref, scale, bar, f"sum|dy_lo||x_lo| + 4 * {err32:.2e} + 1e-6"
    bar, text = sum(COEF[k] * ops[i].get("scale") for i, k in zip(members, kernels)), " + ".join(f"{COEF[k]:.0e} sum|dy||x|" for k in kernels)
    if all(case.products[i].shape[0] == 1 for i in members):            # a reduction of one row: the rounding of its landing
        bar, text = bar + HALF_ULP * (dw0.abs().double() + scale), text + " + half an ulp of the landing"
    return ref, scale, bar, text


def judge_dw(y, case, ops, owner, members, family, label):
    """prints the measured maximum and the fraction of the bar it uses, then asserts the bar"""
    ref, scale, bar, text = dw_bar(case, ops, members, family, ops[owner].dw0)
    err = (y.double() - ref).abs()
    rel, used = (err / scale).max().item(), (err / bar).max().item()
    print(f"WGRADFORM {label} dw[{owner}] {case.products[owner].shape} family {family}: max err / sum|dy||x| = {rel:.2e}; "
          f"max err / bar = {used:.3f} (bar = {text})")
    assert used <= 1.0, (label, owner, family, used)
    return used


def db_bar(o):
    bar = DB_BAR * o.get("colscale")
    return bar + HALF_ULP * (o.db0.abs().double() + o.get("colscale")) if o.dy.shape[0] == 1 else bar


def judge_db(y, o, family, label, i):
    ref = o.db0.double() + o.get("colref")
    bar = db_bar(o)
    err = (y.double() - ref).abs()
    rel, used = (err / o.get("colscale")).max().item(), (err / bar).max().item()
    print(f"WGRADFORM {label} db[{i}] family {family}: max err / sum|dy| = {rel:.2e}; max err / bar = {used:.3f} "
          f"(bar = {DB_BAR:.0e} sum|dy|{' + half an ulp of the landing' if o.dy.shape[0] == 1 else ''})")
    assert used <= 1.0, (label, i, family, used)
    return used


# ---- the recorded algorithm in torch on the CPU ------------------------------------------------------------------------------------
def slice_sum(total, segments):
    """k_slice_sum: per segment four chains over its slices and the remainder on the first, then ((s0 + s1) + (s2 + s3)) onto the total"""
    for parts in segments:
        s = [torch.zeros_like(total) for _ in range(4)]
        z = 0
        while z + 4 <= len(parts):
            for j in range(4):
                s[j] = s[j] + parts[z + j]
            z += 4
        for p in parts[z:]:
            s[0] = s[0] + p
        total = total + ((s[0] + s[1]) + (s[2] + s[3]))
    return total


def partials(o, p, drop=None):
    """the stored slices of one product: bf16 planes and three products with fp32 accumulation, or the exact fp32 product"""
    out = []
    for m0 in range(0, p.shape[0], p.rows_per_slice):
        dy, x = o.dy[m0:m0 + p.rows_per_slice], o.x[m0:m0 + p.rows_per_slice]
        if p.kernel != X3:
            out.append(dy.t() @ x)
            continue
        (dyh, dyl), (xh, xl) = split_planes(dy), split_planes(x)
        acc = dyl.t() @ xh                                              # x_hi dy_lo
        if drop != "x_lo dy_hi":
            acc = acc + dyh.t() @ xl
        out.append(acc + dyh.t() @ xh)
    assert len(out) == p.slices, (p, len(out))
    return out


def db_partials(o, p, hi_only=False):
    dy = split_planes(o.dy)[0] if hi_only else o.dy
    if p.db == "rides":                                                 # the rows of each slice of the product
        return [dy[m0:m0 + p.rows_per_slice].sum(0) for m0 in range(0, p.shape[0], p.rows_per_slice)]
    block = (torch.arange(p.shape[0]) // 4) % p.db_slices               # k_colsum_batch: rows 4 y + wave, stepping 4 by
    return [dy[block == y].sum(0) for y in range(p.db_slices)]


def emulate_dw(case, ops, members, dw0, drop=None):
    segments, total = [], dw0.clone()
    for i in members:
        p = case.products[i]
        parts = partials(ops[i], p, drop)
        if p.in_place:
            total = total + parts[0]
        elif case.reduce:                                               # k_splitk_reduce: the slices in order, then the destination
            s = torch.zeros_like(total)
            for part in parts:
                s = s + part
            total = s + total
        else:
            segments.append(parts)
    return slice_sum(total, segments)


# ---- CPU: the case table and the bars themselves -------------------------------------------------------------------------------
def test_case_table_covers_every_backward_form():
    forms = " | ".join(c.form for c in CASES)
    for wanted in FORMS_WANTED:
        assert wanted in forms, wanted
    ms = {p.shape[0] for c in CASES for p in c.products if p.kernel == X3}
    nks = {v for c in CASES for p in c.products if p.kernel == X3 for v in p.shape[1:]}
    assert {1024, 1055, 2080} <= ms and nks == {128, 132, 260, 516}
    small = [p for c in CASES if c.op == FG for p in c.products]
    assert {p.shape[0] for p in small} == {1, 127, 129, 512, 2048} and {p.slices for p in small} == {1, 2, 4}
    assert {v for p in small for v in p.shape[1:]} == {4, 68, 100, 192}
    sums = BY_NAME["colsum8"].products
    assert {p.shape[0] for p in sums} == {1, 255, 257, 5000} and {p.shape[1] for p in sums} == {4, 260, 768} and len(sums) == 8
    for c in CASES:                                                     # every option on and off among the split-bf16 products
        assert len(c.products) <= _lib.WGRAD_PROBE_MAX
    x3 = [p for c in CASES for p in c.products if p.kernel == X3]
    for option in ("db", "strided", "indexed"):
        assert {bool(getattr(p, option)) for p in x3} == {False, True}, option
    assert sum(1 for p in PASS16 if p.kernel == X3) == 11 and len(PASS16) == 16
    cut = {n: [p.slices for p in BY_NAME[n].products] for n in ("group2", "group2_cut", "group5_db", "group5_db_cut", "group8_db", "group8_db_cut")}
    for n in ("group2", "group5_db", "group8_db"):                      # a cut scratch: fewer slices for every product
        assert all(a > b for a, b in zip(cut[n], cut[n + "_cut"]))
    alone = {p.shape: p.slices for c in CASES if c.op == TN for p in c.products}
    assert BY_NAME["group8_db"].products[0].slices < alone[(1024, 128, 128)]   # slice lengths depend on the OTHER products


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_emulation_stays_inside_the_bars_and_mutants_do_not(name):
    """The bars are sharp without a GPU.  A torch emulation of the recorded algorithm (bf16 planes, fp32 accumulation, the slices
    added in the recorded order) stays inside every bar of every case and family.  On family b the same emulation without the
    x_lo dy_hi cross term, and a bias gradient summed from the hi plane of dy alone, exceed their bars by at least 50 x on EVERY
    element."""
    case = BY_NAME[name]
    for family in case.families:
        ops = case_operands(case, family)
        for owner, members in destinations(case).items():
            judge_dw(emulate_dw(case, ops, members, ops[owner].dw0), case, ops, owner, members, family, f"emulation {name}")
            if family == "b" and [case.products[i].kernel for i in members] == [X3]:
                ref, _, bar, _ = dw_bar(case, ops, members, family, ops[owner].dw0)
                broken = emulate_dw(case, ops, members, ops[owner].dw0, drop="x_lo dy_hi")
                over = ((broken.double() - ref).abs() / bar).min().item()
                print(f"WGRADFORM emulation {name} dw[{owner}]: a dropped cross term is at least {over:.0f} x bar b on EVERY element")
                assert over >= 50, over
        for i, p in enumerate(case.products):
            if not p.db:
                continue
            o = ops[i]
            judge_db(slice_sum(o.db0.clone(), [db_partials(o, p)]), o, family, f"emulation {name}", i)
            if family == "b":
                broken = slice_sum(o.db0.clone(), [db_partials(o, p, hi_only=True)])
                bar = db_bar(o)
                over = ((broken.double() - (o.db0.double() + o.get("colref"))).abs() / bar).min().item()
                print(f"WGRADFORM emulation {name} db[{i}]: summed from the hi plane alone it is at least {over:.0f} x its bar on EVERY element")
                assert over >= 50, over


def test_a_one_row_reduction_needs_the_rounding_of_its_landing():
    """Why the bar of a one-row reduction carries 2^-24 (|dw0| + sum|dy||x|): there the exact-fp32 emulation - one product added to
    dw0, nothing a kernel could do better - is outside 5e-6 sum|dy||x| alone, and inside it with the half ulp of that addition;
    the same for a column sum over one row.  (Every other shape is held inside the plain bar by the emulation test above.)"""
    case = BY_NAME["pass_small_instalment"]
    assert case.products[1].shape == (1, 68, 100)                       # 6 800 elements: some products are far below their dw0
    o = case_operands(case, "a")[1]
    y = emulate_dw(case, [None, o], [1], o.dw0)
    err = (y.double() - (o.dw0.double() + o.get("ref"))).abs()
    plain = (err / (F32_BAR * o.get("scale"))).max().item()
    amended = (err / (F32_BAR * o.get("scale") + HALF_ULP * (o.dw0.abs().double() + o.get("scale")))).max().item()
    print(f"WGRADFORM rows = 1: dw emulation at {plain:.1f} x the plain bar, {amended:.3f} x the bar with the landing's half ulp")
    assert plain > 1.0 >= amended
    sums = BY_NAME["colsum8"]
    assert sums.products[5].shape[:2] == (1, 768)
    o = case_operands(sums, "a")[5]
    err = (slice_sum(o.db0.clone(), [db_partials(o, sums.products[5])]).double() - (o.db0.double() + o.get("colref"))).abs()
    plain, amended = (err / (DB_BAR * o.get("colscale"))).max().item(), (err / db_bar(o)).max().item()
    print(f"WGRADFORM rows = 1: db emulation at {plain:.1f} x the plain bar, {amended:.3f} x the bar with the landing's half ulp")
    assert plain > 1.0 >= amended


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(request):
    """a kernel fault poisons the process: no later case may start more work on that GPU"""
    yield
    if request.node.get_closest_marker("gpu") is not None:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU reported a fault after {request.node.name}: {e}", returncode=3)


def stream():
    return torch.cuda.current_stream().cuda_stream


def padded(t, ld):
    """t [rows][cols] inside a [rows][ld] buffer whose pad columns hold NaN"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)


class Scratch:
    def __init__(self, floats):
        self.floats = floats
        self.buf = torch.full((floats + GUARD,), NAN, device=DEV)
        self.buf[floats:] = 12345.0

    def intact(self):
        return bool((self.buf[self.floats:] == 12345.0).all())


class Dest:
    """a [rows][cols] destination inside a [rows + 1][cols + 4] buffer: y0 inside, NaN in the pad columns and the spare row"""

    def __init__(self, y0):
        self.rows, self.cols = y0.shape
        self.ld = self.cols + 4
        buf = torch.full((self.rows + 1, self.ld), NAN)
        buf[:self.rows, :self.cols] = y0
        self.buf = buf.to(DEV)
        self.before = self.buf.clone()

    @property
    def y(self):
        return self.buf[:self.rows, :self.cols]

    def pads_untouched(self):
        a, b = self.buf.view(torch.int32), self.before.view(torch.int32)
        return bool((a[:, self.cols:] == b[:, self.cols:]).all() and (a[self.rows] == b[self.rows]).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == self.before.view(torch.int32)).all())


class Device:
    """the operands of one case on the GPU in the layouts the case asks for, and its destinations"""

    def __init__(self, case, ops):
        self.case, self.keep, self.dw, self.db = case, [], {}, {}
        self.args = _lib.DrinWgradProbeArgsC(struct_size=C.sizeof(_lib.DrinWgradProbeArgsC), op=case.op, precision=case.precision,
                                             staged=int(case.staged), n_products=len(case.products), layers_done_after=case.layers_done_after)
        self.scratch = Scratch(case.scratch) if case.scratch else None
        if self.scratch is not None:
            self.args.scratch, self.args.scratch_floats = self.scratch.buf.data_ptr(), self.scratch.floats
        for i, (p, o) in enumerate(zip(case.products, ops)):
            M, N, K = p.shape
            lddy, ldx = N + (8 if "dy" in p.strided else 0), K + (16 if "x" in p.strided else 0)
            q = _lib.DrinWgradProductC(lddy=lddy, ldx=ldx, rows=M, n_out=N, k=K)
            dy = padded(o.dy, lddy)
            self.keep.append(dy)
            q.dy = dy.data_ptr()
            if p.kernel is not None:
                x = o.x
                if p.indexed:   # a permutation of a larger table, every 7th entry repeating its neighbour; unnamed rows hold NaN
                    gen = torch.Generator().manual_seed(M)
                    index = torch.randperm(M + 64, generator=gen)[:M]
                    index[1::7] = index[0::7][:len(index[1::7])]
                    table = torch.full((M + 64, K), NAN)
                    table[index] = o.x
                    x, index = table, index.to(DEV)
                    self.keep.append(index)
                    q.x_index = index.data_ptr()
                x = padded(x, ldx)
                self.keep.append(x)
                q.x = x.data_ptr()
                owner = p.dst if p.dst >= 0 else i
                if owner not in self.dw:
                    self.dw[owner] = Dest(ops[owner].dw0)
                q.dw, q.lddw = self.dw[owner].buf.data_ptr(), self.dw[owner].ld
            if p.db:
                self.db[i] = Dest(o.db0[None, :])
                q.db = self.db[i].buf.data_ptr()
            self.args.product[i] = q

    def run(self):
        rc = _lib.load().drin_wgrad_probe(C.byref(self.args), stream())
        return rc, self.args.route

    def everything_untouched(self):
        return all(d.untouched() for d in list(self.dw.values()) + list(self.db.values()))


def assert_route(route, case):
    label = case.name
    got = {k: (tuple(route.grid[:route.gemm_launches]) if k == "grid" else getattr(route, k)) for k in case.call}
    assert got == case.call, f"{label}: the call recorded {got}, the case is there for {case.call}: move the shape"
    for i, p in enumerate(case.products):
        r = route.product[i]
        got = dict(kernel=_lib.WGRAD_KERNEL[r.kernel], slices=r.slices, rows_per_slice=r.rows_per_slice, in_place=r.in_place,
                   launch=r.launch, db_rode=r.db_rode, db_slices=r.db_slices)
        want = dict(kernel=p.kernel or "none", slices=p.slices, rows_per_slice=p.rows_per_slice, in_place=p.in_place, launch=p.launch,
                    db_rode=int(p.db == "rides"), db_slices=p.db_slices)
        assert got == want, f"{label}: product {i} {p.shape} took {got}, the case is there for {want}: move the shape"


def run_case(case, family):
    ops = case_operands(case, family)
    dev = Device(case, ops)
    rc, route = dev.run()
    assert rc == _lib.OK, _lib.load().drin_last_error()
    assert_route(route, case)
    torch.cuda.synchronize()
    assert dev.scratch is None or dev.scratch.intact(), f"{case.name}: wrote behind the scratch"
    for d in list(dev.dw.values()) + list(dev.db.values()):
        assert d.pads_untouched(), f"{case.name}: a pad column or the spare row changed"
    return ops, dev


def judge_case(case, family, ops, dev, label):
    for owner, members in destinations(case).items():
        judge_dw(dev.dw[owner].y.cpu(), case, ops, owner, members, family, label)
    for i, d in dev.db.items():
        judge_db(d.y.cpu()[0], ops[i], family, label, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family", RUNS)
def test_form_against_fp64(name, family):
    case = BY_NAME[name]
    ops, dev = run_case(case, family)
    judge_case(case, family, ops, dev, name)
    if case.op == PASS:                                                 # the same bits on a second run
        _, again = run_case(case, family)
        for k in dev.dw:
            assert torch.equal(dev.dw[k].buf.view(torch.int32), again.dw[k].buf.view(torch.int32)), (name, "dw", k)
        for k in dev.db:
            assert torch.equal(dev.db[k].buf.view(torch.int32), again.db[k].buf.view(torch.int32)), (name, "db", k)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["a", "b", "c"])
@pytest.mark.parametrize("pair", ["pass16", "pass_split8"])
def test_staged_pass_equals_the_plain_one_within_the_bar(pair, family):
    """pass16: at its sizes both parts take the 128-row floor and the two passes agree bit for bit; pass_split8: the staged parts
    take 288- and 192-row slices against the plain pass's 544 (asserted by the route records), so they differ in the last bits."""
    plain, staged = BY_NAME[pair], BY_NAME[pair + "_staged"]
    ops, a = run_case(plain, family)
    _, b = run_case(staged, family)
    for owner, members in destinations(plain).items():
        _, _, bar, _ = dw_bar(plain, ops, members, family, ops[owner].dw0)
        used = ((a.dw[owner].y.cpu().double() - b.dw[owner].y.cpu().double()).abs() / bar).max().item()
        print(f"WGRADFORM staged - plain {pair} dw[{owner}] family {family}: {used:.3f} of the bar")
        assert used <= 1.0, (owner, used)
    for i in a.db:                                                      # the column sums and the riding sums split alike in both
        o = ops[i]
        bar = db_bar(o)
        assert bool(((a.db[i].y.cpu()[0].double() - b.db[i].y.cpu()[0].double()).abs() <= bar).all()), i


def refused(case, status, needle):
    dev = Device(case, case_operands(case, "a"))
    rc, route = dev.run()
    torch.cuda.synchronize()
    assert rc == status and needle in _lib.load().drin_last_error(), (rc, _lib.load().drin_last_error())
    assert (route.gemm_launches, route.colsum_launches, route.sum_launches, route.reduce_launches) == (0, 0, 0, 0)
    assert all(route.product[i].kernel == 0 and route.product[i].db_slices == 0 for i in range(_lib.WGRAD_PROBE_MAX))
    assert dev.everything_untouched() and (dev.scratch is None or dev.scratch.intact())


@pytest.mark.gpu
def test_group_scratch_too_small_at_one_slice_each_is_refused_and_nothing_runs():
    """one slice of each of the five products and their column sums is 286 772 floats: four fewer, DRIN_E_WORKSPACE"""
    full = BY_NAME["group5_db"]
    need = sum(p.shape[1] * (p.shape[2] + (1 if p.db else 0)) for p in full.products)
    assert need == 286772
    refused(Case("too_small", "", G, full.products, {}, scratch=need - 4), _lib.E_WORKSPACE, b"slice scratch")
    one_each = Case("one_slice_each", "", G, tuple(P(**{**p.__dict__, "slices": 1, "rows_per_slice": 32 * -(-p.shape[0] // 32)}) for p in full.products),
                    full.call | dict(grid=(sum(-(-p.shape[1] // 256) * -(-p.shape[2] // 256) for p in full.products),)), scratch=need)
    ops, dev = run_case(one_each, "a")                                  # and with exactly that much: one slice each
    judge_case(one_each, "a", ops, dev, "one slice each")


@pytest.mark.gpu
def test_mention_sized_group_refuses_2049_rows():
    refused(Case("f32_2049", "", FG, (P((127, 68, 100), FS), P((2049, 68, 100), FS)), {}), _lib.E_SHAPE, b"mention-sized")


@pytest.mark.gpu
def test_a_ninth_column_sum_is_refused():
    nine = BY_NAME["colsum8"].products + (P((255, 4, 4), None, db="batch"),)
    refused(Case("colsum9", "", CS, nine, {}), _lib.E_SHAPE, b"at most 8 sums")


# dX = dY W --------------------------------------------------------------------------------------------------------------------
NONE, WT_F32, WT_PLANES = _lib.WGRAD_WT_NONE, _lib.WGRAD_WT_F32_SCRATCH, _lib.WGRAD_WT_PLANES
NN_CASES = {
    # name: ((rows, outputs, reduction) of launch_gemm_nn, precision, wt_form asked, split-K scratch, expected record)
    "x3_1024_planes": ((1024, 128, 128), _lib.PREC_BF16X3, WT_PLANES, None, dict(nn_family="bf16x3", nn_bm=64, nn_bn=128, nn_wt_form=WT_PLANES, grid=(16,))),
    "x3_1024_f32_wt": ((1024, 128, 128), _lib.PREC_BF16X3, WT_F32, None, dict(nn_family="bf16x3", nn_bm=64, nn_bn=128, nn_wt_form=WT_F32, grid=(16,))),
    "x3_1024_no_wt": ((1024, 128, 128), _lib.PREC_BF16X3, NONE, None, dict(nn_family="f32", nn_bm=64, nn_bn=64, nn_wt_form=NONE, nn_splits=1, grid=(32,))),
    "x3_1500_planes": ((1500, 260, 96), _lib.PREC_BF16X3, WT_PLANES, None, dict(nn_family="bf16x3", nn_bm=64, nn_bn=128, nn_wt_form=WT_PLANES, grid=(72,))),
    "x3_1500_f32_wt": ((1500, 260, 96), _lib.PREC_BF16X3, WT_F32, None, dict(nn_family="bf16x3", nn_bm=64, nn_bn=128, nn_wt_form=WT_F32, grid=(72,))),
    "x3_1500_no_wt": ((1500, 260, 96), _lib.PREC_BF16X3_ALL, NONE, None, dict(nn_family="f32", nn_bm=64, nn_bn=64, nn_wt_form=NONE, nn_splits=1, grid=(120,))),
    "f32_small_splitk": ((300, 768, 768), _lib.PREC_F32, NONE, BIG, dict(nn_family="f32", nn_bm=64, nn_bn=64, nn_wt_form=NONE, nn_splits=6, grid=(360,),
                                                                        reduce_launches=1)),
    "f32_64x64": ((300, 68, 64), _lib.PREC_F32, NONE, None, dict(nn_family="f32", nn_bm=64, nn_bn=64, nn_wt_form=NONE, nn_splits=1, grid=(10,))),
}


@functools.lru_cache(maxsize=4)
def nn_operands(shape, family):
    """dX [M][N] = dY [M][Kr] W [Kr][N]; family c scales row m of dY by 2^e[m] and column n of W by 2^f[n] (dx0 alike)"""
    M, N, Kr = shape
    gen = torch.Generator().manual_seed(M * 31 + N * 7 + Kr + ord(family))
    dx0 = torch.randn(M, N, generator=gen)
    if family == "b":
        (dy, _, dyl), (w, _, wl) = exact_plane_values((M, Kr), gen), exact_plane_values((Kr, N), gen)
        lolo = dyl.double() @ wl.double()
    else:
        dy, w, lolo = torch.randn(M, Kr, generator=gen), torch.randn(Kr, N, generator=gen) / Kr ** 0.5, None
        if family == "c":
            e, f = torch.randint(-20, 21, (M,), generator=gen).float(), torch.randint(-20, 21, (N,), generator=gen).float()
            dy, w, dx0 = dy * torch.exp2(e)[:, None], w * torch.exp2(f)[None, :], dx0 * torch.exp2(e[:, None] + f[None, :])
        if family == "d":
            dy = dy.bfloat16().float()
    return dy, w, dx0, dy.double() @ w.double(), (dy.abs() @ w.abs()).double(), lolo, dy @ w


def nn_families(split_bf16):
    return ("a", "b", "c", "d") if split_bf16 else ("a", "b", "c")


def nn_bar(ops, family, split_bf16, accumulate):
    """(fp64 reference, bar per element, text)"""
    dy, w, dx0, ref, scale, lolo, prod32 = ops
    if accumulate:
        ref, prod32 = ref + dx0.double(), prod32 + dx0
    if split_bf16 and family == "b":
        err32 = (prod32.double() - ref).abs().max().item()
        return ref, lolo + (4 * err32 + 1e-6), f"sum|dy_lo||w_lo| + 4 * {err32:.2e} + 1e-6"
    coef = BF16X3_BAR if split_bf16 else F32_BAR
    return ref, coef * scale, f"{coef:.0e} sum|dy||w|"


def nn_judge(y, ops, family, split_bf16, accumulate, label):
    scale = ops[4]
    ref, bar, text = nn_bar(ops, family, split_bf16, accumulate)
    err = (y.double() - ref).abs()
    used = (err / bar).max().item()
    print(f"WGRADFORM nn {label} family {family}: max err / sum|dy||w| = {(err / scale).max().item():.2e}; max err / bar = {used:.3f} (bar = {text})")
    assert used <= 1.0, (label, family, used)


def nn_emulate(ops, split_bf16, accumulate, splits=1, drop=False):
    dy, w, dx0 = ops[:3]
    if split_bf16:
        (dh, dl), (wh, wl) = split_planes(dy), split_planes(w)
        y = dh @ wh + dh @ wl
        if not drop:
            y = y + dl @ wh
    else:
        cdiv = lambda a, b: -(-a // b)
        kps = cdiv(cdiv(dy.shape[1], splits), 32) * 32
        y = torch.zeros_like(dx0)
        for k0 in range(0, dy.shape[1], kps):
            y = y + dy[:, k0:k0 + kps] @ w[k0:k0 + kps]
    return y + dx0 if accumulate else y


@pytest.mark.parametrize("name", sorted(NN_CASES))
def test_nn_emulation_stays_inside_the_bars_and_a_dropped_term_does_not(name):
    shape, _, _, _, want = NN_CASES[name]
    split_bf16 = want["nn_family"] == "bf16x3"
    for family in nn_families(split_bf16):
        ops = nn_operands(shape, family)
        for accumulate in (False, True):
            nn_judge(nn_emulate(ops, split_bf16, accumulate, want.get("nn_splits", 1)), ops, family, split_bf16, accumulate, f"emulation {name}")
        if split_bf16 and family == "b":
            ref, bar, _ = nn_bar(ops, family, True, False)
            over = ((nn_emulate(ops, True, False, drop=True).double() - ref).abs() / bar).min().item()
            print(f"WGRADFORM nn emulation {name}: a dropped cross term is at least {over:.0f} x bar b on EVERY element")
            assert over >= 50, over


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("name", sorted(NN_CASES))
def test_nn_form_against_fp64(name, accumulate):
    """dX through launch_gemm_nn in each WtForms: the planes of W^T written by launch_transpose_split_batch (the form the model's
    backward uses), an fp32 W^T transposed into scratch, and none - where a split-bf16 precision must record the exact-fp32 family."""
    shape, precision, wt_form, scratch_floats, want = NN_CASES[name]
    M, N, Kr = shape
    split_bf16 = want["nn_family"] == "bf16x3"
    for family in nn_families(split_bf16):
        dy, w, dx0 = nn_operands(shape, family)[:3]
        out = Dest(dx0 if accumulate else torch.full((M, N), NAN))
        dyd, wd = padded(dy, Kr + 8), w.to(DEV)
        scratch = Scratch(scratch_floats) if scratch_floats else None
        wt = Scratch(N * Kr) if wt_form != NONE else None
        args = _lib.DrinWgradProbeArgsC(struct_size=C.sizeof(_lib.DrinWgradProbeArgsC), op=_lib.WGRAD_NN, precision=precision, n_products=1,
                                        layers_done_after=-1, accumulate=int(accumulate), wt_form=wt_form)
        if scratch is not None:
            args.scratch, args.scratch_floats = scratch.buf.data_ptr(), scratch.floats
        if wt is not None:
            args.wt, args.wt_floats = wt.buf.data_ptr(), wt.floats
        args.product[0] = _lib.DrinWgradProductC(dy=dyd.data_ptr(), lddy=Kr + 8, x=wd.data_ptr(), ldx=N, dw=out.buf.data_ptr(), lddw=out.ld,
                                                 rows=M, n_out=Kr, k=N)
        rc = _lib.load().drin_wgrad_probe(C.byref(args), stream())
        assert rc == _lib.OK, _lib.load().drin_last_error()
        r = args.route
        got = dict(nn_family=_lib.GEMM_FAMILY[r.nn_family], nn_bm=r.nn_bm, nn_bn=r.nn_bn, nn_wt_form=r.nn_wt_form, nn_splits=r.nn_splits,
                   grid=tuple(r.grid[:r.gemm_launches]), reduce_launches=r.reduce_launches, nn_accumulate=r.nn_accumulate)
        expect = dict(dict(nn_splits=1, reduce_launches=0), **want, nn_accumulate=int(accumulate))
        assert got == expect, f"{name}: the dispatch code took {got}, the case is there for {expect}: move the shape"
        torch.cuda.synchronize()
        y = out.y.cpu()
        assert bool(torch.isfinite(y).all()), f"{name}: elements of the product were not written"
        assert out.pads_untouched() and (scratch is None or scratch.intact()) and (wt is None or wt.intact())
        nn_judge(y, nn_operands(shape, family), family, split_bf16, accumulate, f"{name} {'accumulate' if accumulate else 'store'}")
