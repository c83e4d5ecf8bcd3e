"""Every split-bf16 NT GEMM form against an fp64 product, through `drin_gemm_probe`.

The GEMM module chooses among about twenty kernel forms by size gates.  Each case below is the smallest shape that selects one
form; the test first asserts the ROUTE RECORD that the dispatch code wrote next to its launch (never a restatement of the gates:
a gate that moves turns the case red instead of leaving the form untested), then compares the output with the fp64 product of the
same operands on the CPU.

Contracts of every case: `y` lives in a wider buffer (`ldy = n_out + 4`, one spare row) prefilled with NaN - or with a random
`y0` under `accumulate` - every element of the product is written and no pad column, spare row or guard behind the scratch
changes; strided operands carry NaN in their pad columns.

Input families (per case):
  a  randn (w / sqrt(k)), as the older tests
  b  same-sign operands with exact planes: v = h + l, h a random bf16 in [1, 2), l = 2^-9 (a random bf16 in [0.5, 1)), so hi = h and
     lo = l exactly and every partial product has one sign: a dropped cross term shows at 2^-9 instead of 1e-3 / sqrt(k)
  c  family a with every row of x and of w multiplied by a random power of two in 2^+-20 (bias and y0 scaled alike, see `inputs`)
  d  (activation without a lo plane) x drawn as bf16 values; b and c then use bf16 values for x as well

Bars (none tuned on a kernel's output; `test_emulation_stays_inside_the_bars_and_a_dropped_term_does_not` holds them against a
torch emulation of the algorithm on the CPU):
  a, c, d  |y - ref| <= 2e-5 sum|x||w| per element: the project's split-bf16 bar (test_linear_fwd_bf16x3)
  b        |y - ref| <= sum|x_lo||w_lo| (fp64; the one partial product the algorithm drops) + 4 err32 + 1e-6, err32 = the largest
           error of torch's CPU fp32 product of the same operands (the accumulation-order margin of test_linear_fwd)
  fp16     one pass on fp16 planes is exact per product: against fp64 of the QUANTISED operands, 4 err32 + 1e-6, taken before
           the power-of-two scales are applied (applying them is exact, so this asks no less than the scaled comparison)

Measured maxima: DESIGN.md section 17.
"""
import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Optional

import pytest
import torch

from drin_amd import _lib

DEV = "cuda"
BF16X3_BAR = 2e-5
SCRATCH_FLOATS = 1 << 22   # "a large aligned scratch": 16 MiB, more than any split of these shapes needs
GUARD = 1024               # floats behind the scratch that nothing may touch
NAN = float("nan")


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    form: str                    # the kernel form the case is there for (variants of one form share it)
    op: int
    shape: tuple                 # (rows, n_out, k)
    route: dict                  # expected route record (the fields that name the form)
    weights: str = "f32"         # "f32" | "planes" (bf16 hi / lo planes of w)
    a_lo: bool = True            # False: the activation is exact in bf16, no lo plane (planes launchers)
    scratch: Optional[int] = None   # floats of scratch, None: no scratch
    bias: bool = True
    accumulate: bool = False
    strided: bool = False        # ldx = k + 8, ldw = k + 16 instead of k
    indexed: bool = False        # rows through a_index: a permutation with repeats into a larger table
    families: tuple = ("a", "b", "c")

    @property
    def kind(self):              # what x holds: "f32" values or "bf16" values
        return "f32" if self.a_lo else "bf16"


NT, X3, P4, PL, F16 = (_lib.PROBE_GEMM_NT, _lib.PROBE_GEMM_NT_BF16X3, _lib.PROBE_GEMM_NT_BF16X3_P4, _lib.PROBE_GEMM_X3_PLANES,
                       _lib.PROBE_GEMM_F16_PLANES)
BIG = SCRATCH_FLOATS
D = ("d", "b", "c")


def r(family, bm=256, bn=256, **kw):
    return dict(family=family, bm=bm, bn=bn, **kw)


CASES = [
    # launch_gemm_nt, DRIN_PREC_BF16X3_ALL, fp32 weights
    Case("nt_64x128_ksplit16", "bf16x3 64x128 all-tiles K split", NT, (101, 768, 2048),
         r("bf16x3", 64, 128, w_planes=0, tiles=12, whole_tiles=0, ksplit=16, indexed=0), scratch=BIG),
    Case("nt_256_f32w", "bf16x3 256x256 fp32 weights", NT, (6044, 2048, 64),
         r("bf16x3", w_planes=0, tiles=192, whole_tiles=192, ksplit=1, indexed=0), bias=False, strided=True),
    Case("nt_256_f32w_tail4", "bf16x3 256x256 fp32 weights, tail split", NT, (7324, 2052, 512),
         r("bf16x3", w_planes=0, tiles=261, whole_tiles=256, ksplit=4, indexed=0), scratch=BIG),
    Case("x3_256_f32w_tail4_acc", "bf16x3 256x256 fp32 weights, tail split", X3, (7324, 2052, 512),
         r("bf16x3", w_planes=0, tiles=261, whole_tiles=256, ksplit=4, accumulate=1), scratch=BIG, bias=False, accumulate=True, strided=True),
    # the same launcher with weight planes
    Case("nt_64x128_planes", "bf16x3 64x128 planes", NT, (513, 260, 96),
         r("bf16x3", 64, 128, w_planes=1, tiles=27, whole_tiles=27, ksplit=1, indexed=0), weights="planes"),
    Case("x3_64x128_planes_acc", "bf16x3 64x128 planes", X3, (513, 260, 96),
         r("bf16x3", 64, 128, w_planes=1, tiles=27, accumulate=1, indexed=0), weights="planes", bias=False, accumulate=True, strided=True),
    Case("nt_bm96", "bf16x3 96x256 planes", NT, (6081, 768, 64), r("bf16x3", 96, 256, w_planes=1, tiles=192), weights="planes"),
    Case("nt_bm128", "bf16x3 128x256 planes", NT, (8190, 768, 64), r("bf16x3", 128, 256, w_planes=1, tiles=192), weights="planes", bias=False),
    Case("x3_bm128_acc", "bf16x3 128x256 planes", X3, (8190, 768, 64), r("bf16x3", 128, 256, w_planes=1, tiles=192, accumulate=1),
         weights="planes", accumulate=True, strided=True),
    Case("nt_bm160", "bf16x3 160x256 planes", NT, (10891, 768, 64), r("bf16x3", 160, 256, w_planes=1, tiles=207), weights="planes"),
    Case("nt_p4", "bf16x3_p4", NT, (6044, 2048, 64),
         r("bf16x3_p4", w_planes=1, persist=0, tiles=192, whole_tiles=192, ksplit=1), weights="planes"),
    Case("p4_acc", "bf16x3_p4", P4, (6044, 2048, 64),
         r("bf16x3_p4", persist=0, tiles=192, whole_tiles=192, ksplit=1, accumulate=1), weights="planes", bias=False, accumulate=True, strided=True),
    Case("nt_p4_tail4", "bf16x3_p4 tail split", NT, (7324, 2052, 512),
         r("bf16x3_p4", persist=0, tiles=261, whole_tiles=256, ksplit=4), weights="planes", scratch=BIG, bias=False),
    Case("p4_tail4_acc", "bf16x3_p4 tail split", P4, (7324, 2052, 512),
         r("bf16x3_p4", persist=0, tiles=261, whole_tiles=256, ksplit=4, accumulate=1), weights="planes", scratch=BIG, accumulate=True, strided=True),
    Case("x3_256_planes_indexed", "bf16x3 256x256 planes, indexed rows", X3, (6044, 2048, 64),
         r("bf16x3", w_planes=1, indexed=1, tiles=192, whole_tiles=192, ksplit=1), weights="planes", indexed=True),
    Case("x3_64x128_planes_indexed", "bf16x3 64x128 planes, indexed rows", X3, (513, 260, 96),
         r("bf16x3", 64, 128, w_planes=1, indexed=1, tiles=27), weights="planes", indexed=True, bias=False),
    # launch_gemm_x3_planes
    Case("pl_2ph_splitk8", "planes two-phase <true,true> split K", PL, (101, 768, 768),
         r("planes", a_lo=1, splits=8, ksplit=1, tiles=3), weights="planes", scratch=BIG),
    Case("pl_2ph_nolo", "planes two-phase <false,true>", PL, (300, 768, 64),
         r("planes", a_lo=0, splits=1, ksplit=1, tiles=6, whole_tiles=6), weights="planes", a_lo=False, bias=False, strided=True, families=D),
    Case("pl_2ph_nolo_splitk8", "planes two-phase <false,true> split K", PL, (300, 768, 768),
         r("planes", a_lo=0, splits=8, ksplit=1, tiles=6), weights="planes", a_lo=False, scratch=BIG, families=D),
    Case("pl_2ph_tail2", "planes two-phase tail split", PL, (300, 258, 256),
         r("planes", a_lo=1, splits=1, ksplit=2, tiles=4, whole_tiles=0), weights="planes", scratch=BIG, strided=True),
    Case("pl_p4_single_tile_tail2", "planes_p4 <true> tail split of a single tile", PL, (256, 256, 256),
         r("planes_p4", a_lo=1, f16=0, persist=0, tiles=1, whole_tiles=0, ksplit=2), weights="planes", scratch=65536, bias=False),
    Case("pl_p4_nolo", "planes_p4 <false,false,false>", PL, (10958, 768, 64),
         r("planes_p4", a_lo=0, f16=0, persist=0, tiles=129, whole_tiles=129, ksplit=1), weights="planes", a_lo=False, families=D),
    Case("pl_p4_nolo_tail4", "planes_p4 <false,false,false> tail split", PL, (21966, 768, 512),
         r("planes_p4", a_lo=0, f16=0, persist=0, tiles=258, whole_tiles=256, ksplit=4), weights="planes", a_lo=False, scratch=BIG,
         bias=False, strided=True, families=D),
    Case("pl_p4_tail4", "planes_p4 <true> tail split", PL, (7324, 2052, 512),
         r("planes_p4", a_lo=1, f16=0, persist=0, tiles=261, whole_tiles=256, ksplit=4), weights="planes", scratch=BIG, strided=True),
]
BY_NAME = {c.name: c for c in CASES}
# (case, family), neighbours sharing their operands and reference (`inputs` keeps the last few)
RUNS = sorted(((c, f) for c in CASES for f in c.families), key=lambda cf: (cf[0].shape, cf[0].kind, cf[1], cf[0].name))


# ---- operands and references (CPU, computed once per shape / family / kind and shared: never written to) ----------------------
def split_planes(v):
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


def exact_plane_values(shape, gen, with_lo):
    h = 1 + torch.randint(0, 128, shape, generator=gen).float() / 128            # bf16 in [1, 2)
    l = 2.0 ** -9 * (0.5 + torch.randint(0, 128, shape, generator=gen).float() / 256)   # 2^-9 x (bf16 in [0.5, 1))
    return (h + l if with_lo else h), h, (l if with_lo else torch.zeros(shape))


@dataclass
class Operands:
    x: torch.Tensor
    w: torch.Tensor
    bias: torch.Tensor
    y0: torch.Tensor
    ref: torch.Tensor          # fp64 x w^T (no bias, no y0)
    scale: torch.Tensor        # sum |x||w| per element
    lolo: Optional[torch.Tensor]   # family b: sum |x_lo||w_lo| in fp64
    prod32: torch.Tensor       # torch's CPU fp32 product x w^T
    planes: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=2)
def inputs(shape, family, kind):
    """Operands of one (shape, family, kind) with their fp64 product.  Family c scales row m of x by 2^e[m] and row n of w by 2^f[n];
    element (m, n) of the product then lives at 2^(e[m] + f[n]), so y0 is scaled by that and bias[n] by 2^(f[n] - 20) (the size of
    the product in the rows with the smallest e): an fp32 sum with a term 2^40 times larger than sum|x||w| could not meet any bar
    relative to sum|x||w|, whatever the kernel."""
    M, N, K = shape
    gen = torch.Generator().manual_seed(M * 31 + N * 7 + K + ord(family))
    bias, y0 = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen)
    lolo = None
    if family == "b":
        x, xh, xl = exact_plane_values((M, K), gen, with_lo=kind == "f32")
        w, wh, wl = exact_plane_values((N, K), gen, with_lo=True)
        lolo = xl.double() @ wl.double().t()
    else:
        x, w = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5
        if family == "c":
            e = torch.randint(-20, 21, (M,), generator=gen).float()
            f = torch.randint(-20, 21, (N,), generator=gen).float()
            x, w = x * torch.exp2(e)[:, None], w * torch.exp2(f)[:, None]
            bias, y0 = bias * torch.exp2(f - 20), y0 * torch.exp2(e[:, None] + f[None, :])
        if kind == "bf16":
            x = x.bfloat16().float()
    ref = x.double() @ w.double().t()
    scale = (x.abs() @ w.abs().t()).double()      # all terms of one sign: fp32 gives it to 1e-5, plenty for a denominator
    o = Operands(x, w, bias, y0, ref, scale, lolo, x @ w.t())
    o.planes["x"], o.planes["w"] = split_planes(x), split_planes(w)
    if family == "b":                             # the planes are the drawn (h, l) exactly
        assert torch.equal(o.planes["x"][0].float(), xh) and torch.equal(o.planes["x"][1].float(), xl)
        assert torch.equal(o.planes["w"][0].float(), wh) and torch.equal(o.planes["w"][1].float(), wl)
    return o


def expected(o, case):
    """fp64 reference of the case and err32, the largest error of the CPU fp32 evaluation of the same expression"""
    ref, f32 = o.ref, o.prod32
    if case.bias:
        ref, f32 = ref + o.bias.double(), f32 + o.bias
    if case.accumulate:
        ref, f32 = ref + o.y0.double(), f32 + o.y0
    return ref, (f32.double() - ref).abs().max().item()


def judge(y, o, case, family, label):
    """prints the measured maximum, then asserts the family's bar"""
    ref, err32 = expected(o, case)
    err = (y.double() - ref).abs()
    rel = (err / o.scale).max().item()
    if family == "b":
        bar = o.lolo + (4 * err32 + 1e-6)
        used = (err / bar).max().item()
        print(f"GEMMFORM {label} family {family}: max err / sum|x||w| = {rel:.2e}; max err / bar = {used:.3f} "
              f"(bar = sum|x_lo||w_lo| + 4 * {err32:.2e} + 1e-6; sum|x_lo||w_lo| up to {o.lolo.max().item():.2e})")
        assert used <= 1.0, (label, family, used)
    else:
        print(f"GEMMFORM {label} family {family}: max err / sum|x||w| = {rel:.2e} (bar {BF16X3_BAR:.0e})")
        assert rel <= BF16X3_BAR, (label, family, rel)
    return rel


def emulate(o, a_lo=True, drop=None):
    """the algorithm in torch on the CPU: bf16 planes, three (a_lo: two) products, fp32 accumulation"""
    (xh, xl), (wh, wl) = ((p.float() for p in o.planes[n]) for n in ("x", "w"))
    y = xh @ wh.t()
    if drop != "x_hi w_lo":
        y = y + xh @ wl.t()
    if a_lo and drop != "x_lo w_hi":
        y = y + xl @ wh.t()
    return y


# ---- CPU: the case table and the bars themselves -------------------------------------------------------------------------------
def test_case_table_names_distinct_routes_and_covers_every_option():
    forms = {}
    for c in CASES:
        forms.setdefault(c.form, c)
    assert len(forms) == 19
    keys = ("family", "bm", "bn", "w_planes", "a_lo", "persist", "indexed", "ksplit", "splits", "whole_tiles", "tiles")
    seen = {}
    for form, c in forms.items():
        sig = tuple(c.route.get(k) for k in keys)
        assert sig not in seen, (form, seen.get(sig))
        seen[sig] = form
    for fam in ("bf16x3", "bf16x3_p4", "planes", "planes_p4"):
        mine = [c for c in CASES if c.route["family"] == fam]
        for option in ("bias", "strided") + (("accumulate",) if fam.startswith("bf16x3") else ()):
            assert {getattr(c, option) for c in mine} == {False, True}, (fam, option)


SHAPE_KINDS = sorted({(c.shape, c.kind) for c in CASES} | {((1499, 768, 96), "f32")})


@pytest.mark.parametrize("shape,kind", SHAPE_KINDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_emulation_stays_inside_the_bars_and_a_dropped_term_does_not(shape, kind):
    """The bars are sharp without a GPU: a torch emulation of the algorithm (bf16 planes, fp32 accumulation) stays inside every bar
    at every listed shape, and the same emulation without one cross term - x_lo w_hi; for an activation without a lo plane the
    one cross term there is, x_hi w_lo - exceeds bar b by at least 50 x."""
    plain = Case("emulation", "", 0, shape, {}, bias=False, a_lo=kind == "f32")
    for family in (("a", "b", "c") if kind == "f32" else D):
        o = inputs(shape, family, kind)
        judge(emulate(o, a_lo=plain.a_lo), o, plain, family, f"emulation {shape} {kind}")
        if family == "b":
            ref, err32 = expected(o, plain)
            broken = emulate(o, a_lo=plain.a_lo, drop="x_lo w_hi" if plain.a_lo else "x_hi w_lo")
            over = ((broken.double() - ref).abs() / (o.lolo + 4 * err32 + 1e-6)).min().item()
            print(f"GEMMFORM emulation {shape} {kind}: a dropped cross term is at least {over:.0f} x bar b on EVERY element")
            assert over >= 50, over


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


class Output:
    """y inside a [rows + 1][n_out + 4] buffer: NaN everywhere, or a random y0 (pads included) under accumulate"""

    def __init__(self, M, N, y0=None):
        self.M, self.N, self.ld = M, N, N + 4
        self.buf = torch.full((M + 1, self.ld), NAN, device=DEV)
        if y0 is not None:
            self.buf.copy_(torch.randn(M + 1, self.ld, generator=torch.Generator().manual_seed(M + N)))
            self.buf[:M, :N] = y0.to(DEV)
        self.before = self.buf.clone()

    @property
    def y(self):
        return self.buf[:self.M, :self.N]

    def pads_untouched(self):
        a, b = self.buf.view(torch.int32), self.before.view(torch.int32)
        return bool((a[:, self.N:] == b[:, self.N:]).all() and (a[self.M] == b[self.M]).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == self.before.view(torch.int32)).all())


def probe(op, out, M, N, K, *, a, lda, a_lo=None, b=None, b_hi=None, b_lo=None, ldb=None, bias=None, accumulate=False, precision=0,
          scratch=None, a_index=None, rows=(0, -1, 0), row_scale=None, b_scale=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    args = _lib.DrinGemmProbeArgsC(
        struct_size=C.sizeof(_lib.DrinGemmProbeArgsC), op=op, precision=precision, accumulate=int(accumulate), row_tile_begin=rows[0],
        row_tile_end=rows[1], row_tile_wgs=rows[2], a=ptr(a), a_lo=ptr(a_lo), lda=lda, b=ptr(b), b_hi=ptr(b_hi), b_lo=ptr(b_lo), ldb=ldb,
        bias=ptr(bias), y=out.buf.data_ptr(), ldy=out.ld, rows=M, n_out=N, k=K, scratch=None if scratch is None else scratch.buf.data_ptr(),
        scratch_floats=0 if scratch is None else scratch.floats, a_index=ptr(a_index), row_scale=ptr(row_scale), b_scale=ptr(b_scale))
    rc = _lib.load().drin_gemm_probe(C.byref(args), stream())
    return rc, args.route


def assert_route(route, want, label):
    got = {k: (_lib.GEMM_FAMILY[route.family] if k == "family" else getattr(route, k)) for k in want}
    assert got == want, f"{label}: the dispatch code took {got}, the case is there for {want}: move the shape"
    assert route.launches == 1, label


class Device:
    """the operands of one case on the GPU, in the layouts the case asks for"""

    def __init__(self, case, o):
        M, N, K = case.shape
        self.ldx, self.ldw = (K + 8, K + 16) if case.strided else (K, K)
        self.index = None
        x, planes_x = o.x, o.planes["x"]
        if case.indexed:
            # rows through a_index: a permutation of a larger table with every 7th entry repeating its neighbour; the rows of the
            # table that the index does not name hold NaN
            gen = torch.Generator().manual_seed(M)
            T = M + 64
            index = torch.randperm(T, generator=gen)[:M]
            self.src = torch.arange(M)
            self.src[1::7] = self.src[0::7][:len(self.src[1::7])]
            index[1::7] = index[0::7][:len(index[1::7])]
            table = torch.full((T, K), NAN)
            table[index] = x[self.src]
            x, self.index = table, index.to(DEV)
        self.x = padded(x, self.ldx)
        self.w = padded(o.w, self.ldw) if case.weights == "f32" or case.op == NT else None
        self.bias = o.bias.to(DEV) if case.bias else None
        self.w_hi = self.w_lo = self.x_hi = self.x_lo = self.nt_planes = None
        if case.weights == "planes":
            if case.op == NT:   # launch_gemm_nt: [N][K] hi followed by [N][K] lo in one buffer, contiguous weights only
                self.nt_planes = torch.cat([p.reshape(-1) for p in o.planes["w"]]).to(DEV)
            else:
                self.w_hi, self.w_lo = (padded(p, self.ldw) for p in o.planes["w"])
        if case.op == PL:
            self.x_hi = padded(planes_x[0], self.ldx)
            self.x_lo = padded(planes_x[1], self.ldx) if case.a_lo else None

    def run(self, case, out, scratch, rows=(0, -1, 0), a_lo="case"):
        M, N, K = case.shape
        common = dict(lda=self.ldx, ldb=self.ldw, bias=self.bias, accumulate=case.accumulate, scratch=scratch, rows=rows)
        if case.op == NT:
            return probe(NT, out, M, N, K, a=self.x, b=self.w, b_hi=self.nt_planes, precision=_lib.PREC_BF16X3_ALL, **common)
        if case.op == X3:
            return probe(X3, out, M, N, K, a=self.x, b=self.w, b_hi=self.w_hi, b_lo=self.w_lo, a_index=self.index, **common)
        if case.op == P4:
            return probe(P4, out, M, N, K, a=self.x, b_hi=self.w_hi, b_lo=self.w_lo, **common)
        return probe(PL, out, M, N, K, a=self.x_hi, a_lo=self.x_lo if a_lo == "case" else a_lo, b_hi=self.w_hi, b_lo=self.w_lo, **common)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family", [(c.name, f) for c, f in RUNS])
def test_form_against_fp64(name, family):
    case = BY_NAME[name]
    M, N, K = case.shape
    o = inputs(case.shape, family, case.kind)
    dev = Device(case, o)
    out = Output(M, N, o.y0 if case.accumulate else None)
    scratch = Scratch(case.scratch) if case.scratch else None
    rc, route = dev.run(case, out, scratch)
    assert rc == _lib.OK, _lib.load().drin_last_error()
    assert_route(route, case.route, name)
    y = out.y.cpu()
    assert bool(torch.isfinite(y).all()), f"{name}: elements of the product were not written"
    assert out.pads_untouched(), f"{name}: a pad column or the spare row changed"
    assert scratch is None or scratch.intact(), f"{name}: wrote behind the scratch"
    if case.indexed:
        o = Operands(o.x[dev.src], o.w, o.bias, o.y0, o.ref[dev.src], o.scale[dev.src], None if o.lolo is None else o.lolo[dev.src],
                     o.prod32[dev.src])
    judge(y, o, case, family, name)


# fp16 one-pass form ------------------------------------------------------------------------------------------------------------
def pow2_scale(max_abs):
    """the smallest power of two >= max_abs: max_abs / scale in (0.5, 1]"""
    return torch.exp2(torch.ceil(torch.log2(max_abs)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,scratch_floats,want", [
    ((10958, 768, 64), None, r("planes_p4", a_lo=1, f16=1, persist=0, tiles=129, whole_tiles=129, ksplit=1)),
    ((21966, 768, 512), BIG, r("planes_p4", a_lo=1, f16=1, persist=0, tiles=258, whole_tiles=256, ksplit=2))],
    ids=["f16_p4", "f16_p4_tail2"])
def test_fp16_one_pass_form(shape, scratch_floats, want):
    """`k_gemm_x3_planes_p4<true, true>`: rows scaled by powers of two from 2^-20 to 2^20 (their scale per row), weights of
    magnitude 1e-5 (so that the single weight scale matters: unscaled they would be fp16 subnormals)."""
    M, N, K = shape
    gen = torch.Generator().manual_seed(M + K)
    e = torch.randint(-20, 21, (M,), generator=gen).float()
    e[:41] = torch.arange(-20, 21).float()                              # every power from 2^-20 to 2^20 is there
    x = torch.randn(M, K, generator=gen) * torch.exp2(e)[:, None]
    w = torch.randn(N, K, generator=gen) * 1e-5
    row_scale = pow2_scale(x.abs().max(dim=1).values)
    a16 = (x / row_scale[:, None]).half()
    w_scale = pow2_scale(w.abs().max())
    b16_want = (w / w_scale).half()
    # the weight plane by the library's own launch_to_f16_scaled: the quantisation stated above, bit for bit
    wd = w.to(DEV)
    b16 = torch.full((N, K), NAN, dtype=torch.float16, device=DEV)
    scale2 = torch.full((2 + GUARD,), 12345.0, device=DEV)
    args = _lib.DrinGemmProbeArgsC(struct_size=C.sizeof(_lib.DrinGemmProbeArgsC), op=_lib.PROBE_TO_F16_SCALED, a=wd.data_ptr(),
                                   y=b16.data_ptr(), rows=N * K, scratch=scale2.data_ptr(), scratch_floats=2)
    _lib.check(_lib.load().drin_gemm_probe(C.byref(args), stream()))
    assert scale2[0].item() == w_scale.item() and bool((scale2[2:] == 12345.0).all())
    assert torch.equal(b16.cpu(), b16_want)

    out = Output(M, N)
    scratch = Scratch(scratch_floats) if scratch_floats else None
    rc, route = probe(F16, out, M, N, K, a=a16.to(DEV), lda=K, b_hi=b16, ldb=K, row_scale=row_scale.to(DEV), b_scale=scale2[:1],
                      scratch=scratch)
    assert rc == _lib.OK, _lib.load().drin_last_error()
    assert_route(route, want, "fp16 one pass")
    y = out.y.cpu()
    assert bool(torch.isfinite(y).all()) and out.pads_untouched() and (scratch is None or scratch.intact())
    # before the scales: y / (row_scale w_scale) is exact (powers of two, nothing near the subnormals)
    unscaled = y.double() / (row_scale.double()[:, None] * w_scale.double())
    ref = a16.double() @ b16_want.double().t()
    err32 = ((a16.float() @ b16_want.float().t()).double() - ref).abs().max().item()
    err = (unscaled - ref).abs().max().item()
    print(f"GEMMFORM fp16 one pass {shape}: max err = {err:.2e} on products of magnitude {ref.abs().max().item():.2f} "
          f"(bar 4 * {err32:.2e} + 1e-6 = {4 * err32 + 1e-6:.2e})")
    assert err <= 4 * err32 + 1e-6
    # and the scaled output is the unscaled one times the scales, per row, over all 41 powers
    assert torch.equal(y.double(), unscaled * (row_scale.double()[:, None] * w_scale.double()))


# slices of row tiles and the persistent grid -------------------------------------------------------------------------------------
SLICE_CASES = {
    # 6 row tiles x 3
    "bf16x3_p4": Case("slices_p4", "", P4, (1499, 768, 96), r("bf16x3_p4", persist=0, tiles=18, whole_tiles=18, ksplit=1), weights="planes"),
    # launch_gemm_x3_planes takes the four-phase kernel for an activation without a lo plane from 128 tiles up (at (1499, 768, 96)
    # it is the two-phase kernel, which has no slices: asserted below), so this family's slices run at the smallest listed shape
    # that selects k_gemm_x3_planes_p4<false, false, .>: 43 row tiles x 3
    "planes_p4": Case("slices_planes_p4", "", PL, (10958, 768, 64), r("planes_p4", a_lo=0, persist=0, tiles=129, whole_tiles=129, ksplit=1),
                      weights="planes", a_lo=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(SLICE_CASES))
def test_row_tile_slices_and_persistent_grid(fam):
    """Row tiles [0, S) as G persistent workgroups + [S, end) plain == one launch, bit for bit, for S in {1, 3, 5} and G in
    {1, 3, 8, 64} (more workgroups than the slice has tiles; not a multiple of 8); the one launch is inside the fp64 bar; a slice
    alone leaves every row outside it NaN."""
    case = SLICE_CASES[fam]
    M, N, K = case.shape
    nx, row_tiles = -(-N // 256), -(-M // 256)
    o = inputs(case.shape, "a" if case.a_lo else "d", case.kind)
    dev = Device(case, o)
    single = Output(M, N)
    rc, route = dev.run(case, single, None)
    assert rc == _lib.OK, _lib.load().drin_last_error()
    assert_route(route, case.route, case.name)
    judge(single.y.cpu(), o, case, "a" if case.a_lo else "d", case.name)
    for S in (1, 3, 5):
        for G in (1, 3, 8, 64):
            out = Output(M, N)
            rc, route = dev.run(case, out, None, rows=(0, S, G))
            assert rc == _lib.OK, _lib.load().drin_last_error()
            assert_route(route, dict(case.route, persist=1, whole_tiles=S * nx, tile0=0, work_items=G), f"{fam} S={S} G={G} persistent")
            assert bool(torch.isfinite(out.y[:S * 256]).all()) and bool(torch.isnan(out.buf[S * 256:]).all()), (S, G)
            assert torch.equal(out.y[:S * 256], single.y[:S * 256]), (S, G)
            rc, route = dev.run(case, out, None, rows=(S, -1, 0))
            assert rc == _lib.OK, _lib.load().drin_last_error()
            assert_route(route, dict(case.route, whole_tiles=(row_tiles - S) * nx, tile0=S * nx), f"{fam} S={S} plain rest")
            assert torch.equal(out.y, single.y) and out.pads_untouched(), (S, G)
        alone = Output(M, N)                                            # the plain slice alone: the rows before it stay NaN
        rc, _ = dev.run(case, alone, None, rows=(S, row_tiles, 0))
        assert rc == _lib.OK
        assert bool(torch.isnan(alone.buf[:S * 256]).all()) and torch.equal(alone.y[S * 256:], single.y[S * 256:])
    inner = Output(M, N)                                                # a slice in the middle, persistent
    rc, _ = dev.run(case, inner, None, rows=(2, 4, 3))
    assert rc == _lib.OK
    assert bool(torch.isnan(inner.buf[:512]).all()) and bool(torch.isnan(inner.buf[1024:]).all())
    assert torch.equal(inner.y[512:1024], single.y[512:1024])


@pytest.mark.gpu
def test_two_phase_planes_kernel_has_no_slices():
    """(1499, 768, 96) without a lo plane is 18 tiles: below the four-phase gate of launch_gemm_x3_planes, whose two-phase kernel
    refuses a slice of row tiles and writes nothing."""
    case = Case("no_slices", "", PL, (1499, 768, 96), {}, weights="planes", a_lo=False)
    dev = Device(case, inputs(case.shape, "d", "bf16"))
    out = Output(*case.shape[:2])
    rc, route = dev.run(case, out, None, rows=(0, 3, 8))
    assert rc == _lib.E_UNSUPPORTED and route.launches == 0 and out.untouched()
    rc, route = dev.run(case, out, None)
    assert rc == _lib.OK
    assert_route(route, r("planes", a_lo=0, splits=1, ksplit=1, tiles=18), "unsliced")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["bf16x3_p4", "planes_p4"])
def test_slices_next_to_a_tail_split(fam):
    """(7324, 2052, 512) + scratch: 29 row tiles x 9 = 261 tiles, 256 whole and 5 as four K-slices each.  A persistent slice inside
    the whole tiles + the plain rest (which carries the tail split) == the one launch; a persistent slice that would reach the tail,
    or one with a lo plane of the activation, is refused and writes nothing."""
    shape = (7324, 2052, 512)
    if fam == "bf16x3_p4":
        case = Case("tail_slices_p4", "", P4, shape, r("bf16x3_p4", persist=0, tiles=261, whole_tiles=256, ksplit=4), weights="planes", scratch=BIG)
    else:
        case = Case("tail_slices_planes_p4", "", PL, shape, r("planes_p4", a_lo=0, persist=0, tiles=261, whole_tiles=256, ksplit=4),
                    weights="planes", a_lo=False, scratch=BIG)
    M, N, K = shape
    o = inputs(shape, "a" if case.a_lo else "d", case.kind)
    dev = Device(case, o)
    scratch = Scratch(BIG)
    single = Output(M, N)
    rc, route = dev.run(case, single, scratch)
    assert rc == _lib.OK, _lib.load().drin_last_error()
    assert_route(route, case.route, case.name)
    judge(single.y.cpu(), o, case, "a" if case.a_lo else "d", case.name)
    for S, G in ((28, 64), (11, 3)):                                    # 28: all the row tiles that hold whole tiles only
        out = Output(M, N)
        rc, route = dev.run(case, out, scratch, rows=(0, S, G))
        assert rc == _lib.OK, _lib.load().drin_last_error()
        assert_route(route, dict(case.route, persist=1, whole_tiles=9 * S, tile0=0, ksplit=1, work_items=G), f"{fam} persistent [0, {S})")
        assert bool(torch.isnan(out.buf[S * 256:]).all())
        rc, route = dev.run(case, out, scratch, rows=(S, -1, 0))
        assert rc == _lib.OK, _lib.load().drin_last_error()
        assert_route(route, dict(case.route, whole_tiles=256 - 9 * S, tile0=9 * S, ksplit=4), f"{fam} plain rest with the tail")
        assert torch.equal(out.y, single.y) and out.pads_untouched() and scratch.intact(), (S, G)
    for rows in ((28, -1, 8), (0, -1, 64), (0, 29, 64)):                 # would reach the tail
        out = Output(M, N)
        rc, route = dev.run(case, out, scratch, rows=rows)
        assert rc == _lib.E_UNSUPPORTED and route.launches == 0 and out.untouched(), rows
    if fam == "planes_p4":                                              # the persistent grid is built without a lo plane
        out = Output(M, N)
        rc, route = dev.run(case, out, scratch, rows=(0, 11, 8), a_lo=padded(o.planes["x"][1], dev.ldx))
        assert rc == _lib.E_UNSUPPORTED and route.launches == 0 and out.untouched()
        assert b"persistent" in _lib.load().drin_last_error()
