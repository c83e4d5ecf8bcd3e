"""-m gpu: the four kernel groups that close every training step, each alone through its C entry point (outputs and scratch
filled with NaN first) against a plain reference, at the sizes where their loops, tails and clamps change course:
`drin_triplet_topk` against the integer hinge counts of tests/step_restatement.py, `drin_adam_step` against torch.optim.Adam
bit for bit, `drin_cosine_rows_fwd` / `_bwd` against fp64 autograd row by row, `drin_entity_token_mean` (fp32) against the
fp64 oracle.  DESIGN.md section 26 lists which case covers which boundary; every test prints its measured maxima and
profiles/step_kernels_parity.txt records them."""
import ctypes as C

import numpy as np
import pytest
import torch

from drin_amd import _lib, row_ops, synth
from drin_amd.config import DrinConfig
from drin_amd.metrics import DeviceLossMetric, TripletLoss
from drin_amd.model import Model, _param_list
from drin_amd.train import LibraryAdam
from oracle import drin_oracle as O
from oracle.cases import TINY
from tests.helpers import check_cosine, cos_bwd, cos_case, cos_fwd, rows_ratio
from tests.step_restatement import cosine_rows64_grads, triplet_counts

pytestmark = pytest.mark.gpu

DEV = "cuda"
KERNEL_TOL = 1e-5                                                     # fp32-FMA kernels, DESIGN.md section 16
NAN = float("nan")
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)                      # noqa: E731  (NaN positions count)


# ---- drin_triplet_topk ----------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(5, 256), (5, 257), (5, 258), (3, 514), (4, 1001),      # trips of 256 candidate threads: C = 255, 256, 257, 513, 1000
               (4, 64), (4, 65), (4, 66),                             # the 64-lane row walk: C = 63, 64, 65
               (12, 7), (13, 7), (14, 7), (15, 7), (16, 7), (17, 7), (29, 7),   # the 4-row unroll (bb + 12 < B) per wave
               (4096, 5), (4097, 5),                                  # the refill of the 4096 positive distances in LDS
               (1, 2)]
VARIANT_SHAPES = [(13, 66), (5, 258)]
VARIANTS = ["one-hot", "two golds", "weight 3", "empty row", "tie at k", "nan gold", "+inf"]


def loss_case(B, N, kind, seed, variant="one-hot"):
    """(y uint8 [B, N-1], yhat fp32 [B, N]) on the host.  kind "grid": multiples of 1/64 in [-1, 1] - with a margin that is one
    too, every pos - p + margin is exact in fp32 and many are 0; kind "float": normal deviates."""
    g = torch.Generator().manual_seed(seed)
    C_ = N - 1
    yhat = torch.randint(-64, 65, (B, N), generator=g).float() / 64 if kind == "grid" else torch.randn(B, N, generator=g)
    gold = torch.randint(0, C_, (B,), generator=g)
    y = torch.zeros(B, C_, dtype=torch.uint8)
    y[torch.arange(B), gold] = 1
    r = B // 2                                                        # the row a variant changes
    if variant == "two golds":
        y[r, (int(gold[r]) + 64) % C_] = 1                            # 64 apart where the row is long enough: one lane of k_triplet_rows
        y[0, (int(gold[0]) + 1) % C_] = 1
    elif variant == "weight 3":
        y[r, gold[r]] = 3
    elif variant == "empty row":
        y[r] = 0
    elif variant == "tie at k":
        yhat[r, gold[r]] = yhat[r, :C_].max() + 0.5                    # the gold above its whole row, four scores equal to it
        for j in (1, 2, 3, 4):                                        # and one higher: inside the top k from k = 2 on - from k = 6
            yhat[r, (int(gold[r]) + j) % C_] = yhat[r, gold[r]]       # if a tie counted against it
        yhat[r, (int(gold[r]) + 5) % C_] = yhat[r, gold[r]] + 1.0
    elif variant == "nan gold":
        yhat[r, gold[r]] = NAN
    elif variant == "+inf":
        yhat[r, (int(gold[r]) + 1) % C_] = float("inf")               # beside the gold: 0 * inf makes this row's pos NaN
        yhat[0, gold[0]] = float("inf")                               # the gold itself: pos = -inf
    return y, yhat


def triplet_raw(y, yhat, margin, ks, want_grad=True, correct=None):
    lib = _lib.load()
    B, N = yhat.shape
    loss = torch.full((1,), NAN, device=DEV)
    d = torch.full_like(yhat, NAN) if want_grad else None
    nbytes = lib.drin_loss_workspace_bytes(B)
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    if correct is None and ks:
        correct = torch.zeros(len(ks), dtype=torch.int64, device=DEV)
    arr = (C.c_int32 * len(ks))(*ks) if ks else None
    _lib.check(lib.drin_triplet_topk(ptr(yhat), ptr(y), B, N, margin, arr, len(ks), ptr(loss), ptr(d), ptr(correct) if ks else None,
                                     ptr(ws), nbytes, stream()))
    return loss, d, correct


def check_loss(y, yhat, margin, ks, kind, tag):
    """The raw call and DeviceLossMetric against the restatement; returns what the raw call gave."""
    B, N = yhat.shape
    yd, sd = y.to(DEV), yhat.to(DEV)
    exact = triplet_counts(yd, sd, margin, ks)                          # fp64
    # the hinge mask of fp32 scores is the one fp32 arithmetic gives; on the grid both are the same and exact
    ref = exact if kind == "grid" else triplet_counts(yd, sd, margin, ks, dtype=torch.float32)
    loss, d, correct = triplet_raw(yd, sd, margin, ks)
    scale32 = float(np.float32(ref.scale))
    assert not torch.isnan(d).any(), tag
    got = torch.round(d.double() / scale32).to(torch.int64)
    wrong = int((got != ref.counts).sum())
    ref_grad = ref.counts.double() * ref.scale
    gmax = ref_grad.abs().max().item()
    gerr = (d.double() - ref_grad).abs().max().item()
    want_loss = exact.loss.item()
    lerr = abs(loss.item() - want_loss) if np.isfinite(want_loss) else 0.0
    print(f"{tag}: loss {loss.item():.9g} ref {want_loss:.9g} err {lerr:.2e}; counts differing {wrong} of {B * N} "
          f"(max |count| {int(ref.counts.abs().max())}); grad err {gerr:.2e} of max {gmax:.2e}; hits {correct.tolist() if ks else []}")
    if np.isfinite(want_loss):
        assert lerr <= 3e-7 * max(1.0, abs(want_loss)), tag
    else:
        assert np.array_equal(np.float64(loss.item()), np.float64(want_loss), equal_nan=True), tag
    assert wrong == 0, tag
    np.testing.assert_allclose(d.cpu().numpy(), ref_grad.cpu().numpy(), atol=2e-7 * gmax + 1e-12, rtol=2e-6, err_msg=tag)
    assert torch.count_nonzero(d[:, -1]).item() == 0, tag               # the answer slot: exactly 0
    if ks:
        assert correct.tolist() == ref.hits.tolist(), tag
    # the same numbers through the class the training loop uses
    m = DeviceLossMetric(margin, ks, DEV)
    leaf = sd.clone().requires_grad_(True)
    out = m(yd, leaf)
    out.backward()
    assert torch.equal(bits(out.detach().reshape(1)), bits(loss)) and torch.equal(bits(leaf.grad), bits(d)), tag
    assert m.correct.tolist() == ref.hits.tolist() and m.total == B, tag
    return loss, d, ref


def shape_ks(N):
    return sorted({k for k in (1, 2, 3, 5, 10, 50, N - 1) if k <= N - 1})


@pytest.mark.parametrize("kind", ["grid", "float"])
@pytest.mark.parametrize("B,N", LOSS_SHAPES)
def test_triplet_topk_at_every_loop_boundary(B, N, kind):
    y, yhat = loss_case(B, N, kind, 1000 * B + N)
    check_loss(y, yhat, 0.25, shape_ks(N), kind, f"triplet {kind} ({B},{N})")


@pytest.mark.parametrize("kind", ["grid", "float"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N", VARIANT_SHAPES)
def test_triplet_topk_answers_that_are_not_one_hot(B, N, variant, kind):
    """Any uint8 weight, several golds, none; a tie with the k-th score; NaN and +inf scores - with eight k at once, unsorted,
    1 and N - 1 among them."""
    y, yhat = loss_case(B, N, kind, 77 * B + N, variant)
    ks = [7, 1, N - 1, 2, 64, 3, 20, 5]
    check_loss(y, yhat, 0.25, ks, kind, f"triplet {kind} ({B},{N}) {variant}")


@pytest.mark.parametrize("kind", ["grid", "float"])
@pytest.mark.parametrize("margin", [0.0, 0.25, -0.5])
@pytest.mark.parametrize("B,N", VARIANT_SHAPES)
def test_triplet_topk_margins_counters_and_null_gradient(B, N, margin, kind):
    y, yhat = loss_case(B, N, kind, 5 * B + N)
    ks = [3, 1, N - 1]
    loss, d, ref = check_loss(y, yhat, margin, ks, kind, f"triplet {kind} ({B},{N}) margin {margin}")
    yd, sd = y.to(DEV), yhat.to(DEV)
    # d_scores = NULL: the same loss bits, and no top-k list: nothing is counted
    only, none, _ = triplet_raw(yd, sd, margin, [], want_grad=False)
    assert none is None and torch.equal(bits(only), bits(loss))
    # a second call accumulates into `correct`; count=False passes no counter buffer and leaves it alone
    y2, yhat2 = loss_case(B, N, kind, 6 * B + N, "two golds")
    hits2 = triplet_counts(y2, yhat2, margin, ks).hits
    correct = torch.tensor([11, 22, 33], dtype=torch.int64, device=DEV)
    triplet_raw(yd, sd, margin, ks, correct=correct)
    triplet_raw(y2.to(DEV), yhat2.to(DEV), margin, ks, correct=correct)
    assert correct.tolist() == (torch.tensor([11, 22, 33]) + ref.hits + hits2).tolist()
    m = DeviceLossMetric(margin, ks, DEV)
    m(yd, sd)
    m(y2.to(DEV), yhat2.to(DEV))
    assert m.correct.tolist() == (ref.hits + hits2).tolist() and m.total == 2 * B
    quiet = m(yd, sd, count=False)
    assert m.correct.tolist() == (ref.hits + hits2).tolist() and m.total == 2 * B
    assert torch.equal(bits(quiet.reshape(1)), bits(loss))
    print(f"triplet {kind} ({B},{N}) margin {margin}: counters {correct.tolist()} after two calls from [11, 22, 33]")


# ---- drin_adam_step -------------------------------------------------------------------------------------------------------
def adam_call(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, n=None):
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** float(t), 1 - b2 ** float(t)                  # torch/optim/adam.py, python doubles
    scal = (1 - b1, b2, 1 - b2, bc2 ** 0.5, eps, (lr / bc1) * -1)
    return _lib.load().drin_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel() if n is None else n, *(C.c_float(x) for x in scal), stream())


def adam_values(n, seed, steps):
    g = torch.Generator().manual_seed(seed)
    spread = lambda lo, hi: torch.logspace(lo, hi, n)[torch.randperm(n, generator=g)]   # noqa: E731
    p0 = torch.randn(n, generator=g) * spread(-6, 2)
    grads = [torch.randn(n, generator=g) * spread(-8, 1) for _ in range(steps)]
    return p0.to(DEV), [x.to(DEV) for x in grads]


def adam_against_torch(p0, grads, lr, betas, eps, steps, tag):
    """One step per gradient, numbered by `steps`, of the entry point and of torch.optim.Adam from the same state; param and
    both moments bit for bit after every step.  A step number that does not follow the one before is written into torch's
    state, not run up to.  Returns the final (param, exp_avg, exp_avg_sq) of the entry point."""
    n = p0.numel()
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=lr, betas=betas, eps=eps)
    assert opt.defaults.get("foreach") is None and not opt.defaults.get("fused")     # the default: multi-tensor on the device
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    worst = 0
    for t, gr in zip(steps, grads):
        ref.grad = gr.clone()
        if ref in opt.state and int(opt.state[ref]["step"]) != t - 1:
            opt.state[ref]["step"].fill_(t - 1)
        opt.step()
        st = opt.state[ref]
        assert int(st["step"]) == t
        _lib.check(adam_call(p, gr, m, v, t, lr, betas, eps))
        for name, mine, theirs in (("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"]), ("param", p, ref.data)):
            diff = int((bits(mine) != bits(theirs)).sum())
            worst = max(worst, diff)
            assert diff == 0, f"{tag} step {t}: {name} differs in {diff} of {n} elements"
    print(f"{tag}: steps {list(steps)[:len(grads)]}, {n} elements, bit differences {worst}")
    return p, m, v


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2_097_152, 2_097_152 + 1024 + 3])
def test_adam_sizes_tail_only_to_second_stride_trip(n):
    """n < 4: no float4 at all; 2 097 152 fills the 2048-block grid exactly once, 1024 + 3 more is a second trip and a tail."""
    p0, grads = adam_values(n, 5 + n % 1000, 3)
    adam_against_torch(p0, grads, 1e-3, (0.9, 0.999), 1e-8, (1, 2, 3), f"adam n={n}")


@pytest.mark.parametrize("betas", [(0.8, 0.99), (0.51, 0.9)])
def test_adam_other_hyper_parameters(betas):
    """Other betas (1 - 0.51 is just inside the lerp form that is built), eps and lr, at step 1 and - on the moments that step
    left - at step 1000, where the bias corrections are 1 - 2e-97 and 0.99996 or 1."""
    p0, grads = adam_values(1025, 9, 3)
    adam_against_torch(p0, grads, 3e-4, betas, 1e-6, (1, 1000, 1001), f"adam betas={betas} eps=1e-6 lr=3e-4")


@pytest.mark.parametrize("special", [0.0, 1e-30, 1e20, NAN, -0.0], ids=["zero", "1e-30", "1e20", "nan", "-zero"])
def test_adam_special_gradients_keep_to_their_slot(special):
    """g = 0 on zero moments (0 / eps), g^2 underflowing, g^2 overflowing, NaN and -0: once inside a float4 between ordinary
    neighbours and once in the middle of the three-element tail; torch's bits at the slot, and the neighbours' bits are those
    of a run with an ordinary value there."""
    n = 43                                                            # ten float4 and a tail of three
    slots = [5, 41]
    p0, grads = adam_values(n, 21, 3)
    plain = adam_against_torch(p0, grads, 1e-3, (0.9, 0.999), 1e-8, (1, 2, 3), "adam ordinary")
    grads[0] = grads[0].clone()
    grads[0][slots] = special
    got = adam_against_torch(p0, grads, 1e-3, (0.9, 0.999), 1e-8, (1, 2, 3), f"adam special {special!r}")
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[slots] = False
    for a, b in zip(got, plain):
        assert torch.equal(bits(a)[others], bits(b)[others])
    print(f"adam special {special!r}: slots {slots} param {got[0][slots].tolist()} exp_avg {got[1][slots].tolist()} exp_avg_sq {got[2][slots].tolist()}")


def test_adam_refusals_leave_every_buffer_alone():
    p0, grads = adam_values(64, 3, 1)
    bufs = [p0.clone(), grads[0].clone(), torch.full((64,), 0.25, device=DEV), torch.full((64,), 0.5, device=DEV)]
    before = [b.clone() for b in bufs]
    lib = _lib.load()
    args = [C.c_float(x) for x in (0.999, 0.001, 1.0, 1e-8, -1e-3)]
    assert lib.drin_adam_step(*(ptr(b) for b in bufs), 64, C.c_float(0.5), *args, stream()) == _lib.E_UNSUPPORTED   # beta1 = 0.5 exactly
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(bufs, before))
    for k in range(4):                                                 # each operand in turn 4 bytes off a 16-byte boundary
        ptrs = [C.c_void_p(b.data_ptr() + (4 if i == k else 0)) for i, b in enumerate(bufs)]
        assert lib.drin_adam_step(*ptrs, 8, C.c_float(0.1), *args, stream()) == _lib.E_ALIGN, k
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(bufs, before))


def test_library_adam_with_its_own_betas_eps_and_a_rewritten_lr():
    """LibraryAdam(betas=(0.8, 0.99), eps=1e-6) on a TINY model against torch.optim.Adam on a twin: parameters and moments bit
    for bit over three steps, and over a fourth after a scheduler's write of param_groups[0]["lr"]."""
    cfg = DrinConfig(**TINY)
    sd = synth.make_state_dict(cfg, 8)
    batch = [t.to(DEV) for t in synth.make_batch(cfg, 16, 31)]
    a, b = (Model(cfg, precision="f32").to(DEV) for _ in range(2))
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    oa = LibraryAdam(a, lr=1e-3, betas=(0.8, 0.99), eps=1e-6)
    ob = torch.optim.Adam(b.parameters(), lr=1e-3, betas=(0.8, 0.99), eps=1e-6)
    loss_fn = TripletLoss(cfg.triplet_margin)
    for step in range(1, 5):
        if step == 4:
            oa.param_groups[0]["lr"] = 2.5e-4
            ob.param_groups[0]["lr"] = 2.5e-4
        for model, opt in ((a, oa), (b, ob)):
            opt.zero_grad(set_to_none=True)
            loss_fn(batch[14], model(batch[:14])).backward()
            opt.step()
        offsets, live, _total = a.bucket_layout()
        checked = 0
        for off, pa, pb in zip(offsets, _param_list(a), _param_list(b)):
            assert torch.equal(bits(pa.detach()), bits(pb.detach())), step
            if off < live and pb in ob.state:
                n = pa.numel()
                assert torch.equal(bits(oa.exp_avg[off:off + n]), bits(ob.state[pb]["exp_avg"].flatten())), step
                assert torch.equal(bits(oa.exp_avg_sq[off:off + n]), bits(ob.state[pb]["exp_avg_sq"].flatten())), step
                checked += n
        assert checked > 0 and oa.t == step and oa.lr == ob.param_groups[0]["lr"]
    assert oa.one_launch_steps == 4
    moved = max((pa.detach() - sd[k].to(DEV)).abs().max().item() for k, pa in a.named_parameters())
    print(f"LibraryAdam betas (0.8, 0.99) eps 1e-6: 4 steps bit for bit over {checked} elements, largest parameter move {moved:.3e}")


# ---- drin_cosine_rows_fwd / _bwd, row_ops.cosine_rows -----------------------------------------------------------------------
COS_SHAPES = [(1, 1, 4), (5, 3, 4), (1, 4, 252), (5, 5, 252), (1, 3, 256), (5, 101, 256), (1, 1, 260), (5, 4, 260), (1, 101, 512),
              (5, 5, 512), (1, 4, 516), (5, 3, 516), (1, 5, 768), (5, 101, 768), (1, 3, 772), (5, 1, 772), (1, 101, 1024), (5, 4, 1024),
              (5, 5, 1024), (5, 3, 768)]                              # D4 = 1, 63, 64, 65, 128, 129, 192, 193, 256; every N of {1, 3, 4, 5, 101}


@pytest.mark.parametrize("B,N,D", COS_SHAPES)
def test_cosine_rows_forward_and_backward_per_row(B, N, D):
    x, y, dout = cos_case(B, N, D, 13 * D + 7 * N + B)
    check_cosine(x, y, dout, 1e-8, f"cosine ({B},{N},{D})")


def test_cosine_rows_width_limit():
    """D = 1028: one float4 more than the backward keeps in registers - refused there, while the forward has no such limit."""
    x, y, dout = cos_case(2, 3, 1028, 1)
    out64, _, _ = cosine_rows64_grads(x, y, dout, 1e-8)
    out = cos_fwd(x.to(DEV), y.to(DEV), 1e-8)
    ferr = (out.double().cpu() - out64).abs().max().item()
    print(f"cosine (2,3,1028): forward max err {ferr:.2e} of max |ref| {out64.abs().max().item():.2e}")
    assert ferr <= KERNEL_TOL * out64.abs().max().item()
    status, dx, dy = cos_bwd(x.to(DEV), y.to(DEV), dout.to(DEV), 1e-8)
    torch.cuda.synchronize()
    assert status == _lib.E_UNSUPPORTED and torch.isnan(dx).all() and torch.isnan(dy).all()
    with pytest.raises(_lib.DrinError):
        xl = x.to(DEV).requires_grad_(True)
        row_ops.cosine_rows(xl, y.to(DEV), 1e-8).sum().backward()


def unit_rows(t):
    return t / torch.linalg.vector_norm(t, dim=-1, keepdim=True)


@pytest.mark.parametrize("D", [260, 768])
def test_cosine_rows_clamp_at_default_eps(D):
    """eps = 1e-8: an all-zero mention row, one of norm 1e-9, an all-zero candidate row, one of norm 1e-9, and pairs that have
    both - beside ordinary rows.  A clamped norm makes gradients of order 1 / eps, which is why the bar is per row."""
    B, N = 5, 5
    x, y, dout = cos_case(B, N, D, 40 + D)
    dout = torch.where(dout == 0, torch.ones(()), dout)
    dout[4, 0] = 0.0
    x[1] = 0.0
    x[2] = unit_rows(x[2]) * 1e-9
    y[0, 1] = 0.0                                                      # ordinary mention, zero candidate
    y[3, 2] = unit_rows(y[3, 2]) * 1e-9                                # ordinary mention, sub-eps candidate
    y[1, 3] = 0.0                                                      # zero mention and zero candidate
    y[2, 0] = unit_rows(y[2, 0]) * 1e-9                                # sub-eps mention and sub-eps candidate
    y[1, 4] = unit_rows(y[1, 4]) * 1e-9                                # zero mention, sub-eps candidate
    y[2, 2] = 0.0                                                      # sub-eps mention, zero candidate
    out, dx, dy = check_cosine(x, y, dout, 1e-8, f"cosine clamp eps=1e-8 D={D}")
    assert torch.count_nonzero(out[1]).item() == 0 and out[0, 1].item() == 0.0
    assert torch.count_nonzero(dy[1, 3]).item() == 0 and dy[0, 1].abs().max().item() > 1e6


@pytest.mark.parametrize("D", [256, 516])
def test_cosine_rows_clamp_at_large_eps(D):
    """eps = 0.5 with norms from {0.1, 0.2} and {2, 3} on both operands: both sides of both clamps, none within a factor 2 of
    eps (the subgradient at equality is nobody's contract)."""
    B, N = 5, 5
    x, y, dout = cos_case(B, N, D, 90 + D)
    xn = torch.tensor([0.1, 2.0, 0.2, 3.0, 2.0])
    yn = torch.tensor([0.1, 2.0, 0.2, 3.0, 0.1, 3.0, 2.0])[(torch.arange(B)[:, None] * 3 + torch.arange(N)[None]) % 7]
    x = unit_rows(x) * xn[:, None]
    y = unit_rows(y) * yn[:, :, None]
    check_cosine(x, y, dout, 0.5, f"cosine clamp eps=0.5 D={D}")


# ---- drin_entity_token_mean, fp32 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 260, 768, 1024])
@pytest.mark.parametrize("T", [9, 10, 11, 20])
def test_entity_token_mean_fp32_unrolled_trip_and_second_column_trip(T, D):
    """One pair per ntok = 0 ... T: the 8-row unrolled trip runs from ntok = 10 on, with every remainder behind it up to T = 20
    (two trips and three rows); D = 1024 is 256 float4 columns on a 192-thread block, a second trip of its column loop."""
    pairs = T + 1
    g = torch.Generator().manual_seed(100 * T + D)
    feat = torch.randn(pairs, T, D, generator=g)
    mask = (torch.arange(T)[None, :] < torch.arange(pairs)[:, None]).to(torch.int64)    # pair p has ntok = p
    want = O.entity_token_mean(feat.double()[None], mask[None])[0]
    out = torch.full((pairs, D), NAN, device=DEV)
    feat_d, mask_d = feat.to(DEV), mask.to(DEV)
    _lib.check(_lib.load().drin_entity_token_mean(ptr(feat_d), ptr(mask_d), ptr(out), pairs, T, D, stream()))
    got = out.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.isnan(want[1]).all() and torch.isnan(want[2]).all() and not torch.isnan(want[[0] + list(range(3, pairs))]).any()
    err = torch.nan_to_num(got.double() - want, nan=0.0).abs().max().item()
    print(f"entity token mean T={T} D={D}: max err {err:.2e} over {pairs} pairs (max |ref| {torch.nan_to_num(want, nan=0.0).abs().max().item():.2e})")
    assert err <= 1e-6
