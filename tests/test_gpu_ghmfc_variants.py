"""GHMFC's other mention encoders on the MI355X: drin_act_dropout_* against fp64 with host-regenerated masks, drin_span_mean_*
against fp64, VariantModel's forward against the reference's goldens and its gradients against the fp64 restatement evaluated
at the library's own max indices and dropout masks (tests/ghmfc_variant_restatement.py).  Bars: fp32 element-wise kernels 1e-5
of max|ref|, the span mean 1e-6, model scores 1e-4 (bf16x3) / 1e-5 (f32), every gradient tensor 2e-4 of its max|ref|
(DESIGN.md sections 16, 18, 20).  Every test prints its measured maxima; profiles/ghmfc_variant_parity.txt records them.

The loss of a batch that holds an empty span is NaN (the reference's too), so the gradient tests of the "forms" cases run on
the batch without that row; the empty span's forward NaN row and backward zero block are checked on the kernels and the
forward tests."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.attention import dropout_keep
from drin_amd.config import wikidiverse_config
from drin_amd.ghmfc_variants import VariantModel
from drin_amd.metrics import TopkAccuracy, TripletLoss
from drin_amd.row_ops import act_dropout, span_mean
from drin_amd.train import MELRunner
from tests.ghmfc_variant_inputs import (CASES, EMPTY_SPAN_ROW, FULL_CASES, SHAPE_CASES, SPAN_FORMS, TINY_CASES, case_of, geometry,
                                        mask_lengths, variant_inputs)
from tests.ghmfc_variant_restatement import span_mean as span_mean_fp64
from tests.ghmfc_variant_restatement import variant_scores
from tests.test_ghmfc_host import as_tensors, compare
from tests.test_ghmfc_variants_host import case_model, golden, restatement_args

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
GRAD_TOL, KERNEL_TOL, SPAN_TOL = 2e-4, 1e-5, 1e-6
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731


def rel_err(got, ref, what, scale=None, where=None):
    got, ref = got.double(), ref.double()
    if where is not None:
        got, ref = got[where], ref[where]
    scale = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    print(f"{what}: max err {err:.3e} (max |ref| {scale:.3e}) ratio {err / max(scale, 1e-300):.2e}")
    return err / max(scale, 1e-300)


# ---- activation and row dropout ----------------------------------------------------------------------------
def act_fwd(x, rows, width, act, p, seed=0, call=0, out=None):
    y = torch.full_like(x, float("nan")) if out is None else out
    _lib.check(_lib.load().drin_act_dropout_fwd(ptr(x), ptr(y), rows, width, _lib.ROW_ACT[act], p, seed, call, stream()))
    return y


def act_bwd(x, dy, rows, width, act, p, seed=0, call=0, out=None):
    dx = torch.full_like(dy, float("nan")) if out is None else out
    _lib.check(_lib.load().drin_act_dropout_bwd(ptr(x), ptr(dy), ptr(dx), rows, width, _lib.ROW_ACT[act], p, seed, call, stream()))
    return dx


def act_fp64(x64, act):
    if act == "relu":
        return torch.relu(x64)
    if act == "gelu":
        return 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    return x64 * 1.0


@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("rows,width", [(1, 4), (3, 20), (5, 260), (1000, 512), (37, 2048), (20000, 516)])
def test_act_dropout_against_fp64_with_the_host_mask(rows, width, act):
    n = rows * width
    gen = torch.Generator(device=DEV).manual_seed(rows * 13 + width)
    x = torch.randn(rows, width, device=DEV, generator=gen) * 1.5
    dy = torch.randn(rows, width, device=DEV, generator=gen)
    flat = x.view(-1)
    flat[0], flat[1], flat[2], flat[3] = 0.0, -0.0, 30.0, -30.0        # exact zeros (relu'(0) = 0), both signs, both tails
    if n > 4:
        flat[n - 1] = float("nan")
        flat[n // 2] = 0.0
    nan = torch.isnan(x)
    fine = ~nan
    seed, call = 0xFEDCBA9876543210, 5
    tag = f"act_dropout ({rows},{width}) {act}"
    x64 = x.double().requires_grad_(True)
    a64 = act_fp64(x64, act)
    (g64,) = torch.autograd.grad((a64 * dy.double()).sum(), x64)       # dy act'(x)
    plain_y, plain_dx = act_fwd(x, rows, width, act, 0.0), act_bwd(x, dy, rows, width, act, 0.0)
    for p in (0.0, 0.1, 0.5):
        keep = dropout_keep(seed, call, rows, 1, 1, width, p).to(DEV).view(rows, width)
        ref_y = torch.where(keep, a64.detach() / (1.0 - p), torch.zeros_like(a64))
        ref_dx = torch.where(keep, g64 / (1.0 - p), torch.zeros_like(g64))
        y, dx = act_fwd(x, rows, width, act, p, seed, call), act_bwd(x, dy, rows, width, act, p, seed, call)
        assert rel_err(y, ref_y, f"{tag} p={p} y", where=fine) <= KERNEL_TOL
        assert rel_err(dx, ref_dx, f"{tag} p={p} dx", where=fine) <= KERNEL_TOL
        assert not y[~keep].any() and not dx[~keep].any()              # a dropped element is exactly 0, a dropped NaN too
        assert torch.equal(torch.isnan(y), nan & keep)                 # the NaN stays in its element
        assert not torch.isnan(dx[fine]).any() and (act != "gelu" or torch.equal(torch.isnan(dx), nan & keep))
        if p == 0.0:                                                   # no mask: the plain activation's bits, whatever (seed, call)
            assert torch.equal(y[fine], plain_y[fine]) and torch.equal(dx[fine], plain_dx[fine])
            if act == "none":
                assert torch.equal(y[fine], x[fine]) and torch.equal(dx, dy)
            if act == "relu":
                assert torch.equal(y[fine], torch.relu(x)[fine])
        else:
            share = keep.double().mean().item()
            assert n < 1000 or abs(share - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
        if act == "none":                                              # plain dropout is its own backward, and reads no x
            assert torch.equal(act_bwd(None, x, rows, width, act, p, seed, call)[fine], y[fine])
        assert torch.equal(act_fwd(x, rows, width, act, p, seed, call)[fine], y[fine])          # the same bits every run
        assert torch.equal(act_bwd(x, dy, rows, width, act, p, seed, call)[fine], dx[fine])
        xi, dyi = x.clone(), dy.clone()                                # in place: y = x, dx = dy
        assert torch.equal(act_bwd(x, dyi, rows, width, act, p, seed, call, out=dyi)[fine], dx[fine])
        assert torch.equal(act_fwd(xi, rows, width, act, p, seed, call, out=xi)[fine], y[fine])
    if n > 1000:
        assert not torch.equal(act_fwd(x, rows, width, act, 0.1, seed, call + 1)[fine], act_fwd(x, rows, width, act, 0.1, seed, call)[fine])


def test_act_dropout_function_differentiates_and_counts_as_norm():
    x = torch.randn(7, 24, device=DEV, requires_grad=True)
    G = torch.randn(7, 24, device=DEV)
    drop = (0.5, 3, 1)
    _lib.profile_begin()
    y = act_dropout(x, "gelu", drop)
    (y * G).sum().backward()
    torch.cuda.synchronize()
    classes = _lib.profile_end()
    assert classes["norm"][1] == 2 and sum(n for _ms, n in classes.values()) == 2
    assert torch.equal(x.grad, act_bwd(x.detach(), G, 7, 24, "gelu", *drop)) and torch.equal(y, act_fwd(x.detach(), 7, 24, "gelu", *drop))
    with pytest.raises(ValueError, match="act"):
        act_dropout(x, "tanh")
    with pytest.raises(RuntimeError, match="GPU only"):
        act_dropout(torch.zeros(2, 4), "relu")


# ---- the span mean ---------------------------------------------------------------------------------------------
def span_reference(seq, begin, end, dout):
    B, L, D = seq.shape
    out = span_mean_fp64(seq.double(), begin, end)
    dseq = torch.zeros(B, L, D, dtype=torch.float64, device=seq.device)
    for b in range(B):
        s, e = slice(int(begin[b]), int(end[b])).indices(L)[:2]
        if e > s:
            dseq[b, s:e] = dout[b].double() / (e - s)
    return out, dseq


@pytest.mark.parametrize("D", [16, 260, 768])
@pytest.mark.parametrize("B", [1, 5])
def test_span_mean_forward_and_backward(B, D):
    lib, L = _lib.load(), 12
    forms = [(b, e) for _m, b, e in SPAN_FORMS]
    batches = [forms] if B == 5 else [[f] for f in forms + [(-3, -1), (-20, 3)]]
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + D)
    for spans in batches:
        begin = torch.tensor([s[0] for s in spans], dtype=torch.int64, device=DEV)
        end = torch.tensor([s[1] for s in spans], dtype=torch.int64, device=DEV)
        seq, dout = torch.randn(B, L, D, device=DEV, generator=gen), torch.randn(B, D, device=DEV, generator=gen)
        out, dseq = torch.full((B, D), 7.0, device=DEV), torch.full((B, L, D), float("nan"), device=DEV)
        _lib.check(lib.drin_span_mean_fwd(ptr(seq), ptr(begin), ptr(end), ptr(out), B, L, D, stream()))
        _lib.check(lib.drin_span_mean_bwd(ptr(dout), ptr(begin), ptr(end), ptr(dseq), B, L, D, stream()))
        ref_out, ref_dseq = span_reference(seq, begin, end, dout)
        empty = torch.tensor([len(range(*slice(s, e).indices(L))) == 0 for s, e in spans], device=DEV)
        tag = f"span_mean B={B} D={D} {spans}"
        assert torch.equal(torch.isnan(out), empty[:, None].expand(B, D)) and torch.equal(torch.isnan(ref_out), torch.isnan(out))
        assert not torch.isnan(dseq).any()                             # every element written
        assert not dseq[empty].any()                                   # the empty span: a block of zeros
        if (~empty).any():
            assert rel_err(out[~empty], ref_out[~empty], tag + " out") <= SPAN_TOL
            assert rel_err(dseq, ref_dseq, tag + " dseq") <= SPAN_TOL
        assert torch.equal(dseq != 0, ref_dseq != 0)
        leaf = seq.clone().requires_grad_(True)
        got = span_mean(leaf, begin, end)
        got.backward(dout)
        assert torch.equal(got.nan_to_num(7.0), out.nan_to_num(7.0)) and torch.equal(leaf.grad, dseq)


def test_span_mean_counts_as_pool():
    seq = torch.randn(2, 5, 16, device=DEV, requires_grad=True)
    _lib.profile_begin()
    span_mean(seq, torch.tensor([0, 1]), torch.tensor([2, 9])).sum().backward()
    torch.cuda.synchronize()
    classes = _lib.profile_end()
    assert classes["pool"][1] == 2 and sum(n for _ms, n in classes.values()) == 2


# ---- the model: forward ------------------------------------------------------------------------------------------
def model_and_batch(name, precision, dropout=0.0, seed=0, rows=None):
    arrays = variant_inputs(name)
    if rows is not None:
        arrays = [a[rows] if isinstance(a, np.ndarray) else a for a in arrays]
    model = case_model(name, precision, dropout=dropout, seed=seed).to(DEV)
    return model, as_tensors(arrays, torch.float32, DEV), arrays


def finite_rows(name):
    """the rows whose span is not empty: the batch of the gradient tests"""
    return [b for b in range(case_of(name)["B"]) if b != EMPTY_SPAN_ROW] if case_of(name)["spans"] == "forms" else None


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_goldens(name, precision):
    model, batch, _ = model_and_batch(name, precision)
    model.eval()
    scores, mention = model(batch), model.encode_mentions(batch)
    assert not scores.requires_grad and tuple(scores.shape) == (case_of(name)["B"], geometry(name)["N"])
    want = golden(name, "scores")
    tag = f"{name} {precision}"
    compare(scores, want, TOL[precision] / max(np.nanmax(np.abs(want)), 1e-30), f"{tag} scores vs golden")
    compare(mention, golden(name, "mention_repr"), TOL[precision], f"{tag} mention_repr vs golden")
    if case_of(name)["spans"] == "forms":
        assert torch.isnan(scores[EMPTY_SPAN_ROW]).all() and int(torch.isnan(scores).any(1).sum()) == 1
    model.train()
    with torch.no_grad():                                             # train() at dropout 0: the same composition, the same bits
        assert torch.equal(model(batch).nan_to_num(7.0), scores.nan_to_num(7.0))
        assert torch.equal(model.encode_mentions(batch).nan_to_num(7.0), mention.nan_to_num(7.0))
    if case_of(name)["repr"] == "max" and case_of(name)["enc"] != "linear":
        idx = model.max_indices["text"]
        assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(mention.shape)
    else:
        assert model.max_indices == {}


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_all_zero_mask_in_the_transformer_is_finite_and_private(precision):
    """The library's definition (torch has two answers, so no golden holds one): zero attention rows, finite scores, and no
    other mention's bits change."""
    name = "tr_max_b3"
    model, batch, _ = model_and_batch(name, precision)
    model.eval()
    base = model(batch)
    masked = list(batch)
    masked[1] = batch[1].clone()
    masked[1][0] = 0
    scores = model(masked)
    assert torch.isfinite(scores).all() and torch.equal(scores[1:], base[1:]) and not torch.equal(scores[0], base[0])


# ---- the model: gradients ------------------------------------------------------------------------------------------
def grad_weights(shape, seed=77):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


def stream_keeps(model, p):
    """every mask of the most recent training forward, regenerated on the host from the stream's log, in draw order"""
    s = model.dropout_stream
    return [dropout_keep(s.seed, call, B, H, Lq, Lk, p).to(DEV) for call, B, H, Lq, Lk in s.log]


def reference_at_library_indices(model, arrays, name, G, keeps=None, p=0.0):
    """fp64 scores and per-tensor gradients of the restatement at model.max_indices (and the given masks); also the sequence
    under the final representation"""
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    b64 = as_tensors(arrays, torch.float64, DEV)
    idx = model.max_indices.get("text")
    scores, _m, pre = variant_scores(b64, sd, **restatement_args(name), idx=idx, keeps=keeps, p=p, return_pre=True)
    grads = torch.autograd.grad((scores * G.double()).sum(), list(sd.values()), allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g) for k, g in zip(sd, grads)}
    return scores.detach(), grads, pre.detach()


def key_bias_rows(k, t):
    """rows E : 2 E of an in_proj_bias - the key bias, whose true gradient is zero (softmax ignores a constant added to every
    key) - or None"""
    if not k.endswith("in_proj_bias"):
        return None
    E = t.numel() // 3
    rows = torch.zeros(t.numel(), dtype=torch.bool, device=t.device)
    rows[E:2 * E] = True
    return rows


def check_against_reference(tag, model, scores, ref_scores, ref_grads, precision):
    assert rel_err(scores, ref_scores, f"{tag} scores", 1.0) <= TOL[precision]
    params = dict(model.named_parameters())
    assert list(params) == list(ref_grads)
    top = max(g.abs().max().item() for g in ref_grads.values())
    assert top > 0
    worst = 0.0
    for k, ref in ref_grads.items():
        got = params[k].grad
        assert got is not None and torch.isfinite(got).all(), k
        diff = (got.double() - ref).abs()
        kb = key_bias_rows(k, ref)
        if kb is not None:                                            # the key bias against the model's largest gradient
            ratio = diff[kb].max().item() / top
            worst = max(worst, ratio)
            assert ratio <= GRAD_TOL, (k, "key bias", ratio)
            diff, ref = diff[~kb], ref[~kb]
        own = ref.abs().max().item()
        ratio = diff.max().item() / (own if own > 0 else top)
        worst = max(worst, ratio)
        assert ratio <= GRAD_TOL, (k, ratio)
    print(f"{tag} gradients: worst tensor {worst:.2e} of its max|ref| (largest max|ref| {top:.3e})")


def check_indices(tag, model, pre, precision):
    if "text" not in model.max_indices:
        return
    lib_idx = model.max_indices["text"].long()
    assert tuple(lib_idx.shape) == (pre.shape[0], pre.shape[2]) and int(lib_idx.min()) >= 0 and int(lib_idx.max()) < pre.shape[1]
    differs = lib_idx != pre.argmax(1)
    at_lib = pre.gather(1, lib_idx[:, None, :])[:, 0, :]
    gap = ((pre.max(1).values - at_lib).abs().max() / pre.abs().max()).item()
    print(f"{tag}: {int(differs.sum())} of {differs.numel()} indices differ from the fp64 argmax, largest value gap {gap:.2e}")
    assert gap <= TOL[precision]


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


GRAD_CASES = TINY_CASES + SHAPE_CASES + FULL_CASES


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_against_fp64_at_the_librarys_indices(name, precision):
    model, batch, arrays = model_and_batch(name, precision, rows=finite_rows(name))
    model.train()
    scores = model(batch)
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    ref_scores, ref_grads, pre = reference_at_library_indices(model, arrays, name, G)
    tag = f"{name} {precision}"
    check_against_reference(tag, model, scores, ref_scores, ref_grads, precision)
    check_indices(tag, model, pre, precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["tr_avg_b5", "tr_gates"])
def test_dropout_against_fp64_with_the_host_masks(name, precision):
    p = 0.1
    model, batch, arrays = model_and_batch(name, precision, dropout=p, seed=21, rows=finite_rows(name))
    model.train()
    scores = model(batch)
    g = geometry(name)
    B, L, D, H, F, layers = batch[0].shape[0], g["L"], g["D"], g["H"], g["ffn"], g["layers"]
    per_layer = [(B, H, L, L), (B * L, 1, 1, D), (B * L, 1, 1, F), (B * L, 1, 1, D)]   # attention, drop1, drop, drop2
    assert model.dropout_stream.log == [(4 * i + j, *per_layer[j]) for i in range(layers) for j in range(4)]
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    keeps = stream_keeps(model, p)
    ref_scores, ref_grads, _pre = reference_at_library_indices(model, arrays, name, G, keeps, p)
    check_against_reference(f"{name} {precision} dropout {p}", model, scores, ref_scores, ref_grads, precision)
    with torch.no_grad():
        assert not torch.equal(model(batch), scores)                  # the next draws: other masks
        model.dropout_stream.counter = 0
        assert torch.equal(model(batch), scores)                      # the same draws: the same bits
        model.eval()
        plain, _b, _a = model_and_batch(name, precision, rows=finite_rows(name))
        assert torch.equal(model(batch), plain.eval()(batch))         # eval() ignores dropout


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_text_variant_draws_its_two_attention_masks(precision):
    name, p = "text_max_b3", 0.1
    model, batch, arrays = model_and_batch(name, precision, dropout=p, seed=4)
    model.train()
    scores = model(batch)
    g = geometry(name)
    assert model.dropout_stream.log == [(0, 3, g["H"], g["L"], g["P"]), (1, 3, g["H"], g["L"], g["L"])]
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    ref_scores, ref_grads, _pre = reference_at_library_indices(model, arrays, name, G, stream_keeps(model, p), p)
    check_against_reference(f"{name} {precision} dropout {p}", model, scores, ref_scores, ref_grads, precision)


def test_backward_is_reproducible_and_freezing_changes_no_bit():
    model, batch, _ = model_and_batch("tr_full_max_b2", "bf16x3")
    model.train()
    G = grad_weights((2, 11))

    def grads():
        model.zero_grad(set_to_none=True)
        (model(batch) * G).sum().backward()
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    first, second = grads(), grads()
    assert len(first) == 98 and all(torch.equal(first[k], second[k]) for k in first)
    live = [k for k in first if k.startswith("entity_encoder")]
    for k, p in model.named_parameters():
        p.requires_grad_(k in live)
    frozen = grads()
    assert len(live) == 2 and all(torch.equal(frozen[k], first[k]) for k in live)
    assert all(frozen[k] is None for k in first if k not in live)


def test_adam_steps_track_the_restatement():
    """Ten Adam steps (lr 1e-3) in f32 against an fp64 Adam on the restatement.  Bars as tests/test_gpu_ghmfc_train.py's test of
    the same name: scores 1e-4, parameters 2e-4, with its exception for rows E : 2E of every in_proj_bias (the key bias: a true
    gradient of zero, so Adam normalises rounding noise into lr-sized steps that cannot affect a score).  ADAM_SEED was picked
    on the CPU (fp64, the restatement alone) among 80 .. 99 as the one whose smallest gradient element over the ten steps is
    largest against its tensor's maximum (1.7e-5): elements whose true gradient is near zero have the key bias's problem."""
    name = "tr_adam_b16"
    model, batch, arrays = model_and_batch(name, "f32")
    model.train()
    args = restatement_args(name)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    b64 = as_tensors(arrays, torch.float64, DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt64 = torch.optim.Adam(list(sd.values()), lr=1e-3)
    G = grad_weights((16, 4), seed=ADAM_SEED)
    for _ in range(10):
        opt.zero_grad()
        (model(batch) * G).sum().backward()
        opt.step()
        opt64.zero_grad()
        (variant_scores(b64, sd, **args) * G.double()).sum().backward()
        opt64.step()
    with torch.no_grad():
        assert rel_err(model(batch), variant_scores(b64, sd, **args), "adam scores", 1.0) < 1e-4
        worst = 0.0
        for k, p in model.named_parameters():
            diff = (p.double() - sd[k]).abs()
            kb = key_bias_rows(k, diff)
            if kb is not None:
                diff[kb] = 0.0
            worst = max(worst, diff.max().item())
            assert diff.max().item() < 2e-4, (k, diff.max().item())
        print(f"adam parameters: worst {worst:.3e}")


ADAM_SEED = 84


def test_test_epoch_matches_the_restatement():
    name = "tr_max_b3"
    g = geometry(name)
    cfg = wikidiverse_config(metrics_topk=(1, 2))
    model, _batch, arrays = model_and_batch(name, "f32")
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    B = case_of(name)["B"]
    mf, mmask, begin, end, _image, ef, _, _ = as_tensors(arrays, torch.float32)
    answer = torch.eye(g["N"] - 1, dtype=torch.int8)[torch.tensor([0, 2, 1])]
    zeros = torch.zeros(B, dtype=torch.int64)                         # what the loader's collate makes of the scalar 0 items
    batch = [mf, mmask, begin, end, zeros, ef, zeros, zeros, answer]
    with torch.no_grad():
        ref = variant_scores([t.double() if t.is_floating_point() else t for t in batch[:8]], sd, **restatement_args(name))
    meters = [TopkAccuracy(k) for k in cfg.metrics_topk]
    for m in meters:
        m.update(ref, answer)
    want_loss = TripletLoss(cfg.triplet_margin)(answer, ref).item()
    want_topk = [float(m.compute()) / (1 - cfg.acc_correction[2]) for m in meters]
    log = MELRunner(cfg, model, DEV).test([batch])
    print(f"test epoch: loss {log.loss:.9f} vs {want_loss:.9f}, top-k {log.topk} vs {want_topk}")
    assert abs(log.loss - want_loss) <= 1e-7
    assert np.allclose(log.topk, want_topk, rtol=0, atol=1e-5)
    assert model.training is False and int(mask_lengths(name).min()) >= 1
