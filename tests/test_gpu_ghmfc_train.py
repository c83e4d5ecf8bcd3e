"""GHMFC training on the MI355X: each backward row kernel against fp64 autograd, the sequence max and its scatter exactly,
the dropout core against the fp64 core with the host-generated mask, and TrainableModel's gradients against the fp64
restatement evaluated at the library's own max indices (tests/ghmfc_train_restatement.py says why).  Bars: fp32-FMA kernels
1e-5 of max|ref|, model scores 1e-4 (bf16x3) / 1e-5 (f32), every gradient tensor 2e-4 of its
max|ref| (sections 14 / 16).  Every test prints its measured maxima; profiles/ghmfc_train_parity.txt records them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.attention import dropout_keep
from drin_amd.ghmfc import GhmfcConfig, Model
from drin_amd.ghmfc_train import TrainableModel
from tests.ghmfc_inputs import CASES, KEYS, ghmfc_inputs, geometry
from tests.ghmfc_train_inputs import TRAIN_CASES, train_inputs
from tests.ghmfc_train_restatement import ghmfc_train_scores
from tests.helpers import ln_bwd, rel_err
from tests.test_ghmfc_host import as_tensors, cfg_for

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
GRAD_TOL, KERNEL_TOL = 2e-4, 1e-5
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731


# ---- LayerNorm with a fused residual -----------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,E", [(1, 16), (5, 260), (1000, 768), (37, 2048)])
def test_layernorm_backward_against_fp64(rows, E, with_res):
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(rows * 7 + E)
    x = torch.randn(rows, E, device=DEV, generator=gen) * 1.5 + 0.3
    res = torch.randn(rows, E, device=DEV, generator=gen) if with_res else None
    gamma = torch.randn(E, device=DEV, generator=gen)
    gamma[::5] = 0.0                                                  # some exact zeros
    beta = torch.randn(E, device=DEV, generator=gen)
    dy = torch.randn(rows, E, device=DEV, generator=gen)
    eps = 1e-5
    y, mean, rstd = torch.full_like(x, float("nan")), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    _lib.check(lib.drin_layernorm_res_train_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, E, eps, stream()))
    # (y against the scoring pass's bits: test_eval_and_train_forward_agree, through the model)
    h64 = (x.double() + (res.double() if with_res else 0.0)).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu = h64.mean(-1, keepdim=True)
    var = ((h64 - mu) ** 2).mean(-1, keepdim=True)
    y64 = (h64 - mu) / torch.sqrt(var + eps) * g64 + b64
    ref_dh, ref_dg, ref_db = torch.autograd.grad((y64 * dy.double()).sum(), [h64, g64, b64])
    tag = f"layernorm ({rows},{E}) res={with_res}"
    assert rel_err(y, y64.detach(), tag + " y") <= KERNEL_TOL
    assert rel_err(mean, mu.detach()[:, 0], tag + " mean", max(mu.abs().max().item(), 1.0)) <= KERNEL_TOL
    assert rel_err(rstd, 1.0 / torch.sqrt(var.detach() + eps)[:, 0], tag + " rstd") <= KERNEL_TOL
    dh, dgamma, dbeta = ln_bwd(x, res, mean, rstd, gamma, dy)
    assert rel_err(dh, ref_dh, tag + " dh") <= KERNEL_TOL
    assert rel_err(dgamma, ref_dg, tag + " dgamma") <= KERNEL_TOL
    assert rel_err(dbeta, ref_db, tag + " dbeta") <= KERNEL_TOL
    frozen, none_g, none_b = ln_bwd(x, res, mean, rstd, gamma, dy, sums=False)
    assert none_g is None and none_b is None and torch.equal(frozen, dh)   # a frozen LayerNorm: the same dh bits
    again = ln_bwd(x, res, mean, rstd, gamma, dy)
    assert all(torch.equal(a, b) for a, b in zip(again, (dh, dgamma, dbeta)))   # the same bits every run


# ---- the max over a sequence -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,E", [(2, 1, 16), (3, 5, 260), (2, 200, 16)])
def test_seq_max_indices_and_scatter_are_exact(B, S, E):
    lib = _lib.load()
    rng = np.random.default_rng(B * 100 + S)
    x = rng.standard_normal((B, S, E)).astype(np.float32)
    if S > 1:
        top = x.max(1)
        x[0, S - 1, 0:4] = top[0, 0:4]                                # an exact tie with a later position
        x[0, 0, 4:8] = top[0, 4:8]                                    # ... and with the first one
        x[B - 1, :, 8] = 0.25                                         # a whole column tied
        x[0, :, 9] = np.where(np.arange(S) % 2 == 0, 0.0, -0.0)       # signed zeros are equal
        x[0, S // 2, 10] = np.nan                                     # a NaN wins
        x[0, S - 1, 11] = np.nan                                      # a NaN after the maximum
        x[B - 1, 1, 12] = np.nan
        x[B - 1, S - 1, 12] = np.nan                                  # two NaNs: the lowest position
        x[B - 1, :, 13] = -np.inf
    else:
        x[0, 0, 3] = np.nan
        x[1, 0, 5] = -np.inf
    xt = torch.from_numpy(x).to(DEV)
    out, idx = torch.full((B, E), 7.0, device=DEV), torch.full((B, E), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.drin_seq_max_train_fwd(ptr(xt), ptr(out), ptr(idx), B, S, E, stream()))
    want_idx = np.argmax(x, axis=1)                                   # first occurrence, NaN counts as the maximum
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    want = np.take_along_axis(x, want_idx[:, None, :], 1)[:, 0, :]
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    # (out against the scoring pass's bits: test_eval_and_train_forward_agree, through the model)
    ref = torch.from_numpy(x).max(1).values.numpy()
    assert np.array_equal(np.nan_to_num(got, nan=7.0), np.nan_to_num(ref, nan=7.0))
    dout = torch.randn(B, E, device=DEV)
    dx = torch.full((B, S, E), float("nan"), device=DEV)
    _lib.check(lib.drin_seq_max_bwd(ptr(dout), ptr(idx), ptr(dx), B, S, E, stream()))
    want_dx = torch.zeros(B, S, E, device=DEV).scatter_(1, idx.long()[:, None, :], dout[:, None, :])
    assert torch.equal(dx, want_dx) and int((dx != 0).sum()) <= B * E


# ---- the gate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_gate_backward_against_fp64(B, D):
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(B * 31 + D)
    tl, vl, dout = (torch.randn(B, D, device=DEV, generator=gen) for _ in range(3))
    ws = torch.randn(2, 2 * D, device=DEV, generator=gen) / math.sqrt(2 * D)
    bs = torch.randn(2, device=DEV, generator=gen)
    ws[1], bs[1] = ws[0], bs[0]
    ws[1, 1:] += 0.05 * torch.randn(2 * D - 1, device=DEV, generator=gen)
    tl[B - 1], vl[B - 1] = 0.0, 0.0                                   # gelu(0) = 0: this mention's two logits are both bs[0]
    out = torch.full((B, D), float("nan"), device=DEV)
    _lib.check(lib.drin_gate_mix_fwd(ptr(tl), ptr(vl), ptr(ws), ptr(bs), ptr(out), B, D, stream()))
    leaves = [t.double().requires_grad_(True) for t in (tl, vl, ws, bs)]
    gelu = lambda a: 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))   # noqa: E731
    t, v = gelu(leaves[0]), gelu(leaves[1])
    z = torch.cat([t, v], 1) @ leaves[2].T + leaves[3]
    assert z[B - 1, 0].item() == z[B - 1, 1].item()
    s = torch.softmax(z, 1)
    out64 = s[:, :1] * t + s[:, 1:] * v
    refs = torch.autograd.grad((out64 * dout.double()).sum(), leaves)
    tag = f"gate ({B},{D})"
    assert rel_err(out, out64.detach(), tag + " out") <= KERNEL_TOL
    floats = lib.drin_gate_mix_bwd_scratch_floats(B, D)

    def run(sums=True):
        dtl, dvl = torch.full_like(tl, float("nan")), torch.full_like(vl, float("nan"))
        dws, dbs = (torch.full_like(ws, float("nan")), torch.full_like(bs, float("nan"))) if sums else (None, None)
        scratch = torch.full((floats,), float("nan"), device=DEV) if sums else None
        _lib.check(lib.drin_gate_mix_bwd(ptr(tl), ptr(vl), ptr(ws), ptr(bs), ptr(dout), ptr(dtl), ptr(dvl), ptr(dws), ptr(dbs), ptr(scratch),
                                         floats if sums else 0, B, D, stream()))
        return dtl, dvl, dws, dbs

    got = run()
    for name, g, r in zip(("dtl", "dvl", "dws", "dbs"), got, refs):
        assert rel_err(g, r, f"{tag} {name}") <= KERNEL_TOL, name
    assert all(torch.equal(a, b) for a, b in zip(run(), got))
    frozen = run(sums=False)
    assert torch.equal(frozen[0], got[0]) and torch.equal(frozen[1], got[1]) and frozen[2] is None


# ---- the dropout core ----------------------------------------------------------------------------------------
def core_fp64(q, k, v, mask, keep, p, B, H, Lq, Lk, dh):
    """out [B Lq, E] in fp64 from fp64 leaves; keep: bool [B, H, Lq, Lk] or None"""
    qh, kh, vh = (t.reshape(B, -1, H, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    w = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    if keep is not None:
        w = w * keep.to(w.dtype) / (1.0 - p)
    return (w @ vh).permute(0, 2, 1, 3).reshape(B * Lq, H * dh)


def core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh, drop=None):
    """(out, dq, dk, dv) through the dropout entry points (drop = (p, seed, call)) or the undropped ones (None)"""
    lib = _lib.load()
    E = H * dh
    out, lse = torch.full((B * Lq, E), float("nan"), device=DEV), torch.empty(B, H, Lq, device=DEV)
    dq, dk, dv = (torch.full((B * n, E), float("nan"), device=DEV) for n in (Lq, Lk, Lk))
    delta = torch.empty(B, H, Lq, device=DEV)
    geo = (B, H, Lq, Lk, dh)
    fwd_args = (ptr(q), E, ptr(k), E, ptr(v), E, ptr(mask), ptr(out), E, ptr(lse)) + geo
    if drop is None:
        _lib.check(lib.drin_attention_train_fwd(*fwd_args, stream()))
    else:
        _lib.check(lib.drin_attention_dropout_fwd(*fwd_args, *drop, stream()))
    bwd_args = (ptr(q), E, ptr(k), E, ptr(v), E, ptr(mask), ptr(out), E, ptr(lse), ptr(dout), E, ptr(dq), E, ptr(dk), E, ptr(dv), E,
                ptr(delta)) + geo
    if drop is None:
        _lib.check(lib.drin_attention_bwd(*bwd_args, stream()))
    else:
        _lib.check(lib.drin_attention_dropout_bwd(*bwd_args, *drop, stream()))
    return out, dq, dk, dv, lse


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,Lq,Lk,dh", [(2, 2, 5, 7, 8), (2, 2, 17, 70, 5), (1, 2, 9, 40, 256)])
def test_dropout_core_against_fp64_with_the_host_mask(B, H, Lq, Lk, dh, p):
    gen = torch.Generator(device=DEV).manual_seed(Lq * 100 + Lk)
    E = H * dh
    q, k, v, dout = (torch.randn(B * n, E, device=DEV, generator=gen) for n in (Lq, Lk, Lk, Lq))
    mask = torch.ones(B, Lk, dtype=torch.int64, device=DEV)
    mask[0, 1::3] = 0
    if B > 1:
        mask[B - 1] = 0                                               # a fully masked mention
    seed, call = 0x1234567890ABCDEF, 3
    keep = dropout_keep(seed, call, B, H, Lq, Lk, p).to(DEV)
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    out64 = core_fp64(*leaves, mask, keep, p, B, H, Lq, Lk, dh)
    refs = torch.autograd.grad((out64 * dout.double()).sum(), leaves)
    out, dq, dk, dv, lse = core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh, (p, seed, call))
    tag = f"dropout core ({B},{H},{Lq},{Lk},{dh}) p={p}"
    assert rel_err(out, out64.detach(), tag + " out") <= KERNEL_TOL
    for name, g, r in (("dq", dq, refs[0]), ("dk", dk, refs[1]), ("dv", dv, refs[2])):
        assert rel_err(g, r, f"{tag} {name}") <= KERNEL_TOL, name
    gone = (mask == 0).reshape(B * Lk)
    assert not dk[gone].any() and not dv[gone].any()                  # a dropped key: exactly-zero rows
    plain = core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh)
    assert torch.equal(lse, plain[4])                                 # lse is that of the undropped scores
    zero = core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh, (0.0, seed, call))
    assert all(torch.equal(a, b) for a, b in zip(zero, plain))        # p = 0: the undropped entry points' bits
    again = core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh, (p, seed, call))
    assert all(torch.equal(a, b) for a, b in zip(again, (out, dq, dk, dv, lse)))
    other = core_run(q, k, v, mask, dout, B, H, Lq, Lk, dh, (p, seed, call + 1))
    assert not torch.equal(other[0], out)


# ---- the model -------------------------------------------------------------------------------------------------
def model_and_batch(name, precision, dropout=0.0, seed=0):
    if name in CASES:
        cfg, wseed, arrays, H = cfg_for(name), CASES[name]["seed"], ghmfc_inputs(name), geometry(name)["H"]
    else:
        case = TRAIN_CASES[name]
        g = case["geom"]
        cfg = GhmfcConfig(dataset_name="wikimel" if "T" in case else "wikidiverse", num_candidates=g["N"], embed_dim=g["D"],
                          image_dim=g["R"], mention_tokens=g["L"], image_regions=g["P"], num_heads=g["H"], entity_tokens=case.get("T", 0))
        wseed, arrays, H = case["seed"], train_inputs(name), g["H"]
    torch.manual_seed(wseed)
    model = TrainableModel(cfg, precision=precision, dropout=dropout, seed=seed).to(DEV).train()
    return model, as_tensors(arrays, torch.float32, DEV), (arrays, H)


def grad_weights(shape, seed=77):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


def stream_keeps(model, p):
    """the four masks of the most recent training forward, regenerated on the host from the stream's log"""
    s = model.dropout_stream
    return [dropout_keep(s.seed, call, B, H, Lq, Lk, p).to(DEV) for call, B, H, Lq, Lk in s.log[-4:]]


def reference_at_library_indices(model, arrays, H, G, keeps=None, p=0.0):
    """fp64 scores and per-tensor gradients of the restatement evaluated at model.max_indices; also the tensors under the maxima"""
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    b64 = as_tensors(arrays, torch.float64, DEV)
    idx = model.max_indices
    scores, pre_t, pre_v = ghmfc_train_scores(b64, sd, H, idx["text"], idx["image"], keeps, p, return_pre_max=True)
    grads = torch.autograd.grad((scores * G.double()).sum(), [sd[k] for k in KEYS], allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g) for k, g in zip(KEYS, grads)}
    return scores.detach(), grads, pre_t.detach(), pre_v.detach()


def check_against_reference(tag, model, scores, ref_scores, ref_grads, precision, zero_ok=False):
    assert rel_err(scores, ref_scores, f"{tag} scores", 1.0) <= TOL[precision]
    params = dict(model.named_parameters())
    top = max(g.abs().max().item() for g in ref_grads.values())
    worst = 0.0
    for k in KEYS:
        own = ref_grads[k].abs().max().item()
        assert own > 0 or zero_ok, f"{k}: the fp64 gradient is exactly zero"
        got = params[k].grad
        assert got is not None and torch.isfinite(got).all(), k
        ratio = (got.double() - ref_grads[k]).abs().max().item() / (own if own > 0 else top)
        worst = max(worst, ratio)
        assert ratio <= GRAD_TOL, (k, ratio)
    print(f"{tag} gradients: worst tensor {worst:.2e} of its max|ref| (largest max|ref| {top:.3e})")


def check_indices(tag, model, pre_t, pre_v, precision, must_equal):
    for side, pre in (("text", pre_t), ("image", pre_v)):
        lib_idx = model.max_indices[side].long()
        assert lib_idx.dtype == torch.int64 and tuple(lib_idx.shape) == (pre.shape[0], pre.shape[2])
        assert int(lib_idx.min()) >= 0 and int(lib_idx.max()) < pre.shape[1]
        arg = pre.argmax(1)
        differs = lib_idx != arg
        at_lib = pre.gather(1, lib_idx[:, None, :])[:, 0, :]
        gap = ((pre.max(1).values - at_lib).abs().max() / pre.abs().max()).item()
        print(f"{tag} {side}: {int(differs.sum())} of {differs.numel()} indices differ from the fp64 argmax, largest value gap {gap:.2e}")
        assert gap <= TOL[precision]
        if must_equal:
            assert not differs.any()


MODEL_CASES = ["wd_b1", "wd_b5", "wm_t6", "heads_5_9", "long_200", "ones", "gates", "full_b2"]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_gradients_against_fp64_at_the_librarys_indices(name, precision):
    model, batch, (arrays, H) = model_and_batch(name, precision)
    scores = model(batch)
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    ref_scores, ref_grads, pre_t, pre_v = reference_at_library_indices(model, arrays, H, G)
    tag = f"{name} {precision}"
    check_against_reference(tag, model, scores, ref_scores, ref_grads, precision, zero_ok=name == "ones")
    check_indices(tag, model, pre_t, pre_v, precision, must_equal=precision == "f32" and name in ("wd_b1", "heads_5_9"))


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["wd_b5", "gates"])
def test_model_with_dropout_against_fp64_with_the_host_masks(name, precision):
    p = 0.1
    model, batch, (arrays, H) = model_and_batch(name, precision, dropout=p, seed=21)
    scores = model(batch)
    assert model.dropout_stream.counter == 4 and [e[0] for e in model.dropout_stream.log] == [0, 1, 2, 3]
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    keeps = stream_keeps(model, p)
    ref_scores, ref_grads, _pt, _pv = reference_at_library_indices(model, arrays, H, G, keeps, p)
    check_against_reference(f"{name} {precision} dropout {p}", model, scores, ref_scores, ref_grads, precision)
    with torch.no_grad():
        assert not torch.equal(model(batch), scores)                  # the next draws: other masks
        model.dropout_stream.counter = 0
        assert torch.equal(model(batch), scores)                      # the same draws: the same bits
        model.eval()
        plain = Model(model.cfg, precision=precision).to(DEV).eval()
        plain.load_state_dict(model.state_dict())
        assert torch.equal(model(batch), plain(batch))                # eval() ignores dropout


def test_backward_is_reproducible_and_freezing_changes_no_bit():
    model, batch, _ = model_and_batch("full_b2", "bf16x3")
    G = grad_weights((2, 11))

    def grads():
        model.zero_grad(set_to_none=True)
        (model(batch) * G).sum().backward()
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    first, second = grads(), grads()
    assert all(torch.equal(first[k], second[k]) for k in KEYS)
    live = [k for k in KEYS if "score_linear" in k or "entity_encoder" in k]
    for k, p in model.named_parameters():
        p.requires_grad_(k in live)
    frozen = grads()
    assert len(live) == 4 and all(torch.equal(frozen[k], first[k]) for k in live)
    assert all(frozen[k] is None for k in KEYS if k not in live)


@pytest.mark.parametrize("name", ["wd_b5", "wm_t6"])
def test_eval_and_train_forward_agree(name):
    """eval(): TrainableModel is ghmfc.Model bit for bit (scores and mention representations).  train() at dropout 0 runs the
    same kernels operation by operation (LayerNorm and the max with their training outputs): the same bits again."""
    for precision in ("bf16x3", "f32"):
        model, batch, _ = model_and_batch(name, precision)
        plain = Model(model.cfg, precision=precision).to(DEV).eval()
        plain.load_state_dict(model.state_dict())
        with torch.no_grad():
            want, want_m = plain(batch), plain.encode_mentions(batch)
            assert torch.isfinite(want).all()
            train_scores, train_m = model(batch), model.encode_mentions(batch)
            model.eval()
            got, got_m = model(batch), model.encode_mentions(batch)
        assert torch.equal(got, want) and torch.equal(got_m, want_m) and not got.requires_grad
        assert torch.equal(train_scores, want) and torch.equal(train_m, want_m)


def test_wm_b3_gives_nan_rows_as_the_reference():
    model, batch, _ = model_and_batch("wm_b3", "f32")
    scores = model(batch)
    plain = Model(model.cfg, precision="f32").to(DEV).eval()
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = plain(batch)
    assert torch.isnan(want).any() and torch.equal(torch.isnan(scores), torch.isnan(want))


def test_adam_steps_track_the_restatement():
    """Ten Adam steps (lr 1e-3) in f32 against an fp64 Adam on the restatement, which takes the library's max indices at every
    step.  Bars as tests/test_gpu_melhi.py's test of the same name: scores 1e-4, parameters 2e-4.  Exception: rows E : 2E of the
    four in_proj_bias - softmax is invariant to a bias added to every key, so their true gradient is zero and Adam
    normalises fp32 rounding noise into lr-sized steps; they cannot affect a score.  ADAM_SEED was picked on the CPU (fp64,
    the restatement's own argmax) so that no other element's gradient falls below 1e-6 of its tensor's maximum over the ten
    steps - elements whose true gradient is (near) zero have the same noise problem."""
    model, batch, (arrays, H) = model_and_batch("adam_b16", "f32")
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
        idx = model.max_indices
        (ghmfc_train_scores(b64, sd, H, idx["text"], idx["image"]) * G.double()).sum().backward()
        opt64.step()
    with torch.no_grad():
        scores = model(batch)
        idx = model.max_indices
        assert rel_err(scores, ghmfc_train_scores(b64, sd, H, idx["text"], idx["image"]), "adam scores", 1.0) < 1e-4
        params = dict(model.named_parameters())
        worst = 0.0
        for k in KEYS:
            diff = (params[k].double() - sd[k]).abs()
            if k.endswith("in_proj_bias"):
                E = diff.numel() // 3
                diff[E:2 * E] = 0.0                                   # the key bias: see the docstring
            worst = max(worst, diff.max().item())
            assert diff.max().item() < 2e-4, k
        print(f"adam parameters: worst {worst:.3e}")


ADAM_SEED = 84


def test_profiler_classes_of_the_new_kernels():
    model, batch, _ = model_and_batch("wd_b5", "f32", dropout=0.1)
    G = grad_weights((5, 4))
    _lib.profile_begin()
    (model(batch) * G).sum().backward()
    torch.cuda.synchronize()
    with_dropout = _lib.profile_end()
    # forward: 8 LayerNorms, 2 maxima, 1 gate; backward: 8 x (row kernel + sums), 2 scatters, gate (row kernel + sums)
    assert with_dropout["norm"][1] == 11 + 16 + 2 + 2
    # 4 attentions: forward 1, backward delta + dq + dkv, except the two whose query side is the detached batch tensor ... no:
    # every query here is a projection of a parameter, so all three backward kernels run
    assert with_dropout["attn"][1] == 4 * 4
    lib = _lib.load()
    x = torch.randn(3, 5, 16, device=DEV)
    out, idx = torch.empty(3, 16, device=DEV), torch.empty(3, 16, dtype=torch.int32, device=DEV)
    _lib.profile_begin()
    _lib.check(lib.drin_seq_max_train_fwd(ptr(x), ptr(out), ptr(idx), 3, 5, 16, stream()))
    _lib.check(lib.drin_seq_max_bwd(ptr(out), ptr(idx), ptr(x), 3, 5, 16, stream()))
    torch.cuda.synchronize()
    only = _lib.profile_end()
    assert only["norm"][1] == 2 and sum(n for _ms, n in only.values()) == 2
