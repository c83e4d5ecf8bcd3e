"""The trainable attention on the MI355X: drin_attention_train_fwd against drin_attention and fp64 logsumexp,
drin_attention_bwd against fp64 autograd of the restatement (tests/attention_restatement.py), the write / stride / mask
contracts of both, and drin_amd.attention.MultiheadAttention against the fp64 restatement in both precisions.

Bars.  Core gradients: max|got - ref| <= 1e-5 x max(scale), the project's fp32 bar for this core, where the scale is the
fp64 gradient recomputed with absolute values at the cancelling step (with one kept key ds is identically 0, so max|ref| is
no scale).  Module: output within 1e-4 (bf16x3) / 1e-5 (f32) of max|ref|, every gradient tensor within 2e-4 of its max|ref|
(the MELHI gradient bar).  DESIGN.md section 16 has the measured maxima."""
import ctypes as C
import math

import pytest
import torch

from drin_amd import _lib
from drin_amd.attention import MultiheadAttention, attention_core, attention_core_packed
from tests import attention_restatement as restate
from tests.test_gpu_ghmfc import attention, masks_for

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
GRAD_TOL = 2e-4
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
FWD_SHAPES = [(1, 1, 1, 1, 1), (3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (49, 128, 256, 8, 2), (128, 49, 96, 8, 2), (7, 65, 9, 4, 3),
              (2, 512, 16, 2, 2), (130, 200, 96, 1, 1)]
BWD_SHAPES = [(1, 1, 1, 1, 1), (3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (17, 64, 4, 2, 2), (16, 63, 64, 1, 2), (7, 65, 9, 4, 3),
              (33, 33, 132, 1, 1), (49, 128, 256, 8, 2), (128, 49, 96, 8, 2), (2, 512, 16, 2, 2), (130, 200, 96, 1, 1)]
SMALL_SHAPES = [(3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (17, 64, 4, 2, 2), (7, 65, 9, 4, 3)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def train_fwd(q, k, v, mask, B, H, Lq, Lk, dh):
    """(out [B Lq, E], lse [B, H, Lq]), both prefilled with NaN."""
    out = torch.full((B * Lq, H * dh), float("nan"), device=DEV)
    lse = torch.full((B, H, Lq), float("nan"), device=DEV)
    _lib.check(_lib.load().drin_attention_train_fwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(mask), ptr(out),
                                                    out.stride(0), ptr(lse), B, H, Lq, Lk, dh, stream()))
    return out, lse


def bwd(q, k, v, mask, out, lse, dout, dq, dk, dv, B, H, Lq, Lk, dh):
    """drin_attention_bwd into the given (strided) gradient buffers; dq may be None."""
    delta = torch.full((B, H, Lq), float("nan"), device=DEV)
    _lib.check(_lib.load().drin_attention_bwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(mask), ptr(out),
                                              out.stride(0), ptr(lse), ptr(dout), dout.stride(0), ptr(dq), dq.stride(0) if dq is not None else 0,
                                              ptr(dk), dk.stride(0), ptr(dv), dv.stride(0), ptr(delta), B, H, Lq, Lk, dh, stream()))
    return dq, dk, dv


def nan_like(rows, E):
    return torch.full((rows, E), float("nan"), device=DEV)


def bwd_masks(B, Lk, gen):
    m = masks_for(B, Lk)
    rnd = (torch.rand(B, Lk, device=DEV, generator=gen) < 0.6).to(torch.int64)
    rnd[:, Lk // 2] = 1
    m["random"] = rnd
    return m


def operands(Lq, Lk, dh, H, B):
    gen = torch.Generator(device=DEV).manual_seed(Lq * 1000 + Lk + dh)
    E = H * dh
    q, k, v, dout = (torch.randn(B * n, E, device=DEV, generator=gen) for n in (Lq, Lk, Lk, Lq))
    return gen, q, k, v, dout


def run_core(q, k, v, mask, dout, dims, want_dq=True):
    Lq, Lk, dh, H, B = dims
    E = H * dh
    out, lse = train_fwd(q, k, v, mask, B, H, Lq, Lk, dh)
    dq, dk, dv = bwd(q, k, v, mask, out, lse, dout, nan_like(B * Lq, E) if want_dq else None, nan_like(B * Lk, E), nan_like(B * Lk, E),
                     B, H, Lq, Lk, dh)
    return out, lse, dq, dk, dv


def fp64_gradients(q, k, v, mask, dout, dims):
    """fp64 autograd of the restatement, and the scale of each gradient: the same sums with absolute values at the
    cancelling step ds = p (dp - sum_j p dp)."""
    Lq, Lk, dh, H, B = dims
    E = H * dh
    q3, k3, v3 = (t.double().reshape(B, -1, E).requires_grad_(True) for t in (q, k, v))
    g3 = dout.double().reshape(B, Lq, E)
    out = restate.attention_core(q3, k3, v3, mask, H)
    ref = torch.autograd.grad((out * g3).sum(), (q3, k3, v3))
    heads = lambda t: t.detach().abs().reshape(B, -1, H, dh).permute(0, 2, 1, 3)   # noqa: E731
    p = restate.core_weights(q3.detach(), k3.detach(), mask, H)
    a = heads(g3) @ heads(v3).transpose(-1, -2)
    ds_abs = p * (a + (p * a).sum(-1, keepdim=True)) / math.sqrt(dh)
    scales = (ds_abs @ heads(k3), ds_abs.transpose(-1, -2) @ heads(q3), p.transpose(-1, -2) @ heads(g3))
    return [r.reshape(-1, E) for r in ref], [s.max().item() for s in scales]


# ---- 1. the forward that keeps its row statistics -----------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", FWD_SHAPES)
def test_train_forward(Lq, Lk, dh, H, B):
    gen = torch.Generator(device=DEV).manual_seed(Lq * 1000 + Lk)
    E = H * dh
    q = torch.randn(B * Lq, E, device=DEV, generator=gen)
    kv = torch.randn(B * Lk, 2 * E + 4, device=DEV, generator=gen)    # K | V packed: row stride 2 E + 4 > E
    k, v = kv[:, :E], kv[:, E:2 * E]
    for mname, mask in masks_for(B, Lk).items():
        out, lse = train_fwd(q, k, v, mask, B, H, Lq, Lk, dh)
        assert torch.equal(out, attention(q, k, v, mask, B, H, Lq, Lk, dh))          # bit-equal to drin_attention
        s = (q.double().reshape(B, Lq, H, dh).permute(0, 2, 1, 3) @ k.double().reshape(B, Lk, H, dh).permute(0, 2, 3, 1)) / math.sqrt(dh)
        if mask is not None:
            s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
        ref = torch.logsumexp(s, -1)
        live = torch.isfinite(ref)
        err = (lse.double() - ref)[live].abs().max().item() if live.any() else 0.0
        bound = 1e-5 * max(1.0, ref[live].abs().max().item() if live.any() else 0.0)
        print(f"train_fwd ({Lq},{Lk},{dh},{H},{B}) {mname}: lse max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert torch.equal(lse[~live], ref[~live].float())             # exactly -inf where no key is kept
        if mname == "gone":
            assert (~live).sum().item() == H * Lq and (lse[B - 1] == float("-inf")).all()


# ---- 2. the backward against fp64 autograd -------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", BWD_SHAPES)
def test_core_backward_against_fp64(Lq, Lk, dh, H, B):
    dims = (Lq, Lk, dh, H, B)
    gen, q, k, v, dout = operands(*dims)
    for mname, mask in bwd_masks(B, Lk, gen).items():
        _out, _lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)
        refs, scales = fp64_gradients(q, k, v, mask, dout, dims)
        for name, got, ref, scale in zip(("dq", "dk", "dv"), (dq, dk, dv), refs, scales):
            err = (got.double() - ref).abs().max().item()
            print(f"attention_bwd ({Lq},{Lk},{dh},{H},{B}) {mname} {name}: max err {err:.3e} scale {scale:.3e} "
                  f"ratio {err / scale if scale > 0 else 0.0:.3e}")
            assert torch.isfinite(got).all()
            if scale == 0:
                assert not got.any()
            else:
                assert err <= 1e-5 * scale, (mname, name, err, scale)


# ---- 3. contracts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", SMALL_SHAPES)
def test_core_backward_contracts(Lq, Lk, dh, H, B):
    dims = (Lq, Lk, dh, H, B)
    E = H * dh
    gen, q, k, v, dout = operands(*dims)
    for mname, mask in bwd_masks(B, Lk, gen).items():
        out, lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)                  # outputs prefilled with NaN
        assert all(torch.isfinite(t).all() for t in (dq, dk, dv)), "written, not accumulated"
        _o, _l, dq2, dk2, dv2 = run_core(q, k, v, mask, dout, dims)
        assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "two runs are bit-equal"
        _o, _l, none, dk3, dv3 = run_core(q, k, v, mask, dout, dims, want_dq=False)
        assert none is None and torch.equal(dk, dk3) and torch.equal(dv, dv3), "dq = NULL changes no bit of dk / dv"
        # dK | dV in one [rows, 2 E + 4] buffer prefilled with 7: only their columns change, same bits
        packed = torch.full((B * Lk, 2 * E + 4), 7.0, device=DEV)
        bwd(q, k, v, mask, out, lse, dout, None, packed[:, :E], packed[:, E:2 * E], B, H, Lq, Lk, dh)
        assert torch.equal(packed[:, :E], dk) and torch.equal(packed[:, E:2 * E], dv) and (packed[:, 2 * E:] == 7.0).all()
        wide = torch.full((B * Lq, E + 3), 7.0, device=DEV)
        bwd(q, k, v, mask, out, lse, dout, wide[:, :E], nan_like(B * Lk, E), nan_like(B * Lk, E), B, H, Lq, Lk, dh)
        assert torch.equal(wide[:, :E], dq) and (wide[:, E:] == 7.0).all()
        # strided q / k / v / dout views change no bit
        qw, gw = (torch.randn(B * Lq, E + 8, device=DEV, generator=gen) for _ in range(2))
        kvw = torch.randn(B * Lk, 2 * E + 4, device=DEV, generator=gen)
        qw[:, 4:4 + E], gw[:, :E], kvw[:, :E], kvw[:, E:2 * E] = q, dout, k, v
        qs, gs, ks, vs = qw[:, 4:4 + E], gw[:, :E], kvw[:, :E], kvw[:, E:2 * E]
        out_s, lse_s = train_fwd(qs, ks, vs, mask, B, H, Lq, Lk, dh)
        assert torch.equal(out_s, out) and torch.equal(lse_s, lse)
        dq4, dk4, dv4 = bwd(qs, ks, vs, mask, out, lse, gs, nan_like(B * Lq, E), nan_like(B * Lk, E), nan_like(B * Lk, E), B, H, Lq, Lk, dh)
        assert torch.equal(dq, dq4) and torch.equal(dk, dk4) and torch.equal(dv, dv4)
        if mask is not None:                                                        # a dropped key's rows are exactly 0
            dropped = (mask == 0).reshape(-1)
            assert not dk[dropped].any() and not dv[dropped].any()
        if mname == "gone":                                                         # the fully masked mention: exactly 0
            assert not dq[(B - 1) * Lq:].any() and not dk[(B - 1) * Lk:].any() and not dv[(B - 1) * Lk:].any()
            assert dv[:(B - 1) * Lk].any()


def test_autograd_core_matches_the_entry_points():
    """attention_core / attention_core_packed are the two entry points and nothing else: same bits, views read in place."""
    dims = Lq, Lk, dh, H, B = (12, 3, 8, 2, 5)
    E = H * dh
    gen, q, k, v, dout = operands(*dims)
    mask = bwd_masks(B, Lk, gen)["random"]
    out, _lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)
    leaves = [t.reshape(B, -1, E).clone().requires_grad_(True) for t in (q, k, v)]
    got = attention_core(*leaves, mask, H)
    grads = torch.autograd.grad(got, leaves, dout.reshape(B, Lq, E))
    assert torch.equal(got.reshape(-1, E), out)
    assert all(torch.equal(g.reshape(-1, E), r) for g, r in zip(grads, (dq, dk, dv)))
    kv = torch.cat([k, v], 1).reshape(B, Lk, 2 * E).requires_grad_(True)
    q3 = leaves[0].detach()                                            # q needs no gradient: dq is skipped
    got = attention_core_packed(q3, kv, mask, H)
    (gkv,) = torch.autograd.grad(got, [kv], dout.reshape(B, Lq, E))
    assert torch.equal(got.reshape(-1, E), out) and torch.equal(gkv.reshape(-1, 2 * E), torch.cat([dk, dv], 1))


# ---- 4. the module against the fp64 restatement ----------------------------------------------------------------
MODULE_SHAPES = [(3, 5, 7, 32, None, 4), (2, 3, 9, 40, 20, 8), (8, 128, 49, 128, 256, 2), (2, 49, 128, 2048, 768, 8)]


def module_case(B, Lq, Lk, E, kdim, H, precision):
    gen = torch.Generator(device=DEV).manual_seed(B * 100 + Lq + Lk + E)
    torch.manual_seed(E + H)
    mha = MultiheadAttention(E, H, kdim=kdim, vdim=kdim, batch_first=True, precision=precision).to(DEV)
    with torch.no_grad():
        for n, p in mha.named_parameters():
            if n.endswith("bias"):                                    # torch draws zero biases
                p.copy_(torch.randn(p.shape, device=DEV, generator=gen) * 0.1)
    query = torch.randn(B, Lq, E, device=DEV, generator=gen)
    key = torch.randn(B, Lk, kdim or E, device=DEV, generator=gen)
    proj = torch.randn(B, Lq, E, device=DEV, generator=gen)
    drop = torch.rand(B, Lk, device=DEV, generator=gen) < 0.4
    drop[:, :2] = False                                               # at least two kept keys per mention
    masks = {"random": drop}
    if B >= 2:
        gone = drop.clone()
        gone[B - 1] = True                                            # one mention fully masked
        masks["gone"] = gone
    return mha, query, key, proj, masks


def module_grads(mha, query, key, proj, mask):
    """(out, {name: gradient}) of loss = sum(out * proj) through the module; key is value."""
    q, k = query.clone().requires_grad_(True), key.clone().requires_grad_(True)
    params = [p for p in mha.parameters() if p.requires_grad]
    out, weights = mha(q, k, k, key_padding_mask=mask)
    assert weights is None
    grads = torch.autograd.grad((out * proj).sum(), [q, k] + params)
    names = ["query", "key"] + [n for n, p in mha.named_parameters() if p.requires_grad]
    return out.detach(), dict(zip(names, grads))


def reference_grads(mha, query, key, proj, mask):
    sd = {n: p.detach().double().requires_grad_(True) for n, p in mha.named_parameters()}
    q, k = query.double().requires_grad_(True), key.double().requires_grad_(True)
    out = restate.multihead_attention(sd, q, k, k, mask, mha.num_heads)
    names = list(sd)
    grads = torch.autograd.grad((out * proj.double()).sum(), [q, k] + [sd[n] for n in names])
    return out.detach(), dict(zip(["query", "key"] + names, grads))


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,Lq,Lk,E,kdim,H", MODULE_SHAPES)
def test_module_against_fp64(B, Lq, Lk, E, kdim, H, precision):
    mha, query, key, proj, masks = module_case(B, Lq, Lk, E, kdim, H, precision)
    mha.train()
    for mname, mask in masks.items():
        if (B, Lq) == (8, 128) and mname == "random":
            _lib.profile_begin()
            out, grads = module_grads(mha, query, key, proj, mask)
            prof = _lib.profile_end()
            assert precision != "bf16x3" or prof["gemm_x3"][1] > 0, prof          # crosses the GEMM module's split-bf16 gates
        else:
            out, grads = module_grads(mha, query, key, proj, mask)
        ref_out, ref_grads = reference_grads(mha, query, key, proj, mask)
        err = ((out.double() - ref_out).abs().max() / ref_out.abs().max()).item()
        print(f"mha ({B},{Lq},{Lk},{E},{kdim},{H}) {precision} {mname} out: {err:.3e}")
        assert err <= TOL[precision]
        assert sorted(grads) == sorted(ref_grads)
        for name, ref in ref_grads.items():
            rel = ((grads[name].double() - ref).abs().max() / ref.abs().max()).item()
            print(f"mha ({B},{Lq},{Lk},{E},{kdim},{H}) {precision} {mname} d {name}: {rel:.3e}")
            assert rel < GRAD_TOL, (name, rel)
        _out2, again = module_grads(mha, query, key, proj, mask)                     # two backward passes: the same bits
        assert all(torch.equal(grads[n], again[n]) for n in grads)


@pytest.mark.parametrize("B,Lq,Lk,E,kdim,H", MODULE_SHAPES[:3])
def test_module_frozen_subset_and_eval(B, Lq, Lk, E, kdim, H):
    mha, query, key, proj, masks = module_case(B, Lq, Lk, E, kdim, H, "bf16x3")
    mask = masks["random"]
    _out, full = module_grads(mha, query, key, proj, mask)
    for n, p in mha.named_parameters():
        p.requires_grad_(n.startswith("out_proj"))
    q = query.clone()                                                  # no input gradient either
    out, _w = mha(q, key, key, key_padding_mask=mask)
    gw, gb = torch.autograd.grad((out * proj).sum(), [mha.out_proj.weight, mha.out_proj.bias])
    assert torch.equal(gw, full["out_proj.weight"]) and torch.equal(gb, full["out_proj.bias"])
    # eval() under no_grad: drin_linear_fwd -> drin_attention -> drin_linear_fwd composed by hand
    mha.eval()
    with torch.no_grad():
        got, _w = mha(query, key, key, key_padding_mask=mask)
    lib, prec = _lib.load(), _lib.PREC_BF16X3

    def linear(x, w, b):
        y = torch.empty(x.shape[0], w.shape[0], device=DEV)
        _lib.check(lib.drin_linear_fwd(ptr(x), ptr(w.contiguous()), ptr(b.contiguous()), ptr(y), x.shape[0], w.shape[0], x.shape[1], prec,
                                       stream()))
        return y

    bias = mha.in_proj_bias.detach()
    xq, xk, keep = query.reshape(B * Lq, E), key.reshape(B * Lk, -1), (~mask).to(torch.int64)
    if kdim is None:                                                   # K | V: one product, read in place
        w = mha.in_proj_weight.detach()
        kv = linear(xk, w[E:], bias[E:])
        ctx = attention(linear(xq, w[:E], bias[:E]), kv[:, :E], kv[:, E:], keep, B, H, Lq, Lk, E // H)
    else:
        ctx = attention(linear(xq, mha.q_proj_weight.detach(), bias[:E]), linear(xk, mha.k_proj_weight.detach(), bias[E:2 * E]),
                        linear(xk, mha.v_proj_weight.detach(), bias[2 * E:]), keep, B, H, Lq, Lk, E // H)
    want = linear(ctx, mha.out_proj.weight.detach(), mha.out_proj.bias.detach()).reshape(B, Lq, E)
    assert torch.equal(got, want)                                      # the same launches: the same bits


def test_module_dropout_only_refused_in_training():
    mha = MultiheadAttention(32, 4, dropout=0.1, batch_first=True).to(DEV)
    x = torch.randn(2, 5, 32, device=DEV)
    with pytest.raises(NotImplementedError, match="dropout"):
        mha(x, x, x)
    mha.eval()
    out, _w = mha(x, x, x)
    assert torch.isfinite(out).all()


# ---- 5. kernel classes -----------------------------------------------------------------------------------------
def test_new_kernels_count_as_attn():
    dims = (12, 3, 8, 2, 5)
    _gen, q, k, v, dout = operands(*dims)
    _lib.profile_begin()
    run_core(q, k, v, None, dout, dims)
    prof = _lib.profile_end()
    assert prof["attn"][1] == 4 and sum(n for _ms, n in prof.values()) == 4, prof      # forward, delta, dq, dkv
    _lib.profile_begin()
    run_core(q, k, v, None, dout, dims, want_dq=False)
    assert _lib.profile_end()["attn"][1] == 3
