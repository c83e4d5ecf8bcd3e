"""The matrix-core attention core on the MI355X: drin_attention_mfma_fwd / drin_attention_mfma_bwd
against the fp64 restatement (tests/attention_restatement.py), their write / stride / mask contracts, dropout against the
fp64 core under the host-regenerated mask, MultiheadAttention(core="mfma") against the fp64 restatement and the GHMFC models
with core="mfma" on the tiny golden cases.

Bars (the project's split-bf16 ones).  Core: out within 1e-4 of max|ref|; lse within 1e-4 max(1, max|ref|) and exactly -inf
where no key is kept; dq, dk, dv within 2e-4 of the cancellation-aware scale of tests/test_gpu_attention_train.py
(fp64_gradients).  tests/test_attention_mfma_host.py holds the scheme itself (fp64 emulation of the three-pass split on these
shapes) under a quarter of each bar, so a red test here means the kernel.  Module and models: the bars of their own tests.

Shapes (Lq, Lk, dh, H, B).  The kernels' edges: 16-wide MFMA tiles; 32-row staged tiles; a workgroup owns 64 rows (dh <=
128) or 32 (dh > 128, where the two waves of a pair take 8 column tiles each); dh is padded to a multiple of 32; dh % 4 != 0
or unaligned rows take the scalar staging path.  (63, 65, 64, 1, 2) and (65, 33, 132, 1, 1) are one off the 64-row tile, the
32-row staged tile and - at dh = 132 - the 32-row owned tile of the wide kernels.  Every test prints its measured maxima;
profiles/attention_mfma_parity.txt records them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.attention import MultiheadAttention, attention_core, attention_core_packed, dropout_keep
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantModel
from tests import attention_restatement as restate
from tests.test_ghmfc_variants_host import variant_cfg
from tests.test_gpu_attention_train import (GRAD_TOL, MODULE_SHAPES, TOL, bwd_masks, fp64_gradients, module_grads, operands,
                                            reference_grads)
from tests.test_gpu_ghmfc import attention_fp64, masks_for
from tests.test_gpu_ghmfc_train import core_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_TOL, LSE_TOL, CORE_GRAD_TOL = 1e-4, 1e-4, 2e-4
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
SHAPES = [(1, 1, 1, 1, 1), (3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (15, 17, 32, 2, 2), (16, 16, 36, 1, 2), (17, 15, 4, 2, 2),
          (63, 65, 64, 1, 2), (65, 33, 132, 1, 1), (49, 128, 256, 8, 2), (128, 49, 96, 8, 2), (2, 512, 16, 2, 2), (130, 200, 96, 1, 1)]
CONTRACT_SHAPES = [(3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (17, 15, 4, 2, 2), (15, 17, 32, 2, 2)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mfma_fwd(q, k, v, mask, B, H, Lq, Lk, dh, drop=(0.0, 0, 0), want_lse=True):
    """(out [B Lq, E], lse [B, H, Lq] or None), both prefilled with NaN."""
    out = torch.full((B * Lq, H * dh), float("nan"), device=DEV)
    lse = torch.full((B, H, Lq), float("nan"), device=DEV) if want_lse else None
    _lib.check(_lib.load().drin_attention_mfma_fwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(mask), ptr(out),
                                                   out.stride(0), ptr(lse), B, H, Lq, Lk, dh, *drop, stream()))
    return out, lse


def mfma_bwd(q, k, v, mask, out, lse, dout, dq, dk, dv, B, H, Lq, Lk, dh, drop=(0.0, 0, 0)):
    """drin_attention_mfma_bwd into the given (strided) gradient buffers; dq may be None."""
    delta = torch.full((B, H, Lq), float("nan"), device=DEV)
    _lib.check(_lib.load().drin_attention_mfma_bwd(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(mask), ptr(out),
                                                   out.stride(0), ptr(lse), ptr(dout), dout.stride(0), ptr(dq),
                                                   dq.stride(0) if dq is not None else 0, ptr(dk), dk.stride(0), ptr(dv), dv.stride(0),
                                                   ptr(delta), B, H, Lq, Lk, dh, *drop, stream()))
    return dq, dk, dv


def nan_like(rows, E):
    return torch.full((rows, E), float("nan"), device=DEV)


def run_core(q, k, v, mask, dout, dims, want_dq=True, drop=(0.0, 0, 0)):
    Lq, Lk, dh, H, B = dims
    E = H * dh
    out, lse = mfma_fwd(q, k, v, mask, B, H, Lq, Lk, dh, drop)
    dq, dk, dv = mfma_bwd(q, k, v, mask, out, lse, dout, nan_like(B * Lq, E) if want_dq else None, nan_like(B * Lk, E),
                          nan_like(B * Lk, E), B, H, Lq, Lk, dh, drop)
    return out, lse, dq, dk, dv


# ---- 1. the forward against fp64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", SHAPES)
def test_forward_against_fp64(Lq, Lk, dh, H, B):
    gen = torch.Generator(device=DEV).manual_seed(Lq * 1000 + Lk)
    E = H * dh
    q = torch.randn(B * Lq, E, device=DEV, generator=gen)
    kv = torch.randn(B * Lk, 2 * E + 4, device=DEV, generator=gen)    # K | V packed: row stride 2 E + 4 > E
    k, v = kv[:, :E], kv[:, E:2 * E]
    for mname, mask in masks_for(B, Lk).items():
        out, lse = mfma_fwd(q, k, v, mask, B, H, Lq, Lk, dh)
        ref = attention_fp64(q, k, v, mask, B, H, Lq, Lk, dh)
        scale = ref.abs().max().item()
        err = (out.double() - ref).abs().max().item()
        s = (q.double().reshape(B, Lq, H, dh).permute(0, 2, 1, 3) @ k.double().reshape(B, Lk, H, dh).permute(0, 2, 3, 1)) / math.sqrt(dh)
        if mask is not None:
            s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
        ref_lse = torch.logsumexp(s, -1)
        live = torch.isfinite(ref_lse)
        lerr = (lse.double() - ref_lse)[live].abs().max().item() if live.any() else 0.0
        lbound = LSE_TOL * max(1.0, ref_lse[live].abs().max().item() if live.any() else 0.0)
        print(f"mfma_fwd ({Lq},{Lk},{dh},{H},{B}) {mname}: out max err {err:.3e} ratio {err / scale if scale > 0 else 0.0:.3e}; lse max err {lerr:.3e} "
              f"(bound {lbound:.3e})")
        assert torch.isfinite(out).all()
        assert err <= OUT_TOL * scale, (mname, err, scale)
        assert lerr <= lbound
        assert torch.equal(lse[~live], ref_lse[~live].float())         # exactly -inf where no key is kept
        out2, none = mfma_fwd(q, k, v, mask, B, H, Lq, Lk, dh, want_lse=False)
        assert none is None and torch.equal(out2, out)                 # lse = NULL: the same out bits
        if mname == "gone":                                            # the fully masked mention: zero rows, -inf
            assert (~live).sum().item() == H * Lq and (lse[B - 1] == float("-inf")).all()
            assert not out[(B - 1) * Lq:].any()


# ---- 2. the backward against fp64 autograd -----------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", SHAPES)
def test_backward_against_fp64(Lq, Lk, dh, H, B):
    dims = (Lq, Lk, dh, H, B)
    gen, q, k, v, dout = operands(*dims)
    for mname, mask in bwd_masks(B, Lk, gen).items():
        _out, _lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)
        refs, scales = fp64_gradients(q, k, v, mask, dout, dims)
        for name, got, ref, scale in zip(("dq", "dk", "dv"), (dq, dk, dv), refs, scales):
            err = (got.double() - ref).abs().max().item()
            print(f"mfma_bwd ({Lq},{Lk},{dh},{H},{B}) {mname} {name}: max err {err:.3e} scale {scale:.3e} "
                  f"ratio {err / scale if scale > 0 else 0.0:.3e}")
            assert torch.isfinite(got).all()
            if scale == 0:
                assert not got.any()
            else:
                assert err <= CORE_GRAD_TOL * scale, (mname, name, err, scale)


# ---- 3. contracts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,dh,H,B", CONTRACT_SHAPES)
def test_contracts(Lq, Lk, dh, H, B):
    dims = (Lq, Lk, dh, H, B)
    E = H * dh
    gen, q, k, v, dout = operands(*dims)
    for mname, mask in bwd_masks(B, Lk, gen).items():
        out, lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)                  # outputs prefilled with NaN
        assert all(torch.isfinite(t).all() for t in (out, dq, dk, dv)), "written, not accumulated"
        out2, lse2, dq2, dk2, dv2 = run_core(q, k, v, mask, dout, dims)
        assert torch.equal(out, out2) and torch.equal(lse, lse2), "two runs are bit-equal"
        assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "two runs are bit-equal"
        _o, _l, none, dk3, dv3 = run_core(q, k, v, mask, dout, dims, want_dq=False)
        assert none is None and torch.equal(dk, dk3) and torch.equal(dv, dv3), "dq = NULL changes no bit of dk / dv"
        # dK | dV in one [rows, 2 E + 4] buffer prefilled with 7: only their columns change, same bits
        packed = torch.full((B * Lk, 2 * E + 4), 7.0, device=DEV)
        mfma_bwd(q, k, v, mask, out, lse, dout, None, packed[:, :E], packed[:, E:2 * E], B, H, Lq, Lk, dh)
        assert torch.equal(packed[:, :E], dk) and torch.equal(packed[:, E:2 * E], dv) and (packed[:, 2 * E:] == 7.0).all()
        wide = torch.full((B * Lq, E + 3), 7.0, device=DEV)
        mfma_bwd(q, k, v, mask, out, lse, dout, wide[:, :E], nan_like(B * Lk, E), nan_like(B * Lk, E), B, H, Lq, Lk, dh)
        assert torch.equal(wide[:, :E], dq) and (wide[:, E:] == 7.0).all()
        wide_out = torch.full((B * Lq, E + 3), 7.0, device=DEV)
        _lib.check(_lib.load().drin_attention_mfma_fwd(ptr(q), E, ptr(k), E, ptr(v), E, ptr(mask), ptr(wide_out), E + 3, None, B, H, Lq,
                                                       Lk, dh, 0.0, 0, 0, stream()))
        assert torch.equal(wide_out[:, :E], out) and (wide_out[:, E:] == 7.0).all()
        # strided q / k / v / dout views change no bit
        qw, gw = (torch.randn(B * Lq, E + 8, device=DEV, generator=gen) for _ in range(2))
        kvw = torch.randn(B * Lk, 2 * E + 4, device=DEV, generator=gen)
        qw[:, 4:4 + E], gw[:, :E], kvw[:, :E], kvw[:, E:2 * E] = q, dout, k, v
        qs, gs, ks, vs = qw[:, 4:4 + E], gw[:, :E], kvw[:, :E], kvw[:, E:2 * E]
        out_s, lse_s = mfma_fwd(qs, ks, vs, mask, B, H, Lq, Lk, dh)
        assert torch.equal(out_s, out) and torch.equal(lse_s, lse)
        dq4, dk4, dv4 = mfma_bwd(qs, ks, vs, mask, out, lse, gs, nan_like(B * Lq, E), nan_like(B * Lk, E), nan_like(B * Lk, E), B, H, Lq,
                                 Lk, dh)
        assert torch.equal(dq, dq4) and torch.equal(dk, dk4) and torch.equal(dv, dv4)
        if mask is not None:                                                        # a dropped key's rows are exactly 0
            dropped = (mask == 0).reshape(-1)
            assert not dk[dropped].any() and not dv[dropped].any()
        if mname == "gone":                                                         # the fully masked mention: exactly 0
            assert not dq[(B - 1) * Lq:].any() and not dk[(B - 1) * Lk:].any() and not dv[(B - 1) * Lk:].any()
            assert dv[:(B - 1) * Lk].any()


def test_autograd_core_routes_to_the_entry_points_and_counts_as_attn():
    """attention_core(core="mfma") / attention_core_packed are the two entry points and nothing else (same bits, views read in
    place), and their launches count under profiler class attn: forward, delta, dq, dkv."""
    dims = Lq, Lk, dh, H, B = (12, 3, 8, 2, 5)
    E = H * dh
    gen, q, k, v, dout = operands(*dims)
    mask = bwd_masks(B, Lk, gen)["random"]
    _lib.profile_begin()
    out, _lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims)
    prof = _lib.profile_end()
    assert prof["attn"][1] == 4 and sum(n for _ms, n in prof.values()) == 4, prof
    leaves = [t.reshape(B, -1, E).clone().requires_grad_(True) for t in (q, k, v)]
    got = attention_core(*leaves, mask, H, core="mfma")
    grads = torch.autograd.grad(got, leaves, dout.reshape(B, Lq, E))
    assert torch.equal(got.reshape(-1, E), out)
    assert all(torch.equal(g.reshape(-1, E), r) for g, r in zip(grads, (dq, dk, dv)))
    kv = torch.cat([k, v], 1).reshape(B, Lk, 2 * E).requires_grad_(True)
    got = attention_core_packed(leaves[0].detach(), kv, mask, H, core="mfma")      # q needs no gradient: dq is skipped
    (gkv,) = torch.autograd.grad(got, [kv], dout.reshape(B, Lq, E))
    assert torch.equal(got.reshape(-1, E), out) and torch.equal(gkv.reshape(-1, 2 * E), torch.cat([dk, dv], 1))
    fma = attention_core(*leaves, mask, H)                                         # the default core is another kernel
    assert not torch.equal(fma, attention_core(*leaves, mask, H, core="mfma"))
    with pytest.raises(ValueError, match="core"):
        attention_core(*leaves, mask, H, core="wmma")


# ---- 4. dropout -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,Lq,Lk,dh", [(2, 2, 5, 7, 8), (2, 2, 17, 70, 5), (1, 2, 9, 40, 256)])
def test_dropout_against_fp64_with_the_host_mask(B, H, Lq, Lk, dh, p):
    dims = (Lq, Lk, dh, H, B)
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
    out, lse, dq, dk, dv = run_core(q, k, v, mask, dout, dims, drop=(p, seed, call))
    tag = f"mfma dropout ({B},{H},{Lq},{Lk},{dh}) p={p}"
    err, scale = (out.double() - out64.detach()).abs().max().item(), out64.abs().max().item()
    print(f"{tag} out: max err {err:.3e} ratio {err / scale:.3e}")
    assert err <= OUT_TOL * scale
    # the gradient scale with absolute values at the cancelling step, under the mask (fp64_gradients' rule)
    heads = lambda t: t.detach().abs().reshape(B, -1, H, dh).permute(0, 2, 1, 3)   # noqa: E731
    pw = restate.core_weights(leaves[0].detach().reshape(B, Lq, E), leaves[1].detach().reshape(B, Lk, E), mask, H)
    m = keep.double() / (1.0 - p)
    a = (heads(dout.double()) @ heads(leaves[2]).transpose(-1, -2)) * m
    ds_abs = pw * (a + (pw * a).sum(-1, keepdim=True)) / math.sqrt(dh)
    scales = [(ds_abs @ heads(leaves[1])).max().item(), (ds_abs.transpose(-1, -2) @ heads(leaves[0])).max().item(),
              ((pw * m).transpose(-1, -2) @ heads(dout.double())).max().item()]
    for name, g, r, sc in zip(("dq", "dk", "dv"), (dq, dk, dv), refs, scales):
        gerr = (g.double() - r).abs().max().item()
        print(f"{tag} {name}: max err {gerr:.3e} scale {sc:.3e} ratio {gerr / sc:.3e}")
        assert torch.isfinite(g).all() and gerr <= CORE_GRAD_TOL * sc, name
    gone = (mask == 0).reshape(B * Lk)
    assert not dk[gone].any() and not dv[gone].any()                  # a dropped key: exactly-zero rows
    plain = run_core(q, k, v, mask, dout, dims)
    assert torch.equal(lse, plain[1])                                 # lse is that of the undropped scores
    zero = run_core(q, k, v, mask, dout, dims, drop=(0.0, seed, call))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(zero, plain))    # p = 0: the undropped bits, whatever seed and call are
    again = run_core(q, k, v, mask, dout, dims, drop=(p, seed, call))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(again, (out, lse, dq, dk, dv)))
    other = run_core(q, k, v, mask, dout, dims, drop=(p, seed, call + 1))
    assert not torch.equal(other[0], out)


# ---- 5. the module -----------------------------------------------------------------------------------------------
def module_case(B, Lq, Lk, E, kdim, H, precision):
    """module_case of tests/test_gpu_attention_train.py with core="mfma": the same draws"""
    gen = torch.Generator(device=DEV).manual_seed(B * 100 + Lq + Lk + E)
    torch.manual_seed(E + H)
    mha = MultiheadAttention(E, H, kdim=kdim, vdim=kdim, batch_first=True, precision=precision, core="mfma").to(DEV)
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


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,Lq,Lk,E,kdim,H", MODULE_SHAPES)
def test_module_against_fp64(B, Lq, Lk, E, kdim, H, precision):
    """section 16's four module cases at its bars for the projections' precision, with the split-bf16 core between them"""
    mha, query, key, proj, masks = module_case(B, Lq, Lk, E, kdim, H, precision)
    mha.train()
    for mname, mask in masks.items():
        out, grads = module_grads(mha, query, key, proj, mask)
        ref_out, ref_grads = reference_grads(mha, query, key, proj, mask)
        err = ((out.double() - ref_out).abs().max() / ref_out.abs().max()).item()
        print(f"mha mfma ({B},{Lq},{Lk},{E},{kdim},{H}) {precision} {mname} out: {err:.3e}")
        assert err <= TOL[precision]
        assert sorted(grads) == sorted(ref_grads)
        for name, ref in ref_grads.items():
            rel = ((grads[name].double() - ref).abs().max() / ref.abs().max()).item()
            print(f"mha mfma ({B},{Lq},{Lk},{E},{kdim},{H}) {precision} {mname} d {name}: {rel:.3e}")
            assert rel < GRAD_TOL, (name, rel)
        _out2, again = module_grads(mha, query, key, proj, mask)                     # two backward passes: the same bits
        assert all(torch.equal(grads[n], again[n]) for n in grads)


@pytest.mark.parametrize("B,Lq,Lk,E,kdim,H", MODULE_SHAPES[:3])
def test_module_eval_is_the_hand_composition(B, Lq, Lk, E, kdim, H):
    """eval() under no_grad: drin_linear_fwd -> drin_attention_mfma_fwd -> drin_linear_fwd composed by hand, bit for bit"""
    mha, query, key, _proj, masks = module_case(B, Lq, Lk, E, kdim, H, "bf16x3")
    mask = masks["random"]
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
        ctx, _l = mfma_fwd(linear(xq, w[:E], bias[:E]), kv[:, :E], kv[:, E:], keep, B, H, Lq, Lk, E // H)
    else:
        ctx, _l = mfma_fwd(linear(xq, mha.q_proj_weight.detach(), bias[:E]), linear(xk, mha.k_proj_weight.detach(), bias[E:2 * E]),
                           linear(xk, mha.v_proj_weight.detach(), bias[2 * E:]), keep, B, H, Lq, Lk, E // H)
    want = linear(ctx, mha.out_proj.weight.detach(), mha.out_proj.bias.detach()).reshape(B, Lq, E)
    assert torch.equal(got, want)                                      # the same launches: the same bits


# ---- 6. the models -------------------------------------------------------------------------------------------------
def multimodal_model(name, precision, **kwargs):
    from tests.test_gpu_ghmfc_train import CASES, as_tensors, cfg_for, geometry, ghmfc_inputs
    cfg, arrays, H = cfg_for(name), ghmfc_inputs(name), geometry(name)["H"]
    torch.manual_seed(CASES[name]["seed"])
    model = TrainableModel(cfg, precision=precision, dropout=0.0, **kwargs).to(DEV).train()
    return model, as_tensors(arrays, torch.float32, DEV), (arrays, H)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_multimodal_model_with_the_mfma_core(precision):
    from tests import test_gpu_ghmfc_train as t
    name = "wd_b5"
    model, batch, (arrays, H) = multimodal_model(name, precision, core="mfma")
    scores = model(batch)
    G = t.grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    ref_scores, ref_grads, _pt, _pv = t.reference_at_library_indices(model, arrays, H, G)
    t.check_against_reference(f"{name} {precision} mfma", model, scores, ref_scores, ref_grads, precision)
    # the default core: the bits of a model built without the argument; the mfma core: other kernels
    plain, _b, _ = multimodal_model(name, precision)
    named, _b, _ = multimodal_model(name, precision, core="fma")
    with torch.no_grad():
        assert torch.equal(plain(batch), named(batch)) and not torch.equal(plain(batch), scores)


def variant_model(name, precision, rows=None, **kwargs):
    from tests import test_gpu_ghmfc_variants as t
    arrays = t.variant_inputs(name)
    if rows is not None:
        arrays = [a[rows] if isinstance(a, np.ndarray) else a for a in arrays]
    torch.manual_seed(t.case_of(name)["seed"])
    model = VariantModel(variant_cfg(name), precision=precision, **kwargs).to(DEV)
    return model, t.as_tensors(arrays, torch.float32, DEV), arrays


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_transformer_model_with_the_mfma_core(p, precision):
    from tests import test_gpu_ghmfc_variants as t
    name = "tr_max_b3"
    model, batch, arrays = variant_model(name, precision, dropout=p, seed=21, core="mfma")
    model.train()
    scores = model(batch)
    G = t.grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    keeps = t.stream_keeps(model, p) if p > 0 else None
    ref_scores, ref_grads, pre = t.reference_at_library_indices(model, arrays, name, G, keeps, p)
    t.check_against_reference(f"{name} {precision} mfma dropout {p}", model, scores, ref_scores, ref_grads, precision)
    plain, _b, _a = variant_model(name, precision, dropout=p, seed=21)
    named, _b, _a = variant_model(name, precision, dropout=p, seed=21, core="fma")
    with torch.no_grad():
        a, b = plain.train()(batch), named.train()(batch)
        assert torch.equal(a, b) and not torch.equal(a, scores)
        a, b = plain.eval()(batch), named.eval()(batch)
        assert torch.equal(a, b) and not torch.equal(a, model.eval()(batch))   # eval() of the variant runs the chosen core too
