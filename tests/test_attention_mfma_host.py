"""The matrix-core attention core without a GPU: the two entry points in the library and in the ctypes
mirror (their host-side validation: tests/test_attention_host.py), the `core` argument of every layer above them, the shim's DRIN_ATTENTION_CORE, and the
arithmetic scheme itself: an fp64 emulation of the three-pass split-bf16 products (operands rounded to hi + lo, the lo lo
pass dropped, P and dS split as well) against exact fp64 on the shape list of tests/test_gpu_attention_mfma.py.  The scheme
alone must stay under a quarter of each bar of that file, so that a miss on the GPU means the kernel, not the scheme."""
import ctypes as C
import inspect
import math

import pytest
import torch

from drin_amd import _lib, attention
from drin_amd.attention import MultiheadAttention, attention_core, attention_core_packed, multihead_attention_forward
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantModel
from tests import attention_restatement as restate
from tests.test_ghmfc_host import cfg_for
from tests.test_ghmfc_variants_host import bind, reference_args, variant_cfg
from tests.test_gpu_attention_train import fp64_gradients

SHAPES = [(1, 1, 1, 1, 1), (3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (15, 17, 32, 2, 2), (16, 16, 36, 1, 2), (17, 15, 4, 2, 2),
          (63, 65, 64, 1, 2), (65, 33, 132, 1, 1), (49, 128, 256, 8, 2), (128, 49, 96, 8, 2), (2, 512, 16, 2, 2), (130, 200, 96, 1, 1)]
OUT_TOL, LSE_TOL, CORE_GRAD_TOL = 1e-4, 1e-4, 2e-4       # the bars of tests/test_gpu_attention_mfma.py


def test_symbols_are_exported_and_mirrored():
    lib = _lib.load()
    for name in ("drin_attention_mfma_fwd", "drin_attention_mfma_bwd"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
    assert len(lib.drin_attention_mfma_fwd.argtypes) == len(lib.drin_attention_dropout_fwd.argtypes) == 19
    assert list(lib.drin_attention_mfma_fwd.argtypes) == list(lib.drin_attention_dropout_fwd.argtypes)
    assert list(lib.drin_attention_mfma_bwd.argtypes) == list(lib.drin_attention_dropout_bwd.argtypes)
    assert lib.drin_version() == _lib.ABI_VERSION == 12


def test_core_argument_defaults_and_refusals():
    for fn in (attention_core, attention_core_packed, multihead_attention_forward, MultiheadAttention.__init__, TrainableModel.__init__,
               VariantModel.__init__, VariantModel.__new__):
        assert inspect.signature(fn).parameters["core"].default == "fma", fn
    assert attention.CORES == ("fma", "mfma")
    assert MultiheadAttention(8, 2, batch_first=True).core == "fma"
    assert MultiheadAttention(8, 2, batch_first=True, core="mfma", precision="f32").core == "mfma"   # independent of the precision
    with pytest.raises(ValueError, match="core"):
        MultiheadAttention(8, 2, batch_first=True, core="wmma")
    x = torch.zeros(2, 3, 8)
    for call in (lambda: attention_core(x, x, x, None, 2, core="tensor"), lambda: attention_core_packed(x, torch.zeros(2, 3, 16), None, 2, core=""),
                 lambda: TrainableModel(cfg_for("wd_b1"), core="MFMA"), lambda: VariantModel(variant_cfg("tr_max_b3"), core="x")):
        with pytest.raises(ValueError, match="core"):                 # refused before any tensor is looked at
            call()
    with pytest.raises(RuntimeError, match="GPU only"):               # an accepted core: next is the device check
        attention_core(x, x, x, None, 2, core="mfma")
    assert "split-bf16" in attention_core.__doc__ and "not exact" in attention_core.__doc__


def attentions_of(model):
    return [m for m in model.modules() if isinstance(m, MultiheadAttention)]


def test_models_hand_the_core_to_every_attention():
    m = TrainableModel(cfg_for("wd_b1"), core="mfma")
    assert m.core == "mfma" and len(attentions_of(m)) == 4 and all(a.core == "mfma" for a in attentions_of(m))
    assert all(a.core == "fma" for a in attentions_of(TrainableModel(cfg_for("wd_b1"))))
    text = VariantModel(variant_cfg("text_max_b3"), core="mfma")
    assert text.core == "mfma" and attentions_of(text) and all(a.core == "mfma" for a in attentions_of(text))
    tr = VariantModel(variant_cfg("tr_max_b3"), core="mfma")         # its self-attentions go through multihead_attention_forward
    assert tr.core == "mfma" and VariantModel(variant_cfg("tr_max_b3")).core == "fma"
    assert 'core=self.core' in inspect.getsource(VariantModel._transformer)


@pytest.mark.parametrize("final_layer,kind", [("multimodal", TrainableModel), ("transformer", VariantModel)])
def test_shim_honours_the_environment(monkeypatch, final_layer, kind):
    ghmfc_shim = bind(monkeypatch, reference_args(mention_final_layer_name=final_layer))
    monkeypatch.delenv("DRIN_ATTENTION_CORE", raising=False)
    m = ghmfc_shim.Model()
    assert isinstance(m, kind) and m.core == "fma"
    monkeypatch.setenv("DRIN_ATTENTION_CORE", "mfma")
    m = ghmfc_shim.Model()
    assert isinstance(m, kind) and m.core == "mfma" and all(a.core == "mfma" for a in attentions_of(m))
    monkeypatch.setenv("DRIN_ATTENTION_CORE", "fast")
    with pytest.raises(ValueError, match="core"):
        ghmfc_shim.Model()


# ---- the scheme in fp64 ---------------------------------------------------------------------------------------------
def bf16(x):
    return x.float().bfloat16().double()


def split(x):
    hi = bf16(x)
    return hi, bf16(x - hi)


def prod3(a, b):
    """a @ b with both operands as bf16 hi + lo and the lo lo pass dropped, summed in fp64"""
    (ah, al), (bh, bl) = split(a), split(b)
    return ah @ bh + ah @ bl + al @ bh


def emulate(q, k, v, mask, dout, dims):
    """(out, lse, dq, dk, dv) of the kernels' scheme in fp64: [B, H, L, dh] inside, [B L, E] / [B, H, Lq] out"""
    Lq, Lk, dh, H, B = dims
    E = H * dh
    heads = lambda t: t.double().reshape(B, -1, H, dh).permute(0, 2, 1, 3)   # noqa: E731
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(-1, E)                    # noqa: E731
    qh, kh, vh, gh = heads(q), heads(k), heads(v), heads(dout)
    inv = 1.0 / math.sqrt(dh)
    keep = torch.ones(B, 1, 1, Lk, dtype=torch.bool) if mask is None else (mask != 0)[:, None, None, :]
    s2 = prod3((qh.float() * (math.log2(math.e) * inv)).double(), kh.transpose(-1, -2)).masked_fill(~keep, float("-inf"))   # log2 units
    m = s2.max(-1, keepdim=True).values
    live = torch.isfinite(m)
    p = torch.where(live, torch.exp2(s2 - torch.where(live, m, torch.zeros_like(m))), torch.zeros_like(s2))
    l = p.sum(-1, keepdim=True)
    out = torch.where(live, prod3(p, vh) / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(qh))
    lse2 = torch.where(live, m + torch.log2(torch.where(live, l, torch.ones_like(l))), m)
    # backward: p from the unscaled product and the forward's lse, as the kernels recompute it
    sb = prod3(qh, kh.transpose(-1, -2)) * (math.log2(math.e) * inv)
    pb = torch.where(live & keep, torch.exp2(sb - torch.where(live, lse2, torch.zeros_like(lse2))), torch.zeros_like(sb))
    delta = (gh * out).sum(-1, keepdim=True)
    ds = pb * (prod3(gh, vh.transpose(-1, -2)) - delta)
    dq, dk, dv = prod3(ds, kh) * inv, prod3(ds.transpose(-1, -2), qh) * inv, prod3(pb.transpose(-1, -2), gh)
    return rows(out), (lse2 * math.log(2.0)).squeeze(-1), rows(dq), rows(dk), rows(dv)


def scheme_masks(B, Lk, gen):
    rnd = (torch.rand(B, Lk, generator=gen) < 0.6).to(torch.int64)
    rnd[:, Lk // 2] = 1
    gone = torch.ones(B, Lk, dtype=torch.int64)
    gone[B - 1] = 0                                                   # one mention fully masked
    return {"null": None, "random": rnd, "gone": gone}


@pytest.mark.parametrize("Lq,Lk,dh,H,B", SHAPES)
def test_scheme_stays_under_a_quarter_of_each_bar(Lq, Lk, dh, H, B):
    dims = (Lq, Lk, dh, H, B)
    gen = torch.Generator().manual_seed(Lq * 1000 + Lk + dh)
    E = H * dh
    q, k, v, dout = (torch.randn(B * n, E, generator=gen) for n in (Lq, Lk, Lk, Lq))
    for mname, mask in scheme_masks(B, Lk, gen).items():
        out, lse, dq, dk, dv = emulate(q, k, v, mask, dout, dims)
        q3, k3, v3 = (t.double().reshape(B, -1, E) for t in (q, k, v))
        ref_out = restate.attention_core(q3, k3, v3, mask, H).reshape(-1, E)
        s = (q3.reshape(B, Lq, H, dh).permute(0, 2, 1, 3) @ k3.reshape(B, Lk, H, dh).permute(0, 2, 3, 1)) / math.sqrt(dh)
        if mask is not None:
            s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
        ref_lse = torch.logsumexp(s, -1)
        live = torch.isfinite(ref_lse)
        scale = ref_out.abs().max().item()
        err = (out - ref_out).abs().max().item()
        lerr = (lse - ref_lse)[live].abs().max().item() if live.any() else 0.0
        lscale = max(1.0, ref_lse[live].abs().max().item() if live.any() else 0.0)
        print(f"scheme ({Lq},{Lk},{dh},{H},{B}) {mname}: out {err / scale if scale > 0 else 0.0:.2e} lse {lerr / lscale:.2e}")
        assert err <= 0.25 * OUT_TOL * scale and lerr <= 0.25 * LSE_TOL * lscale
        assert torch.equal(lse[~live], ref_lse[~live])                # -inf where no key is kept
        refs, scales = fp64_gradients(q, k, v, mask, dout, dims)
        for name, got, ref, sc in zip(("dq", "dk", "dv"), (dq, dk, dv), refs, scales):
            gerr = (got - ref).abs().max().item()
            print(f"scheme ({Lq},{Lk},{dh},{H},{B}) {mname} {name}: {gerr / sc if sc > 0 else 0.0:.2e}")
            assert gerr <= 0.25 * CORE_GRAD_TOL * sc if sc > 0 else not got.any(), (mname, name, gerr, sc)
