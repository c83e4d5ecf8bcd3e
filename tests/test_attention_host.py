"""The trainable attention without a GPU: the restatement (tests/attention_restatement.py) against torch's own
nn.MultiheadAttention in float64, the module's parameters against torch's under one seed, every refusal of
drin_amd.attention.MultiheadAttention, and the host-side validation of drin_attention_train_fwd / drin_attention_bwd."""
import ctypes as C

import pytest
import torch
from torch import nn

from drin_amd import _lib
from drin_amd.attention import MultiheadAttention
from tests.attention_restatement import multihead_attention

FORMS = {"packed": dict(embed_dim=24, num_heads=4), "kdim": dict(embed_dim=24, num_heads=3, kdim=20, vdim=12)}


def padding_mask(B, Lk, gen):
    """bool [B, Lk], True = drop, about 40 % dropped and at least two keys kept per mention."""
    drop = torch.rand(B, Lk, generator=gen) < 0.4
    drop[:, :2] = False
    return drop


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("masked", [False, True])
def test_restatement_matches_torch_in_fp64(form, masked):
    gen = torch.Generator().manual_seed(5)
    kw = FORMS[form]
    E, kd, vd = kw["embed_dim"], kw.get("kdim", kw["embed_dim"]), kw.get("vdim", kw["embed_dim"])
    B, Lq, Lk = 3, 5, 7
    torch.manual_seed(11)
    mha = nn.MultiheadAttention(batch_first=True, **kw).double().eval()
    with torch.no_grad():
        for p in mha.parameters():                                    # torch draws zero biases: give every tensor a value
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3)
    q, k, v = (torch.randn(B, n, w, generator=gen, dtype=torch.float64) for n, w in ((Lq, E), (Lk, kd), (Lk, vd)))
    proj = torch.randn(B, Lq, E, generator=gen, dtype=torch.float64)
    mask = padding_mask(B, Lk, gen) if masked else None

    def grads(fn, params):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = fn(*leaves)
        return out, torch.autograd.grad((out * proj).sum(), leaves + params)

    names = [n for n, _ in mha.named_parameters()]
    ref_out, ref_g = grads(lambda a, b, c: mha(a, b, c, key_padding_mask=mask, need_weights=False)[0], list(mha.parameters()))
    sd = {n: p.detach().clone().requires_grad_(True) for n, p in mha.named_parameters()}
    got_out, got_g = grads(lambda a, b, c: multihead_attention(sd, a, b, c, mask, kw["num_heads"]), [sd[n] for n in names])
    for name, got, ref in [("out", got_out, ref_out)] + list(zip(["query", "key", "value"] + names, got_g, ref_g)):
        rel = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"{form} masked={masked} {name}: {rel:.2e}")
        assert rel <= 1e-10, (name, rel)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_state_dict_is_torchs_own(form):
    kw = FORMS[form]
    torch.manual_seed(3)
    ref = nn.MultiheadAttention(batch_first=True, **kw)
    torch.manual_seed(3)
    got = MultiheadAttention(batch_first=True, **kw)
    a, b = ref.state_dict(), got.state_dict()
    assert list(a) == list(b)
    for n in a:
        assert a[n].shape == b[n].shape and torch.equal(a[n], b[n]), n
    assert [n for n, _ in ref.named_parameters()] == [n for n, _ in got.named_parameters()]
    assert got.precision == "bf16x3" and MultiheadAttention(8, 2, batch_first=True, precision="f32").precision == "f32"
    got.load_state_dict(a)                                            # and torch's checkpoints load


def test_refusals():
    with pytest.raises(NotImplementedError, match="batch_first"):
        MultiheadAttention(8, 2)
    with pytest.raises(NotImplementedError, match="add_bias_kv"):
        MultiheadAttention(8, 2, batch_first=True, add_bias_kv=True)
    with pytest.raises(NotImplementedError, match="add_zero_attn"):
        MultiheadAttention(8, 2, batch_first=True, add_zero_attn=True)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        MultiheadAttention(6, 2, batch_first=True)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        MultiheadAttention(8, 2, batch_first=True, kdim=10, vdim=8)
    with pytest.raises(ValueError, match="precision"):
        MultiheadAttention(8, 2, batch_first=True, precision="fp16")
    m = MultiheadAttention(8, 2, batch_first=True)
    x = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="GPU only"):               # a CPU batch
        m(x, x, x)
    with pytest.raises(NotImplementedError, match="need_weights"):
        m(x, x, x, need_weights=True)
    with pytest.raises(NotImplementedError, match="attn_mask"):
        m(x, x, x, attn_mask=torch.zeros(3, 3, dtype=torch.bool))
    d = MultiheadAttention(8, 2, dropout=0.1, batch_first=True)
    d.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        d(x, x, x)
    d.eval()
    with pytest.raises(RuntimeError, match="GPU only"):               # eval with dropout passes that check: next is the device
        d(x, x, x)


def test_new_entry_points_validate_on_host():
    lib = _lib.load()
    one = C.c_void_p(16)   # never dereferenced: every check below fails before a launch

    def fwd(q=one, lse=one, Lk=8, dh=16, ldq=64, ldo=64):
        return lib.drin_attention_train_fwd(q, ldq, one, 64, one, 64, None, one, ldo, lse, 2, 4, 7, Lk, dh, None)

    def bwd(q=one, lse=one, dout=one, dq=one, dk=one, dv=one, delta=one, Lk=8, dh=16, ldk=64, lddo=64, lddq=64, lddv=64):
        return lib.drin_attention_bwd(q, 64, one, ldk, one, 64, None, one, 64, lse, dout, lddo, dq, lddq, dk, 64, dv, lddv, delta,
                                      2, 4, 7, Lk, dh, None)

    for call in (fwd, bwd):
        assert call(q=None) == _lib.E_NULL and call(lse=None) == _lib.E_NULL
        assert call(Lk=0) == _lib.E_SHAPE
        assert call(Lk=513) == _lib.E_SHAPE and b"k_len" in lib.drin_last_error()
        assert call(dh=257) == _lib.E_SHAPE and b"head_dim" in lib.drin_last_error()
    assert fwd(ldq=63) == _lib.E_SHAPE and b"ldq" in lib.drin_last_error()
    assert fwd(ldo=63) == _lib.E_SHAPE
    assert bwd(dout=None) == _lib.E_NULL and bwd(delta=None) == _lib.E_NULL
    assert bwd(ldk=63) == _lib.E_SHAPE and b"ldk" in lib.drin_last_error()
    assert bwd(lddo=63) == _lib.E_SHAPE and b"lddo" in lib.drin_last_error()
    assert bwd(lddq=63) == _lib.E_SHAPE and b"lddq" in lib.drin_last_error()
    assert bwd(lddv=63) == _lib.E_SHAPE and b"lddv" in lib.drin_last_error()
    assert bwd(dq=None, lddq=0, Lk=513) == _lib.E_SHAPE               # dq may be NULL (its stride is then not read) ...
    assert bwd(dv=None) == _lib.E_NULL and b"dk and dv" in lib.drin_last_error()   # ... dk without dv may not
    assert bwd(dk=None) == _lib.E_NULL and b"dk and dv" in lib.drin_last_error()
    assert lib.drin_version() == _lib.ABI_VERSION == 12
