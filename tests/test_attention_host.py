"""The trainable attention without a GPU: the restatement (tests/attention_restatement.py) against torch's own
nn.MultiheadAttention in float64, the module's parameters against torch's under one seed, every refusal of
drin_amd.attention.MultiheadAttention, and the host-side validation of every attention entry point of both cores."""
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


# entry-point family -> (forward, backward or None, takes a dropout rate, the forward's lse: "required" | "optional" | None)
FAMILIES = {"plain": ("drin_attention", None, False, None),
            "train": ("drin_attention_train_fwd", "drin_attention_bwd", False, "required"),
            "dropout": ("drin_attention_dropout_fwd", "drin_attention_dropout_bwd", True, "required"),
            "mfma": ("drin_attention_mfma_fwd", "drin_attention_mfma_bwd", True, "optional")}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_entry_points_validate_on_host(family):
    """Every check of the attention front (csrc/attention_api.hip) through every entry point that has it: the same code and an
    error text with the entry point's name, whichever core is behind it."""
    lib = _lib.load()
    fwd_name, bwd_name, has_rate, fwd_lse = FAMILIES[family]
    one = C.c_void_p(16)   # never dereferenced: every check below fails before a launch

    def fwd(q=one, out=one, lse=one, Lk=8, dh=16, ldq=64, ldo=64, p=0.0, B=2, H=4):
        rate = (p, 1, 2) if has_rate else ()
        lse = () if fwd_lse is None else (lse,)
        return getattr(lib, fwd_name)(q, ldq, one, 64, one, 64, None, out, ldo, *lse, B, H, 7, Lk, dh, *rate, None)

    def bwd(q=one, lse=one, dout=one, dq=one, dk=one, dv=one, delta=one, Lk=8, dh=16, ldk=64, lddo=64, lddq=64, lddv=64, p=0.0, B=2,
            H=4):
        rate = (p, 1, 2) if has_rate else ()
        return getattr(lib, bwd_name)(q, 64, one, ldk, one, 64, None, one, 64, lse, dout, lddo, dq, lddq, dk, 64, dv, lddv, delta,
                                      B, H, 7, Lk, dh, *rate, None)

    def refused(name, status, code, *words):
        error = lib.drin_last_error()
        assert status == code, (name, status, error)
        for word in (name,) + words:
            assert word.encode() in error, (name, word, error)

    for name, call in ((fwd_name, fwd),) + (((bwd_name, bwd),) if bwd_name else ()):
        refused(name, call(q=None), _lib.E_NULL)
        refused(name, call(Lk=0), _lib.E_SHAPE)
        refused(name, call(Lk=513), _lib.E_SHAPE, "k_len")
        refused(name, call(dh=257), _lib.E_SHAPE, "head_dim")
        for bad in (dict(dh=0), dict(B=0), dict(B=65536), dict(H=65536)):
            refused(name, call(**bad), _lib.E_SHAPE)
        if has_rate:
            for p in (1.0, -0.1, float("nan")):
                refused(name, call(p=p), _lib.E_SHAPE, "dropout rate")
            refused(name, call(p=1.0, q=None, Lk=513), _lib.E_SHAPE, "dropout rate")    # the rate is looked at first
    refused(fwd_name, fwd(out=None), _lib.E_NULL)
    refused(fwd_name, fwd(ldq=63), _lib.E_SHAPE, "ldq")
    refused(fwd_name, fwd(ldo=63), _lib.E_SHAPE, "ldo")
    if fwd_lse == "required":
        refused(fwd_name, fwd(lse=None), _lib.E_NULL)
    elif fwd_lse == "optional":                           # accepted: the next check is the one that reports
        refused(fwd_name, fwd(lse=None, ldo=63), _lib.E_SHAPE, "ldo")
    if bwd_name is None:
        return
    for missing in ("lse", "dout", "delta"):
        refused(bwd_name, bwd(**{missing: None}), _lib.E_NULL)
    refused(bwd_name, bwd(ldk=63), _lib.E_SHAPE, "ldk")
    refused(bwd_name, bwd(lddo=63), _lib.E_SHAPE, "lddo")
    refused(bwd_name, bwd(lddq=63), _lib.E_SHAPE, "lddq")
    refused(bwd_name, bwd(lddv=63), _lib.E_SHAPE, "lddv")
    refused(bwd_name, bwd(dq=None, lddq=0, Lk=513), _lib.E_SHAPE)       # dq may be NULL (its stride is then not read) ...
    refused(bwd_name, bwd(dq=None, lddq=0, ldk=63), _lib.E_SHAPE, "ldk")
    refused(bwd_name, bwd(dv=None), _lib.E_NULL, "dk and dv")          # ... dk without dv may not
    refused(bwd_name, bwd(dk=None), _lib.E_NULL, "dk and dv")
    assert bwd(dq=None, dk=None, dv=None) == _lib.OK                    # nothing asked for: nothing launched
    assert bwd(dq=None, dk=None, dv=None, lddq=0, lddv=0) == _lib.OK    # ... and the absent gradients' strides are not read
    assert lib.drin_version() == _lib.ABI_VERSION == 12
