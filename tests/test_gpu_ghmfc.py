"""GHMFC scoring on the MI355X: drin_attention against fp64 softmax attention, drin_ghmfc_forward against the reference's
goldens and the fp64 restatement in both precisions, the C ABI's write footprint and refusals, and a test epoch through
MELRunner.  Bars: scores within 1e-4 (bf16x3) / 1e-5 (f32), mention_repr the same relative to max|ref| (DESIGN.md section 15
has the measured maxima)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.config import wikidiverse_config
from drin_amd.metrics import TopkAccuracy, TripletLoss
from drin_amd.train import MELRunner
from tests.ghmfc_inputs import ALL_ZERO_ROW, CASES, ghmfc_inputs, geometry
from tests.ghmfc_restatement import ghmfc_scores
from tests.test_ghmfc_host import as_tensors, case_model, compare, golden_of

pytestmark = pytest.mark.gpu

TOL = {"bf16x3": 1e-4, "f32": 1e-5}
DEV = "cuda"
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731


# ---- drin_attention alone -------------------------------------------------------------------------------
def attention(q, k, v, mask, B, H, Lq, Lk, dh, out=None):
    """q [B Lq, >= E], k, v [B Lk, >= E] (views with their own row strides)."""
    E = H * dh
    out = torch.full((B * Lq, E), float("nan"), device=DEV) if out is None else out
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().drin_attention(ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(mask), ptr(out),
                                          out.stride(0), B, H, Lq, Lk, dh, stream))
    return out


def attention_fp64(q, k, v, mask, B, H, Lq, Lk, dh):
    q, k, v = (t.double().reshape(B, -1, H, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    w = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)              # a row with no kept key: zero weights
    return (w @ v).permute(0, 2, 1, 3).reshape(B * Lq, H * dh)


def masks_for(B, Lk):
    one = lambda pos: torch.zeros(B, Lk, dtype=torch.int64, device=DEV).index_fill_(1, torch.tensor([pos], device=DEV), 1)   # noqa: E731
    gone = torch.ones(B, Lk, dtype=torch.int64, device=DEV)
    gone[B - 1] = 0                                                   # one mention fully masked
    return {"null": None, "ones": torch.ones(B, Lk, dtype=torch.int64, device=DEV), "first": one(0), "last": one(Lk - 1), "gone": gone}


@pytest.mark.parametrize("Lq,Lk,dh,H,B", [(1, 1, 1, 1, 1), (3, 1, 5, 4, 2), (12, 3, 8, 2, 5), (49, 128, 256, 8, 2), (128, 49, 96, 8, 2),
                                          (7, 65, 9, 4, 3), (2, 512, 16, 2, 2), (130, 200, 96, 1, 1)])
def test_attention_against_fp64(Lq, Lk, dh, H, B):
    gen = torch.Generator(device=DEV).manual_seed(Lq * 1000 + Lk)
    E = H * dh
    q = torch.randn(B * Lq, E, device=DEV, generator=gen)
    kv = torch.randn(B * Lk, 2 * E + 4, device=DEV, generator=gen)    # K | V packed: row stride 2 E + 4 > E
    forms = {"packed": (kv[:, :E], kv[:, E:2 * E]), "plain": (kv[:, :E].contiguous(), kv[:, E:2 * E].contiguous())}
    for mname, mask in masks_for(B, Lk).items():
        ref = attention_fp64(q, forms["plain"][0], forms["plain"][1], mask, B, H, Lq, Lk, dh)
        scale = ref.abs().max().item()
        outs = []
        for fname, (k, v) in forms.items():
            got = attention(q, k, v, mask, B, H, Lq, Lk, dh)
            again = attention(q, k, v, mask, B, H, Lq, Lk, dh)
            err = (got.double() - ref).abs().max().item()
            print(f"attention ({Lq},{Lk},{dh},{H},{B}) {mname} {fname}: max err {err:.3e} (max |ref| {scale:.3e})")
            assert torch.isfinite(got).all() and err <= 1e-5 * scale
            assert torch.equal(got, again)
            outs.append(got)
        assert torch.equal(outs[0], outs[1])                          # the operands' strides change no bit
        if mname == "gone":
            assert torch.equal(outs[0][(B - 1) * Lq:], torch.zeros(Lq, E, device=DEV))   # exactly 0


def test_attention_writes_only_its_columns():
    B, H, Lq, Lk, dh = 2, 3, 5, 7, 5
    E = H * dh
    q, k, v = (torch.randn(B * n, E, device=DEV) for n in (Lq, Lk, Lk))
    out = torch.full((B * Lq, E + 3), 7.0, device=DEV)
    attention(q, k, v, None, B, H, Lq, Lk, dh, out=out)
    assert torch.equal(out[:, E:], torch.full((B * Lq, 3), 7.0, device=DEV)) and not (out[:, :E] == 7.0).any()


# ---- the whole model ------------------------------------------------------------------------------------
def run_case(name, precision, restate=True):
    g = golden_of(name)
    model = case_model(name, precision).to(DEV)
    batch = as_tensors(ghmfc_inputs(name), torch.float32, DEV)
    with torch.no_grad():
        scores, mention = model(batch), model.encode_mentions(batch)
        same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))   # noqa: E731
        assert same(scores, model(batch))                             # the same bits every run (NaN where the golden has NaN)
        assert not scores.requires_grad and not mention.requires_grad
    compare(scores, g[f"{name}/scores"], TOL[precision] / max(np.nanmax(np.abs(g[f"{name}/scores"])), 1e-30), f"{name} {precision} scores vs golden")
    compare(mention, g[f"{name}/mention_repr"], TOL[precision], f"{name} {precision} mention_repr vs golden")
    if restate:
        sd = {k: v.double() for k, v in model.state_dict().items()}
        with torch.no_grad():
            ref, ref_m = ghmfc_scores(as_tensors(ghmfc_inputs(name), torch.float64, DEV), sd, geometry(name)["H"], return_mention=True)
        compare(scores, ref.cpu(), TOL[precision] / max(np.nanmax(np.abs(ref.cpu().numpy())), 1e-30), f"{name} {precision} scores vs fp64")
        compare(mention, ref_m.cpu(), TOL[precision], f"{name} {precision} mention_repr vs fp64")
    return scores


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["wd_b1", "wd_b5", "wm_b3"])
def test_tiny_cases(name, precision):
    scores = run_case(name, precision)
    if name == "wd_b5":
        assert torch.isfinite(scores[ALL_ZERO_ROW]).all()             # the all-zero mask: zero weights, not NaN


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["heads_5_9", "ones", "long_200", "long_512", "b300"])
def test_shape_cases(name, precision):
    run_case(name, precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["full_b4", "full_b64"])
def test_full_width(name, precision):
    run_case(name, precision, restate=name == "full_b4")


# ---- C ABI ----------------------------------------------------------------------------------------------
def test_forward_writes_only_its_outputs_and_workspace():
    name, lib = "wd_b5", _lib.load()
    g, geo = golden_of(name), geometry(name)
    model = case_model(name, "f32").to(DEV)
    mf, mmask, _, _, mimage, ef, _, _ = as_tensors(ghmfc_inputs(name), torch.float32, DEV)
    B, N, D = 5, geo["N"], geo["D"]
    c = _lib.DrinGhmfcConfigC(batch=B, num_candidates=N, embed_dim=D, image_dim=geo["R"], mention_tokens=geo["L"],
                              image_regions=geo["P"], num_heads=geo["H"], entity_tokens=0, precision=_lib.PREC_F32,
                              layer_norm_eps=1e-5, cosine_eps=1e-8)
    params = [p.detach().contiguous() for p in model.param_list()]
    pc = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[p.data_ptr() for p in params]))
    bt = _lib.DrinGhmfcBatchC(ptr(mf), ptr(mmask), ptr(mimage), ptr(ef), None)
    nbytes = lib.drin_ghmfc_workspace_bytes(C.byref(c))
    assert nbytes > 0 and nbytes % 16 == 0
    G = 4096                                                            # guard bytes on both sides of every written buffer

    def guarded(n):
        buf = torch.full((G + n + G,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[G:G + n]

    ws_buf, ws = guarded(nbytes)
    sc_buf, sc = guarded(B * N * 4)
    mr_buf, mr = guarded(B * D * 4)
    intact = lambda buf, n: bool((buf[:G] == 0xA5).all() and (buf[G + n:] == 0xA5).all())   # noqa: E731
    call = lambda size, rep: lib.drin_ghmfc_forward(C.byref(c), C.byref(bt), C.byref(pc), ptr(ws), size, ptr(sc), rep, None)   # noqa: E731
    assert call(nbytes, ptr(mr)) == _lib.OK
    torch.cuda.synchronize()
    assert intact(ws_buf, nbytes) and intact(sc_buf, B * N * 4) and intact(mr_buf, B * D * 4)
    scores = sc.view(torch.float32).reshape(B, N).clone()
    compare(scores, g[f"{name}/scores"], 1e-5 / np.abs(g[f"{name}/scores"]).max(), "C ABI scores")
    compare(mr.view(torch.float32).reshape(B, D), g[f"{name}/mention_repr"], 1e-5, "C ABI mention_repr")
    # a NULL mention_repr is accepted and changes no score
    sc.fill_(0)
    assert call(nbytes, None) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(sc.view(torch.float32).reshape(B, N), scores) and intact(ws_buf, nbytes)
    # refusals: nothing is launched, nothing is written
    sc.fill_(0x5A)
    ws.fill_(0x5A)
    assert call(nbytes - 4, None) == _lib.E_WORKSPACE
    c.embed_dim = 18
    assert call(nbytes, None) == _lib.E_SHAPE
    c.embed_dim, c.mention_tokens = D, 513
    assert call(nbytes, None) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((sc == 0x5A).all()) and bool((ws == 0x5A).all())


# ---- the evaluation path ----------------------------------------------------------------------------------
def test_test_epoch_matches_the_restatement():
    name = "wd_b5"
    geo = geometry(name)
    cfg = wikidiverse_config(metrics_topk=(1, 2))
    model = case_model(name, "f32").to(DEV)
    sd = {k: v.double() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    loader, loss64, total = [], [], 0
    meters = [TopkAccuracy(k) for k in cfg.metrics_topk]
    crit = TripletLoss(cfg.triplet_margin)
    for _ in range(3):
        B = 5
        mf, mmask, begin, end, mimage, ef, _, _ = as_tensors(ghmfc_inputs(name), torch.float32)
        mf = mf + 0.5 * torch.randn(mf.shape, generator=gen)
        ef = ef + 0.5 * torch.randn(ef.shape, generator=gen)
        answer = torch.eye(geo["N"] - 1, dtype=torch.int8)[torch.randint(0, geo["N"] - 1, (B,), generator=gen)]
        zeros = torch.zeros(B, dtype=torch.int64)                       # what the loader's collate makes of the scalar 0 items
        batch = [mf, mmask, begin, end, mimage, ef, zeros, zeros, answer]
        loader.append(batch)
        with torch.no_grad():
            ref = ghmfc_scores([t.double() if t.is_floating_point() else t for t in batch[:8]], {k: v.cpu() for k, v in sd.items()}, geo["H"])
        loss64.append(crit(answer, ref).item())
        for m in meters:
            m.update(ref, answer)
        total += B
    log = MELRunner(cfg, model, DEV).test(loader)
    want_topk = [float(m.compute()) / (1 - cfg.acc_correction[2]) for m in meters]
    print(f"test epoch: loss {log.loss:.7f} vs {np.mean(loss64):.7f}, top-k {log.topk} vs {want_topk}")
    assert abs(log.loss - np.mean(loss64)) <= 1e-5
    assert np.allclose(log.topk, want_topk, rtol=0, atol=1e-5)
    assert model.training is False
