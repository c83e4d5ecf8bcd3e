"""MELHI on the MI355X: scores, NaN rows, image masks and parameter gradients of drin_melhi_forward / drin_melhi_backward
against the reference's goldens and the fp64 restatement, run-to-run bit equality of the gradients, an Adam loop that tracks
the restatement's, and the C ABI's refusals with real device buffers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.melhi import MelhiConfig, Model, orders_and_lengths
from tests.melhi_inputs import CASES, FULL, KEYS, TINY, grad_weights, melhi_inputs
from tests.melhi_restatement import melhi_scores

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TINY_CASES = [n for n, c in CASES.items() if not c.get("full") and "geom" not in c]
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
DEV = "cuda"


def cfg_for(g: dict, thres=(0.3, 0.3)) -> MelhiConfig:
    return MelhiConfig(num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"], image_regions=g["P"],
                       thres_tmim=thres[0], thres_imie=thres[1])


def case_model(name: str, precision: str) -> Model:
    case = CASES[name]
    torch.manual_seed(case["seed"])
    m = Model(cfg_for(FULL if case.get("full") else TINY, case.get("thres", (0.3, 0.3))), precision=precision)
    return m.to(DEV)


def to_dev(batch, dtype=torch.float32):
    out = []
    for x in batch:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if isinstance(x, torch.Tensor):
            x = x.to(DEV, dtype if x.is_floating_point() else torch.int64)
        out.append(x)
    return out


def sd64(model):
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def tiny_golden():
    return np.load(os.path.join(GOLDEN, "melhi_tiny.npz"))


def max_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    ok = ~torch.isnan(b)
    return (a[ok] - b[ok]).abs().max().item() if ok.any() else 0.0


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", TINY_CASES)
def test_tiny_cases_match_goldens_and_restatement(name, precision, tiny_golden):
    model = case_model(name, precision)
    batch = to_dev(melhi_inputs(name, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    scores = model(batch)
    torch.cuda.synchronize()
    assert max_err(scores, torch.from_numpy(tiny_golden[f"{name}/scores"])) < TOL[precision]
    sd = sd64(model)
    t1, t2 = CASES[name].get("thres", (0.3, 0.3))
    ref, mask = melhi_scores(to_dev(batch, torch.float64), sd, t1, t2, return_mask=True)
    assert max_err(scores, ref) < TOL[precision]
    assert np.array_equal(mask.cpu().numpy().astype(np.uint8), tiny_golden[f"{name}/mask"])
    if f"{name}/grad/{KEYS[0]}" not in tiny_golden:
        return
    G = torch.from_numpy(grad_weights(name, scores.shape)).to(DEV)
    (scores * G).sum().backward()
    (ref * G.double()).sum().backward()
    params = dict(model.named_parameters())
    for k in KEYS:
        want = torch.from_numpy(tiny_golden[f"{name}/grad/{k}"]).double()
        got = params[k].grad.detach().double().cpu()
        scale = max(want.abs().max().item(), 1e-6)
        assert (got - want).abs().max().item() / scale < 2e-4, (k, "golden")
        r64 = sd[k].grad.detach().cpu() if sd[k].grad is not None else torch.zeros_like(want)
        assert (got - r64).abs().max().item() / scale < 2e-4, (k, "restatement")


@pytest.mark.parametrize("name", ["full_b4", "full_b64"])
def test_full_width_checksums(name):
    full = np.load(os.path.join(GOLDEN, "melhi_full.npz"))
    model = case_model(name, "bf16x3")
    batch = to_dev(melhi_inputs(name, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    scores = model(batch)
    G = torch.from_numpy(grad_weights(name, scores.shape)).to(DEV)
    (scores * G).sum().backward()
    s = scores.detach().double().cpu()
    assert abs(s.sum().item() - full[f"{name}/scores_sum"]) < 1e-4 * s.numel()
    assert (s.flatten()[:32] - torch.from_numpy(full[f"{name}/scores_head"]).double()).abs().max().item() < 1e-4
    params = dict(model.named_parameters())
    for k in KEYS:
        g = params[k].grad.detach().double().cpu()
        want_l2 = float(full[f"{name}/grad_l2/{k}"])
        assert abs(g.norm().item() - want_l2) <= 2e-4 * max(want_l2, 1e-12), k
        head = torch.from_numpy(full[f"{name}/grad_head/{k}"]).double()
        assert (g.flatten()[:16] - head).abs().max().item() <= 2e-4 * max(g.abs().max().item(), 1e-12), k


def big_batch(B: int, g: dict, seed: int):
    """A full-width, tie-heavy batch made on the device (half of the mentions with a left placeholder)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    D, R, L, P, N = g["D"], g["R"], g["L"], g["P"], g["N"]
    mf = torch.randn(B, L, D, device=DEV, generator=gen)
    mimage = torch.randn(B, P, R, device=DEV, generator=gen).abs()
    ef = torch.randn(B, N, D, device=DEV, generator=gen)
    eimage = torch.randn(B, N, R, device=DEV, generator=gen)
    eimage[::2, 1] = mimage[::2].mean(1) + 0.1 * eimage[::2, 1]
    s = torch.randint(0, 4, (B,), device=DEV, generator=gen) * (torch.rand(B, device=DEV, generator=gen) < 0.5)
    e = s + 1
    mlen = torch.clamp(e + 1 + torch.randint(0, 3, (B,), device=DEV, generator=gen), max=L)
    mlen[:7] = L                                                     # ties at the longest right length
    mmask = (torch.arange(L, device=DEV)[None] < mlen[:, None]).long()
    return [mf, mmask, s + 1, e + 1, mimage, ef, 0, eimage]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_b4096_against_fp64_restatement(precision):
    torch.manual_seed(21)
    model = Model(cfg_for(FULL), precision=precision).to(DEV)
    batch = big_batch(4096, FULL, 5)
    with torch.no_grad():
        scores = model(batch)
        ref = melhi_scores([x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x for x in batch], sd64(model))
    assert max_err(scores, ref) < TOL[precision]


def test_gradients_are_bitwise_reproducible():
    model = case_model("full_b64", "bf16x3")
    batch = to_dev(melhi_inputs("full_b64", {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    G = torch.from_numpy(grad_weights("full_b64", (64, FULL["N"]))).to(DEV)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        (model(batch) * G).sum().backward()
        runs.append([p.grad.clone() for p in model.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_adam_steps_track_the_restatement():
    name = "b64_ties"
    model = case_model(name, "f32")
    batch = to_dev(melhi_inputs(name, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    b64 = to_dev(batch, torch.float64)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt64 = torch.optim.Adam(list(sd.values()), lr=1e-3)
    G = torch.from_numpy(grad_weights(name, (64, TINY["N"]))).to(DEV)
    for _ in range(10):
        opt.zero_grad()
        (model(batch) * G).sum().backward()
        opt.step()
        opt64.zero_grad()
        (melhi_scores(b64, sd) * G.double()).sum().backward()
        opt64.step()
    with torch.no_grad():
        assert max_err(model(batch), melhi_scores(b64, sd)) < 1e-4
        params = dict(model.named_parameters())
        for k in KEYS:
            assert (params[k].double() - sd[k]).abs().max().item() < 2e-4, k


def test_abi_refuses_with_device_buffers():
    lib = _lib.load()
    model = case_model("b4", "bf16x3")
    batch = to_dev(melhi_inputs("b4", {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    order, lengths = orders_and_lengths(batch[2], batch[3], batch[1], TINY["L"])
    c = _lib.DrinMelhiConfigC(batch=4, num_candidates=TINY["N"], embed_dim=TINY["D"], image_dim=TINY["R"], mention_tokens=TINY["L"],
                              image_regions=TINY["P"], precision=_lib.PREC_BF16X3, cosine_eps=1e-8, thres_tmim=0.3, thres_imie=0.3)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    b = _lib.DrinMelhiBatchC(*[ptr(t) for t in (batch[0], batch[1], batch[2], batch[3], batch[4], batch[5], batch[7])])
    p = _lib.DrinMelhiParamsC(*[ptr(t) for t in model.param_list()])
    nbytes = lib.drin_melhi_workspace_bytes(C.byref(c), 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    scores = torch.empty(4, TINY["N"], device=DEV)
    call = lambda o, n, size=nbytes: lib.drin_melhi_forward(C.byref(c), C.byref(b), C.byref(p), o.ctypes.data_as(C.c_void_p),   # noqa: E731
                                                            n.ctypes.data_as(C.c_void_p), ptr(ws), size, ptr(scores), None)
    assert call(order, lengths) == _lib.OK
    torch.cuda.synchronize()
    assert torch.isfinite(scores).all()
    swapped = order.copy()
    swapped[1] = swapped[1][::-1].copy()
    if not np.array_equal(lengths[1][swapped[1]], np.sort(lengths[1])[::-1]):
        assert call(np.ascontiguousarray(swapped), lengths) == _lib.E_INDEX
    assert call(order, lengths, nbytes - 4) == _lib.E_WORKSPACE
    c.embed_dim = 18
    assert call(order, lengths) == _lib.E_SHAPE
