"""MELHI on the MI355X where the shapes choose other kernels: the shape cases of melhi_shapes.npz (widths off the GEMM tiles,
N = P = 1, L = 3 and L = 300, the longest left context, D = 1024), the split-bf16 gates of the GEMM module straddled at full
width (with the gemm_x3 launch counts that prove each gate was crossed), B = 4096 forward and backward, frozen parameter
subsets, and the C ABI's accumulate contract with guard bands around every buffer it writes.

Every comparison is against the fp64 restatement (tests/melhi_restatement.py) on the device, in both precisions, with the
bars of DESIGN.md section 14: scores 1e-4 (bf16x3) / 1e-5 (f32), NaN patterns identical, and per gradient tensor
max |got - ref| / max |ref| < 2e-4.  Each comparison prints its figures ("MEASURE ...") before it asserts.

The whole file takes about 30 s on one MI355X (26 s in the tests, most of it in the fp64 restatement at full width).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.melhi import Model, orders_and_lengths
from tests.melhi_inputs import (CASES, FULL, KEYS, SHAPE_CASES, SHAPE_CHECKSUM, SHAPE_FORWARD_ONLY, geometry, grad_weights,
                                melhi_inputs)
from tests.melhi_restatement import melhi_scores
from tests.test_gpu_melhi import TOL, big_batch, cfg_for, max_err, sd64, to_dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
DEV = "cuda"
GTOL = 2e-4
PRECISIONS = ["bf16x3", "f32"]


@pytest.fixture(scope="module")
def shapes_golden():
    return np.load(os.path.join(GOLDEN, "melhi_shapes.npz"))


def grad_err(got, ref) -> float:
    """max |got - ref| / max |ref| of one gradient tensor; a structurally zero reference must come back exactly zero."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max().item()
    diff = (got - ref).abs().max().item()
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale


def check_grads(tag: str, got: dict, ref: dict):
    errs = {k: grad_err(got[k], ref[k]) for k in got}
    print(f"MEASURE {tag} grad_max {max(errs.values()):.3e} " + " ".join(f"{k.split('.')[-2]}.{k.split('.')[-1]}={e:.2e}"
                                                                       for k, e in errs.items()), flush=True)
    for k, e in errs.items():
        assert e < GTOL, (tag, k, e)


def ref_grads(sd: dict) -> dict:
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in sd.items()}


# ---- the shape cases against their goldens and the restatement ----------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SHAPE_CASES)
def test_shape_cases_match_goldens_and_restatement(name, precision, shapes_golden):
    case, g = CASES[name], geometry(name)
    t1, t2 = case.get("thres", (0.3, 0.3))
    torch.manual_seed(case["seed"])
    model = Model(cfg_for(g, (t1, t2)), precision=precision).to(DEV)
    batch = to_dev(melhi_inputs(name, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    scores = model(batch)
    torch.cuda.synchronize()
    sd = sd64(model)
    ref, mask = melhi_scores(to_dev(batch, torch.float64), sd, t1, t2, return_mask=True)
    e_ref = max_err(scores, ref)
    s = scores.detach().double().cpu()
    if name in SHAPE_CHECKSUM:
        e_gold = (s.flatten()[:32] - torch.from_numpy(shapes_golden[f"{name}/scores_head"]).double()).abs().max().item()
        e_sum = abs(s.sum().item() - float(shapes_golden[f"{name}/scores_sum"])) / s.numel()
    else:
        e_gold, e_sum = max_err(s, torch.from_numpy(shapes_golden[f"{name}/scores"])), 0.0
    print(f"MEASURE shape {name} {precision} scores ref {e_ref:.3e} golden {e_gold:.3e} nan_rows "
          f"{torch.isnan(s).any(-1).sum().item()}", flush=True)
    assert e_ref < TOL[precision] and e_gold < TOL[precision] and e_sum < TOL[precision]
    assert np.array_equal(mask.cpu().numpy().astype(np.uint8), shapes_golden[f"{name}/mask"])
    if name in SHAPE_FORWARD_ONLY:
        assert torch.isnan(s).any()
        return
    G = torch.from_numpy(grad_weights(name, scores.shape)).to(DEV)
    (scores * G).sum().backward()
    (ref * G.double()).sum().backward()
    params = dict(model.named_parameters())
    got = {k: params[k].grad for k in KEYS}
    check_grads(f"shape {name} {precision} restatement", got, ref_grads(sd))
    if name in SHAPE_CHECKSUM:
        for k in KEYS:
            gk = got[k].detach().double().cpu()
            want_l2 = float(shapes_golden[f"{name}/grad_l2/{k}"])
            assert abs(gk.norm().item() - want_l2) <= GTOL * max(want_l2, 1e-12), k
            head = torch.from_numpy(shapes_golden[f"{name}/grad_head/{k}"]).double()
            assert (gk.flatten()[:16] - head).abs().max().item() <= GTOL * max(gk.abs().max().item(), 1e-12), k
    else:
        check_grads(f"shape {name} {precision} golden", got,
                    {k: torch.from_numpy(shapes_golden[f"{name}/grad/{k}"]) for k in KEYS})


# ---- full width: the split-bf16 gates -------------------------------------------------------------------------------------
def gate_batch(B: int):
    """big_batch (ties on both sides, seven right contexts of the longest length) plus one left context of L - 2 tokens, and
    token 0 of every other mention along its mapped image, so that the image mask is mixed and the image gradients are not
    zero."""
    batch = big_batch(B, FULL, 1000 + B)
    L = FULL["L"]
    batch[2][8], batch[3][8] = L - 1, L
    w, b = full_image_map()
    mf, mimage = batch[0], batch[4]
    mf[::2, 0] = mimage[::2].mean(1) @ w.T + b + 0.3 * mf[::2, 0]
    return batch


@functools.lru_cache(maxsize=1)
def full_image_map():
    m = full_model("f32")
    return m.image_map_text.weight.detach().clone(), m.image_map_text.bias.detach().clone()


def gate_grad_weights(B: int) -> torch.Tensor:
    return torch.randn(B, FULL["N"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(2000 + B))


def full_model(precision: str) -> Model:
    torch.manual_seed(21)
    return Model(cfg_for(FULL), precision=precision).to(DEV)


@functools.lru_cache(maxsize=2)
def full_ref(B: int):
    """fp64 restatement of gate_batch(B) on the full-width weights: (scores, {key: gradient})."""
    sd = sd64(full_model("f32"))
    batch = [x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x for x in gate_batch(B)]
    scores, mask = melhi_scores(batch, sd, return_mask=True)
    assert 0 < mask.sum().item() < B
    (scores * gate_grad_weights(B).double()).sum().backward()
    return scores.detach(), ref_grads(sd)


def x3_forward_launches(B: int, N: int) -> int:
    """Split-bf16 NT products of one forward at full width (M >= 256, not accumulating; the lanes have T <= L - 1 < 256 rows):
    eim and ent (M = B N), g0 (M = 2 B), mim, cst and men (M = B)."""
    return 2 * (B * N >= 256) + (2 * B >= 256) + 3 * (B >= 256)


def x3_backward_launches(B: int, N: int) -> int:
    """Split-bf16 TN products of one backward at full width (M >= 1024; N, K >= 128; dW_hh and the lane dW_ih have
    T <= L - 1 rows): entity_final_map twice and image_map_text from deim (M = B N), dW_ih of the time-0 cells (M = 2 B),
    mention_final_map, the two constant blocks of dW_ih and image_map_text from dmim (M = B)."""
    return 3 * (B * N >= 1024) + (2 * B >= 1024) + 4 * (B >= 1024)


def run_full(B: int, precision: str, backward: bool):
    """(scores, {key: gradient} or None, gemm_x3 launches of the profiled call: the backward call when `backward`)."""
    model = full_model(precision)
    batch = gate_batch(B)
    if not backward:
        with torch.no_grad():
            torch.cuda.synchronize()
            _lib.profile_begin()
            scores = model(batch)
            torch.cuda.synchronize()
            prof = _lib.profile_end()
        return scores, None, prof["gemm_x3"][1]
    scores = model(batch)
    loss = (scores * gate_grad_weights(B)).sum()
    torch.cuda.synchronize()
    _lib.profile_begin()
    loss.backward()
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    params = dict(model.named_parameters())
    return scores.detach(), {k: params[k].grad for k in KEYS}, prof["gemm_x3"][1]


def compare_full(B: int, backward: bool):
    """Both precisions at batch B against the fp64 restatement; the profiled call's gemm_x3 launches must be what the gates
    give (x3_forward_launches / x3_backward_launches for bf16x3, none for the f32 control)."""
    ref, ref_g = full_ref(B)
    for precision in PRECISIONS:
        scores, grads, n_x3 = run_full(B, precision, backward)
        e = max_err(scores, ref)
        print(f"MEASURE gate B={B} {'backward' if backward else 'forward'} {precision} scores {e:.3e} gemm_x3 {n_x3}", flush=True)
        assert e < TOL[precision], (B, precision, e)
        if backward:
            check_grads(f"gate B={B} {precision}", grads, ref_g)
        want = (x3_backward_launches if backward else x3_forward_launches)(B, FULL["N"]) if precision == "bf16x3" else 0
        assert n_x3 == want, (B, precision, n_x3, want)


BACKWARD_PAIRS = [(93, 94), (511, 512), (1023, 1024)]   # B N, 2 B and B reach 1024
FORWARD_PAIRS = [(127, 128), (255, 256)]                # 2 B and B reach 256


@pytest.mark.parametrize("B", [b for pair in BACKWARD_PAIRS for b in pair])
def test_backward_gate_at_full_width(B):
    lo, hi = next(pair for pair in BACKWARD_PAIRS if B in pair)
    N = FULL["N"]
    assert x3_backward_launches(hi, N) > x3_backward_launches(lo, N)   # the pair straddles a gate
    assert x3_backward_launches(93, N) == 0
    compare_full(B, backward=True)


@pytest.mark.parametrize("B", [b for pair in FORWARD_PAIRS for b in pair])
def test_forward_gate_at_full_width(B):
    lo, hi = next(pair for pair in FORWARD_PAIRS if B in pair)
    assert x3_forward_launches(hi, FULL["N"]) > x3_forward_launches(lo, FULL["N"])
    compare_full(B, backward=False)


def test_b4096_forward_and_backward():
    compare_full(4096, backward=False)
    compare_full(4096, backward=True)


def test_b4096_gradients_are_bitwise_reproducible():
    model = full_model("bf16x3")
    batch = gate_batch(4096)
    G = gate_grad_weights(4096)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        (model(batch) * G).sum().backward()
        runs.append([p.grad.clone() for p in model.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- frozen parameter subsets ------------------------------------------------------------------------------------------
LSTM = [k for k in KEYS if "mention_lstm" in k]
SUBSETS = {
    "final_maps": [k for k in KEYS if "final_map" in k],                 # the want_lstm early return
    "image_map_text": [k for k in KEYS if k.startswith("image_map_text")],   # the LSTM backward runs, writes no LSTM gradient
    "lstm": LSTM,
    "all_but_w_hh": [k for k in KEYS if k != "mention_encoder.mention_lstm.weight_hh_l0"],
    "b_ih": ["mention_encoder.mention_lstm.bias_ih_l0"],
}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("where", ["full_b128", "odd_w"])
def test_frozen_subsets(where, precision):
    if where == "odd_w":
        torch.manual_seed(CASES["odd_w"]["seed"])
        model = Model(cfg_for(geometry("odd_w")), precision=precision).to(DEV)
        batch = to_dev(melhi_inputs("odd_w", {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
        G = torch.from_numpy(grad_weights("odd_w", (CASES["odd_w"]["B"], geometry("odd_w")["N"]))).to(DEV)
        sd = sd64(model)
        ref = melhi_scores(to_dev(batch, torch.float64), sd)
        (ref * G.double()).sum().backward()
        want = ref_grads(sd)
    else:
        model, batch, G = full_model(precision), gate_batch(128), gate_grad_weights(128)
        want = full_ref(128)[1]
    params = dict(model.named_parameters())
    (model(batch) * G).sum().backward()
    every = {k: params[k].grad.clone() for k in KEYS}
    for subset, keys in SUBSETS.items():
        model.zero_grad(set_to_none=True)
        for k, p in params.items():
            p.requires_grad_(k in keys)
        (model(batch) * G).sum().backward()
        for k in KEYS:
            if k not in keys:
                assert params[k].grad is None, (subset, k)
        got = {k: params[k].grad for k in keys}
        check_grads(f"frozen {where} {precision} {subset}", got, {k: want[k] for k in keys})
        for k in keys:
            assert torch.equal(got[k], every[k]), (subset, k)
    for p in params.values():
        p.requires_grad_(True)


# ---- the C ABI: gradients accumulate, nothing is written outside its buffer ---------------------------------------------
GUARD = 256      # bytes before and after every buffer
PATTERN = 0xA7   # guard bytes


class Guarded:
    """`nbytes` of device memory between two guard bands of PATTERN."""

    def __init__(self, nbytes: int, fill: int = PATTERN):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + nbytes] = fill

    def ptr(self) -> C.c_void_p:
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def f32(self) -> torch.Tensor:
        return self.buf[GUARD:GUARD + self.nbytes].view(torch.float32)

    def guards_intact(self) -> bool:
        return bool((self.buf[:GUARD] == PATTERN).all() and (self.buf[GUARD + self.nbytes:] == PATTERN).all())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("where", ["odd_w", "full_b1024"])
def test_abi_accumulates_and_stays_in_bounds(where, precision):
    lib = _lib.load()
    if where == "odd_w":
        g, (t1, t2) = geometry("odd_w"), CASES["odd_w"].get("thres", (0.3, 0.3))
        torch.manual_seed(CASES["odd_w"]["seed"])
        model = Model(cfg_for(g), precision=precision).to(DEV)
        batch = to_dev(melhi_inputs("odd_w", {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
        G = torch.from_numpy(grad_weights("odd_w", (CASES["odd_w"]["B"], g["N"]))).to(DEV)
        sd = sd64(model)
        ref = melhi_scores(to_dev(batch, torch.float64), sd, t1, t2)
        (ref * G.double()).sum().backward()
        ref, want = ref.detach(), ref_grads(sd)
    else:
        g, (t1, t2) = FULL, (0.3, 0.3)
        model, batch, G = full_model(precision), gate_batch(1024), gate_grad_weights(1024)
        ref, want = full_ref(1024)
    B = batch[0].shape[0]
    c = _lib.DrinMelhiConfigC(batch=B, num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"],
                              image_regions=g["P"], precision=_lib.PREC_BF16X3 if precision == "bf16x3" else _lib.PREC_F32,
                              cosine_eps=1e-8, thres_tmim=t1, thres_imie=t2)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    tensors = [batch[i] for i in (0, 1, 2, 3, 4, 5, 7)]
    assert all(t.is_contiguous() for t in tensors)
    bt = _lib.DrinMelhiBatchC(*[ptr(t) for t in tensors])
    params = [p.detach() for p in model.param_list()]
    p = _lib.DrinMelhiParamsC(*[ptr(t) for t in params])
    order, lengths = orders_and_lengths(batch[2], batch[3], batch[1], g["L"])
    oa, la = order.ctypes.data_as(C.c_void_p), lengths.ctypes.data_as(C.c_void_p)
    n_inf, n_trn = lib.drin_melhi_workspace_bytes(C.byref(c), 0), lib.drin_melhi_workspace_bytes(C.byref(c), 1)
    assert 0 < n_inf < n_trn
    ws_inf, ws_trn = Guarded(n_inf, 0x00), Guarded(n_trn, 0xFF)   # different contents: the forward must not read either
    s_inf, s_trn = Guarded(4 * B * g["N"]), Guarded(4 * B * g["N"])
    gen = torch.Generator(device=DEV).manual_seed(7)
    grads, seeds = [], []
    for k, t in zip(KEYS, params):
        buf = Guarded(4 * t.numel())
        seed = torch.randn(t.numel(), device=DEV, generator=gen) * want[k].abs().max().float()
        buf.f32().copy_(seed)
        grads.append(buf)
        seeds.append(seed.clone())
    gc = _lib.DrinMelhiParamGradsC(*[b.ptr() for b in grads])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gs = G.float().contiguous()
    torch.cuda.synchronize()
    assert lib.drin_melhi_forward(C.byref(c), C.byref(bt), C.byref(p), oa, la, ws_inf.ptr(), n_inf, s_inf.ptr(), st) == _lib.OK, \
        lib.drin_last_error()
    assert lib.drin_melhi_forward(C.byref(c), C.byref(bt), C.byref(p), oa, la, ws_trn.ptr(), n_trn, s_trn.ptr(), st) == _lib.OK, \
        lib.drin_last_error()
    assert lib.drin_melhi_backward(C.byref(c), C.byref(bt), C.byref(p), oa, la, ws_trn.ptr(), n_trn, ptr(gs), C.byref(gc), st) == \
        _lib.OK, lib.drin_last_error()
    torch.cuda.synchronize()
    for what, buf in [("ws_inf", ws_inf), ("ws_trn", ws_trn), ("scores_inf", s_inf), ("scores_trn", s_trn)] + \
            list(zip(KEYS, grads)):
        assert buf.guards_intact(), what
    scores = s_trn.f32().view(B, g["N"])
    assert torch.equal(s_inf.f32().view(B, g["N"]), scores)
    e = max_err(scores, ref)
    print(f"MEASURE abi {where} {precision} scores {e:.3e}", flush=True)
    assert e < TOL[precision]
    added = {k: (b.f32().double() - s.double()).view(t.shape) for k, b, s, t in zip(KEYS, grads, seeds, params)}
    check_grads(f"abi {where} {precision}", added, want)
