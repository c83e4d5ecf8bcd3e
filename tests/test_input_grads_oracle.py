"""The CPU oracle's autograd gives the reference's gradients w.r.t. the batch tensors (tests/golden/input_grads.npz, written by
tools/gen_input_grad_golden.py from the unmodified reference).  Pins oracle/drin_oracle.py for this use: the GPU tests of the
input gradients compare against its fp64 autograd at sizes the fixtures do not cover.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import drin_oracle as O
from oracle.cases import build_case

FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
FULL = ["tiny_wd", "tiny_wm", "tiny_wd_edges_1010", "tiny_wd_static", "tiny_wd_layers3", "tiny_wd_vector", "tiny_wm_silu_relu"]
SUMMARY = ["wd_b4", "wm_b2"]
BAR = 2e-4          # relative Frobenius error per tensor, the bar of the parameter gradients
ABS_ZERO = 1e-6     # entity_object_score with one entity object: analytically 0 (the reference leaves ~1e-9) - unless a
#                     mention's object scores are all zero (tiny_wd): then its rows are ~1e6 through the +1e-9 of model.py:92,
#                     and the tensor is compared relatively


def rel_err(got: np.ndarray, ref: np.ndarray) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def oracle_input_grads(name, dtype=torch.float32):
    cfg, sd, batch = build_case(name)
    inputs = list(batch[:14])
    for i in FLOAT_INPUTS:
        inputs[i] = inputs[i].detach().to(dtype).requires_grad_(True)
    p = {k: v.to(dtype) for k, v in sd.items()}
    scores = O.forward(p, inputs, dtype=dtype, **O.config_kwargs(cfg))
    return cfg, inputs, scores


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "input_grads.npz"))


@pytest.mark.parametrize("name", FULL + SUMMARY)
def test_oracle_input_grads_match_reference(golden, name):
    cfg, inputs, scores = oracle_input_grads(name)
    G = torch.from_numpy(golden[f"{name}/G"])
    (scores * G).sum().backward()
    for i, field in FLOAT_INPUTS.items():
        gr = inputs[i].grad
        assert gr is not None, field
        if name in FULL:
            ref = golden[f"{name}/{field}"]
            assert gr.shape == ref.shape, field
            if field == "entity_object_score" and inputs[11].shape[-1] == 1 and np.abs(ref).max() <= ABS_ZERO:
                assert np.abs(gr.numpy()).max() <= ABS_ZERO, field          # analytically 0 (no zero object-score row)
                continue
            assert rel_err(gr.numpy(), ref) <= BAR, (field, rel_err(gr.numpy(), ref))
        else:
            l2 = float(golden[f"{name}/{field}_l2"])
            if field == "entity_object_score" and inputs[11].shape[-1] == 1 and l2 <= ABS_ZERO:
                assert gr.double().norm().item() <= ABS_ZERO
                continue
            assert abs(gr.double().norm().item() - l2) <= BAR * l2, field
            head = golden[f"{name}/{field}_head"]
            np.testing.assert_allclose(gr.flatten()[:16].numpy(), head, rtol=1e-3, atol=1e-3 * np.abs(head).max() + 1e-12)


# the Python-slice corners of Avg.avg (seq[i, begin:end].mean(0), baselines/ghmfc.py:54-60) at L = 6: negative bounds, 0, L,
# past L, start >= end (empty -> NaN) - the GPU tests of these corners compare against O.span_mean, so it is pinned here first
L_SPAN = 6
SPAN_CORNERS = [(-2, 6), (1, -1), (-5, -3), (0, 6), (0, 1), (5, 6), (6, 6), (2, 9), (-9, 2), (-1, 99), (4, 2), (3, 3),
                (0, -6), (-6, -5), (7, 9), (-3, -4), (0, 0), (1, 7)]


def _span_loop(seq, begin, end):
    return torch.stack([seq[i, int(begin[i]):int(end[i])].mean(0) for i in range(seq.shape[0])])


def _token_loop(feat, mask):
    ntok = mask.sum(-1)
    return torch.stack([torch.stack([feat[i, j, 1:int(ntok[i, j]) - 1].mean(0) for j in range(feat.shape[1])])
                        for i in range(feat.shape[0])])


def _same_with_nan(a, b, what):
    assert torch.equal(torch.isnan(a), torch.isnan(b)), what
    torch.testing.assert_close(torch.nan_to_num(a), torch.nan_to_num(b), rtol=1e-12, atol=1e-12, msg=what)


def test_oracle_span_mean_follows_python_slice_rules():
    g = torch.Generator().manual_seed(5)
    seq = torch.randn(len(SPAN_CORNERS), L_SPAN, 5, generator=g, dtype=torch.float64)
    begin = torch.tensor([b for b, _e in SPAN_CORNERS])
    end = torch.tensor([e for _b, e in SPAN_CORNERS])
    gout = torch.randn(len(SPAN_CORNERS), 5, generator=g, dtype=torch.float64)
    x1, x2 = seq.clone().requires_grad_(True), seq.clone().requires_grad_(True)
    got, ref = O.span_mean(x1, begin, end), _span_loop(x2, begin, end)
    for i, (b, e) in enumerate(SPAN_CORNERS):
        _same_with_nan(got[i], ref[i], f"span [{b}:{e}]")
    # the autograd gradient: 1/count on the clipped span's rows, exactly 0 elsewhere (empty spans: 0 on every row)
    (torch.nan_to_num(got) * gout).sum().backward()
    (torch.nan_to_num(ref) * gout).sum().backward()
    for i, (b, e) in enumerate(SPAN_CORNERS):
        _same_with_nan(x1.grad[i], x2.grad[i], f"span [{b}:{e}] gradient")
        rows = set(range(L_SPAN)[b:e])
        for t in range(L_SPAN):
            if t not in rows:
                assert bool((x1.grad[i, t] == 0).all()), (b, e, t)


@pytest.mark.parametrize("T", [1, 2, 3, 6])
def test_oracle_entity_token_mean_follows_python_slice_rules(T):
    """feat[i, j, 1:ntok-1].mean(0), ntok = mask.sum(): ntok in {0, 1, 2, 3, T} and masks with holes (the count is a sum, not
    the position of the last 1)."""
    g = torch.Generator().manual_seed(T)
    masks = [[0] * T, [1] + [0] * (T - 1), [1] * T]
    if T >= 2:
        masks += [[1, 1] + [0] * (T - 2), [0] * (T - 1) + [1], [1, 0] * (T // 2) + [1] * (T % 2)]
    if T >= 3:
        masks += [[1, 1, 1] + [0] * (T - 3), [0, 1, 0] + [1] * (T - 3), [1] * (T - 1) + [0]]
    mask = torch.tensor(masks, dtype=torch.int64).view(1, len(masks), T)
    feat = torch.randn(1, len(masks), T, 4, generator=g, dtype=torch.float64)
    gout = torch.randn(1, len(masks), 4, generator=g, dtype=torch.float64)
    x1, x2 = feat.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    got, ref = O.entity_token_mean(x1, mask), _token_loop(x2, mask)
    for j in range(len(masks)):
        _same_with_nan(got[0, j], ref[0, j], f"mask {masks[j]}")
    (torch.nan_to_num(got) * gout).sum().backward()
    (torch.nan_to_num(ref) * gout).sum().backward()
    for j in range(len(masks)):
        _same_with_nan(x1.grad[0, j], x2.grad[0, j], f"mask {masks[j]} gradient")
        ntok = sum(masks[j])
        rows = set(range(T)[1:ntok - 1])
        for t in range(T):
            if t not in rows:
                assert bool((x1.grad[0, j, t] == 0).all()), (masks[j], t)
