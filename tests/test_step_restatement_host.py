"""tests/step_restatement.py against what it restates, on the host: the reference's own goldens (`tests/golden/triplet.npz`,
`topk.npz`), the oracle's `triplet_loss` / `topk_counts` / `cosine`, and `metrics.TripletLoss` / `TopkAccuracy` on answers
that are not one-hot, on NaN and on infinite scores."""
import os

import numpy as np
import pytest
import torch

from drin_amd.metrics import TopkAccuracy, TripletLoss
from oracle import drin_oracle as O
from tests.step_restatement import cosine_rows64, cosine_rows64_grads, topk_hits, triplet_counts


def _case(B, N, seed, ties=False, grid=False):
    g = torch.Generator().manual_seed(seed)
    yhat = torch.randn(B, N, generator=g)
    if ties:
        yhat = torch.round(yhat * 2) / 2
    if grid:
        yhat = torch.randint(-64, 65, (B, N), generator=g).float() / 64
    y = torch.zeros(B, N - 1, dtype=torch.uint8)
    y[torch.arange(B), torch.randint(0, N - 1, (B,), generator=g)] = 1
    return y, yhat


def _autograd(loss_fn, y, yhat, margin, dtype):
    leaf = yhat.to(dtype).requires_grad_(True)
    loss = loss_fn(y, leaf, margin)
    loss.backward()
    return loss.detach(), leaf.grad


def test_triplet_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "triplet.npz"))
    for i in range(3):
        got = triplet_counts(torch.from_numpy(g[f"y{i}"]), torch.from_numpy(g[f"yhat{i}"]), 0.25)
        assert abs(got.loss.item() - float(g[f"loss{i}"])) <= 1e-6          # the golden is the reference's fp32 loss


def test_topk_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "topk.npz"))
    ks = [int(k) for k in g["ks"]]
    seen = 0
    for name in g.files:
        if not name.startswith("yhat") or name == "yhat_same_width":
            continue
        tag = name[4:]
        yhat, y = torch.from_numpy(g[name]), torch.from_numpy(g["y" + tag])
        fit = [k for k in ks if k <= yhat.shape[1] - 1]
        assert topk_hits(y, yhat, fit).tolist() == [int(g[f"correct{tag}_k{k}"]) for k in fit]
        assert triplet_counts(y, yhat, 0.25, fit).hits.tolist() == [int(g[f"correct{tag}_k{k}"]) for k in fit]
        seen += len(fit)
    assert seen == 28
    assert topk_hits(torch.from_numpy(g["y_same_width"]), torch.from_numpy(g["yhat_same_width"]), [3]).tolist() == [int(g["correct_same_width_k3"])]


def test_known_answers():
    y = torch.tensor([[1, 0], [0, 1]], dtype=torch.uint8)
    yhat = torch.tensor([[0.5, -0.2, 9.0], [-0.1, 0.3, 9.0]])
    # p = [[-.5,.2],[.1,-.3]], pos = [-.5,-.3]; v[0] = [.25,-.45,-.35,.05], v[1] = [.45,-.25,-.15,.25] (hand-computed in test_oracle_golden.py)
    got = triplet_counts(y, yhat, 0.25)
    assert abs(got.loss.item() - 0.125) < 1e-7
    # A = [[2,0],[0,2]]; R = [2, 2]; counts = A - R y
    assert got.counts.tolist() == [[0, 0, 0], [0, 0, 0]] and got.scale == 1 / 8
    # dyadic scores, so that hinges of exactly 0 occur: p = [[-.5,.25],[.125,-.375]], pos = [-.5,-.375], margin .625:
    # v[0] = .125 - p = [.625,-.125, 0,.5], v[1] = .25 - p = [.75, 0,.125,.625]; a hinge of 0 is active (clamp's mask is >=)
    yhat = torch.tensor([[0.5, -0.25, 9.0], [-0.125, 0.375, 9.0]])
    got = triplet_counts(y, yhat, 0.625)
    assert got.loss.item() == 2.625 / 8
    assert got.counts.tolist() == [[2 - 3, 1, 0], [2, 2 - 4, 0]]           # A = [[2,1],[2,2]], R = [3,4]
    loss, grad = _autograd(lambda yy, ss, m: TripletLoss(m)(yy, ss), y, yhat, 0.625, torch.float64)
    assert loss.item() == 2.625 / 8 and torch.equal(grad * 8, got.counts.double())
    yhat = torch.tensor([[0.9, 0.1, 0.5, 7.0], [0.2, 0.2, 0.1, 7.0], [0.3, 0.6, 0.1, 7.0]])
    y = torch.tensor([[0, 0, 1], [0, 1, 0], [0, 0, 0]], dtype=torch.uint8)
    assert topk_hits(y, yhat, [1, 2, 3]).tolist() == [1, 2, 2]


@pytest.mark.parametrize("B,N,ties", [(1, 2, False), (3, 4, True), (64, 11, False), (64, 101, True), (300, 37, True)])
def test_against_the_oracle(B, N, ties):
    y, yhat = _case(B, N, 100 + B + N, ties)
    ks = [k for k in (1, 3, 5, 10, 20, 50) if k <= N - 1]
    got = triplet_counts(y, yhat, 0.25, ks, chunk_bytes=1 << 16)            # several chunks of mentions
    loss, grad = _autograd(O.triplet_loss, y, yhat, 0.25, torch.float64)
    assert abs(got.loss.item() - loss.item()) <= 1e-13 * max(1.0, abs(loss.item()))
    assert (got.counts.double() * got.scale - grad).abs().max().item() <= 1e-13 * grad.abs().max().item()
    assert torch.equal(torch.round(grad / got.scale).to(torch.int64), got.counts)
    assert got.hits.tolist() == [O.topk_counts(yhat, y, k)[0] for k in ks]
    whole = triplet_counts(y, yhat, 0.25, ks)
    assert torch.equal(whole.counts, got.counts) and abs(whole.loss.item() - got.loss.item()) <= 1e-13
    # the fp32 mask is the one torch's fp32 evaluation has
    loss32, grad32 = _autograd(O.triplet_loss, y, yhat, 0.25, torch.float32)
    got32 = triplet_counts(y, yhat, 0.25, dtype=torch.float32)
    assert torch.equal(torch.round(grad32.double() / got32.scale).to(torch.int64), got32.counts)
    assert abs(got32.loss.item() - loss32.item()) <= 3e-6 * max(1.0, abs(loss32.item()))


def test_weights_nan_and_infinities_against_the_product_classes():
    """Answers that are not one-hot (two golds, a weight of 3, an empty row), a tie with the k-th score, a NaN gold, a NaN
    elsewhere, +-inf scores: `metrics.TripletLoss` under fp64 autograd and `TopkAccuracy.update` give the same numbers."""
    y, yhat = _case(9, 12, 3, grid=True)
    y[0, :] = 0
    y[0, 2], y[0, 7] = 1, 1
    y[1, :] = 0
    y[1, 4] = 3
    y[2, :] = 0
    gold3 = int(y[3].argmax())
    yhat[3, :11] = torch.where(torch.arange(11) % 3 == 0, yhat[3, gold3], yhat[3, :11])   # the gold ties with several
    ks = [1, 2, 4, 11, 7]
    variants = {"plain": yhat}
    for name, row, col, value in (("nan gold", 4, int(y[4].argmax()), float("nan")), ("nan other", 5, (int(y[5].argmax()) + 1) % 11, float("nan")),
                                  ("+inf", 6, (int(y[6].argmax()) + 1) % 11, float("inf")), ("-inf gold", 7, int(y[7].argmax()), float("-inf"))):
        t = yhat.clone()
        t[row, col] = value
        variants[name] = t
    for name, s in variants.items():
        got = triplet_counts(y, s, 0.25, ks)
        loss, grad = _autograd(lambda yy, ss, m: TripletLoss(m)(yy, ss), y, s, 0.25, torch.float64)
        assert torch.equal(torch.isnan(got.loss), torch.isnan(loss)) and (torch.isnan(loss) or got.loss.item() == pytest.approx(loss.item(), rel=1e-13)), name
        want = torch.round(torch.nan_to_num(grad, nan=0.0) / got.scale).to(torch.int64)
        assert torch.equal(got.counts, want), name
        assert not grad.isnan().any(), name                                 # clamp's mask passes nothing through a NaN hinge
        for q, k in enumerate(ks):
            t = TopkAccuracy(k)
            t.update(s, y)
            assert int(t.correct) == int(got.hits[q]), (name, k)
    assert triplet_counts(y, yhat, 0.25, ks).hits[3].item() == int(y.sum())  # k = N - 1: every weight counts


def test_cosine_rows64_value_and_clamp_gradients():
    g = torch.Generator().manual_seed(4)
    x, y, dout = torch.randn(3, 20, generator=g), torch.randn(3, 5, 20, generator=g), torch.randn(3, 5, generator=g)
    out = cosine_rows64(x, y, 1e-8)
    assert (out - O.cosine(x.double()[:, None, :], y.double(), 1e-8)).abs().max().item() <= 1e-15
    assert (out - torch.nn.functional.cosine_similarity(x.double()[:, None, :], y.double(), dim=-1, eps=1e-8)).abs().max().item() <= 1e-15
    x[1] = 0.0                                                               # |x| = 0: the clamp holds, d|x| passes nothing
    y[2, 3] = y[2, 3] / y[2, 3].norm() * 1e-9                                 # |y| < eps
    y[0, 1] = 0.0
    out, dx, dy = cosine_rows64_grads(x, y, dout, 1e-8)
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all() and torch.count_nonzero(out[1]).item() == 0
    x64, y64, g64 = x.double(), y.double(), dout.double()
    ny = y64.norm(dim=-1).clamp(min=1e-8)
    want = (g64[1, :, None] * y64[1] / (1e-8 * ny[1, :, None])).sum(0)        # x = 0: only the x . y term is left
    assert (dx[1] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    want = g64[2, 3] * x64[2] / (x64[2].norm() * 1e-8)                        # |y| clamped: no -c y / |y|^2 term
    assert (dy[2, 3] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    want = g64[0, 1] * x64[0] / (x64[0].norm() * 1e-8)
    assert (dy[0, 1] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # an ordinary pair: d cos / dy = (xn - c yn) / |y|
    xn, yn = x64[0] / x64[0].norm(), y64[0, 0] / y64[0, 0].norm()
    want = g64[0, 0] * (xn - (xn @ yn) * yn) / y64[0, 0].norm()
    assert (dy[0, 0] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # eps above some norms and below others
    out, dx, dy = cosine_rows64_grads(x, y, dout, 0.5)
    assert (out - O.cosine(x64[:, None, :], y64, 0.5)).abs().max().item() <= 1e-15
