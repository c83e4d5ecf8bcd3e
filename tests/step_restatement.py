"""What closes a training step, written from the formulas in plain torch (no library call, importable without a GPU): the
triplet loss with its gradient as INTEGER hinge counts and the top-k hit counts (`metrics.TripletLoss`, `TopkAccuracy.update`),
and the clamped cosine of a mention row with its candidate rows.  The token mean of an entity is `oracle.drin_oracle.
entity_token_mean`, evaluated in fp64 by the caller.

The loss is  L = scale * sum_i sum_{b,n} max(0, v[i,b,n]),  v[i,b,n] = pos[i] - p[b,n] + margin,  p = -y_hat[:, :N-1],
pos[i] = sum_n p[i,n] y[i,n],  scale = 1 / (B B (N-1)).  torch.clamp passes a gradient where v >= 0, so

    dL / dy_hat[b,n] = scale * (A[b,n] - R[b] y[b,n]),    A[b,n] = #{i : v[i,b,n] >= 0},   R[b] = #{(b',n') : v[b,b',n'] >= 0}

and the answer slot (column N-1) gets 0.  `counts = A - R y` is an integer however the scores are rounded: a test can ask for it
exactly.  `dtype` is the precision v is evaluated in, as `(pos - p) + margin` like the reference writes it: float64 by default;
float32 gives the mask torch's own fp32 evaluation of fp32 scores has (a v within one fp32 rounding of 0 has another sign in fp64).
The loss is summed in fp64 either way.  Everything runs on the device its inputs live on; the hit counts are taken on the host."""
from collections import namedtuple

import torch

TripletCounts = namedtuple("TripletCounts", "loss counts scale hits")


def topk_hits(y, yhat, ks):
    """Per k: sum(y * (y_hat >= k-th largest of the row)) over the batch, as `TopkAccuracy.update`: any uint8 weight counts as
    often as it says, a tie with the k-th score is inside, and NaN sorts above everything (`torch.topk`), so that a row with k
    or more NaNs has a NaN bound and no hit, and a NaN gold never counts."""
    C = y.shape[1]
    s = yhat[:, :C].double()
    ranked = torch.sort(s, dim=1, descending=True).values          # NaN first, as torch.topk
    w = y.to(torch.int64)
    return torch.stack([(w * (s >= ranked[:, k - 1:k]).to(torch.int64)).sum() for k in ks]) if len(ks) else torch.zeros(0, dtype=torch.int64)


def triplet_counts(y, yhat, margin, ks=(), dtype=torch.float64, chunk_bytes=64 << 20):
    """-> TripletCounts(loss fp64 scalar, counts int64 [B, N], scale float, hits int64 [len(ks)]); d loss / d y_hat = counts * scale.
    y [B, N-1] uint8 weights, yhat [B, N] (or [B, N-1]: nothing to drop, counts has that width).  The [mentions, B, N-1] block
    of v is walked in chunks of mentions of at most `chunk_bytes`."""
    B, C = y.shape
    width, dev = yhat.shape[1], yhat.device
    p = -yhat[:, :C].to(dtype)
    w = y.to(dtype)
    pos = (p * w).sum(-1)
    m = torch.tensor(margin, dtype=dtype, device=dev)
    A = torch.zeros(B, C, dtype=torch.int64, device=dev)
    R = torch.zeros(B, dtype=torch.int64, device=dev)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    step = max(1, chunk_bytes // (B * C * 8 * 2))
    for i0 in range(0, B, step):
        v = (pos[i0:i0 + step, None, None] - p[None]) + m           # [i, b, n]
        active = v >= 0
        A += active.sum(0)
        R[i0:i0 + step] = active.sum((1, 2))
        total += torch.clamp(v, min=0).double().sum()
    scale = 1.0 / (float(B) * float(B) * float(C))
    counts = torch.zeros(B, width, dtype=torch.int64, device=dev)
    counts[:, :C] = A - R[:, None] * y.to(torch.int64)
    return TripletCounts(total * scale, counts, scale, topk_hits(y.cpu(), yhat.cpu(), list(ks)))


def cosine_rows64(x, y, eps):
    """out [B, N] = x[b] . y[b,n] / (max(|x[b]|, eps) max(|y[b,n]|, eps)) in fp64; x [B, D], y [B, N, D].  Pass fp64 leaves
    and differentiate the result: a clamped norm passes no gradient (and |.| passes none at an all-zero row)."""
    x, y = x.double(), y.double()
    nx = torch.linalg.vector_norm(x, dim=-1).clamp(min=eps)
    ny = torch.linalg.vector_norm(y, dim=-1).clamp(min=eps)
    return (x[:, None, :] * y).sum(-1) / (nx[:, None] * ny)


def cosine_rows64_grads(x, y, dout, eps):
    """-> (out, dx, dy) of `cosine_rows64` for the upstream gradient dout [B, N], all fp64."""
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    out = cosine_rows64(x64, y64, eps)
    dx, dy = torch.autograd.grad((out * dout.double()).sum(), [x64, y64])
    return out.detach(), dx, dy
