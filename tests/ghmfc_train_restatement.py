"""tests/ghmfc_restatement.py's forward with the two things a training step adds, still plain torch at the inputs' dtype:

- `idx_text` / `idx_image` [B, width] (int64): when given, each max over the sequence becomes a gather at those positions.
  The max is full of ties and near-ties, so an fp32 argmax legitimately differs from the fp64 one; a
  gradient reference has to differentiate the SAME selection as the code under test, i.e. take the library's indices.
- `keeps`: four bool [B, H, Lq, Lk] keep masks (t2v a2b, t2v b2a, v2t a2b, v2t b2a - the order of the draws) and the rate
  `p`: the attention weights become w keep / (1 - p).
"""
from __future__ import annotations

import math

import torch

from tests.ghmfc_restatement import FUSION, entity_repr, gelu, layer_norm


def softmax_attention(q, k, v, keep_key, heads: int, keep=None, p: float = 0.0):
    B, Lq, E = q.shape
    Lk, dh = k.shape[1], E // heads
    qh = q.reshape(B, Lq, heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, heads, dh).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, heads, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if keep_key is not None:
        s = s.masked_fill(~keep_key[:, None, None, :], float("-inf"))
    top = s.max(-1, keepdim=True).values
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    e = torch.exp(s - top)
    den = e.sum(-1, keepdim=True)
    w = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    if keep is not None:
        w = w * keep.to(w.dtype) / (1.0 - p)
    return (w @ vh).permute(0, 2, 1, 3).reshape(B, Lq, E)


def cross_attention(sd, prefix: str, seq_a, keep_a, seq_b, keep_b, heads: int, keeps=(None, None), p: float = 0.0):
    g = lambda n: sd[prefix + n]   # noqa: E731
    E = seq_a.shape[-1]
    bias = g("a2b_attention.in_proj_bias")
    q = seq_a @ g("a2b_attention.q_proj_weight").T + bias[:E]
    k = seq_b @ g("a2b_attention.k_proj_weight").T + bias[E:2 * E]
    v = seq_b @ g("a2b_attention.v_proj_weight").T + bias[2 * E:]
    x = softmax_attention(q, k, v, keep_b, heads, keeps[0], p) @ g("a2b_attention.out_proj.weight").T + g("a2b_attention.out_proj.bias")
    x = layer_norm(x, g("layernorms.0.weight"), g("layernorms.0.bias"))
    x = layer_norm(x @ g("a2b_ffn.weight").T + g("a2b_ffn.bias") + x, g("layernorms.1.weight"), g("layernorms.1.bias"))
    w, bias = g("b2a_attention.in_proj_weight"), g("b2a_attention.in_proj_bias")
    q = x @ w[:E].T + bias[:E]
    k = seq_a @ w[E:2 * E].T + bias[E:2 * E]
    v = seq_a @ w[2 * E:].T + bias[2 * E:]
    y = softmax_attention(q, k, v, keep_a, heads, keeps[1], p) @ g("b2a_attention.out_proj.weight").T + g("b2a_attention.out_proj.bias")
    y = layer_norm(y, g("layernorms.2.weight"), g("layernorms.2.bias"))
    return layer_norm(y @ g("b2a_ffn.weight").T + g("b2a_ffn.bias") + y, g("layernorms.3.weight"), g("layernorms.3.bias"))


def pick(x, idx):
    """max over dim 1, or the gather at idx [B, width] when given"""
    return x.max(1).values if idx is None else x.gather(1, idx.long()[:, None, :])[:, 0, :]


def mention_repr(batch, sd, heads: int, idx_text=None, idx_image=None, keeps=None, p: float = 0.0, return_pre_max: bool = False):
    text, mask, image = batch[0], batch[1], batch[4]
    keep = mask != 0
    keeps = keeps or (None, None, None, None)
    pre_t = cross_attention(sd, FUSION + "t2v_attention.", text, keep, image, None, heads, keeps[:2], p)
    pre_v = cross_attention(sd, FUSION + "v2t_attention.", image, None, text, keep, heads, keeps[2:], p)
    t = gelu(pick(pre_t, idx_text) @ sd[FUSION + "text_linear.weight"].T + sd[FUSION + "text_linear.bias"])
    v = gelu(pick(pre_v, idx_image) @ sd[FUSION + "image_linear.weight"].T + sd[FUSION + "image_linear.bias"])
    z = torch.cat([t, v], 1) @ sd[FUSION + "score_linear.weight"].T + sd[FUSION + "score_linear.bias"]
    z = torch.exp(z - z.max(1, keepdim=True).values)
    s = z / z.sum(1, keepdim=True)
    m = s[:, :1] * t + s[:, 1:] * v
    return (m, pre_t, pre_v) if return_pre_max else m


def ghmfc_train_scores(batch, sd, heads: int, idx_text=None, idx_image=None, keeps=None, p: float = 0.0, eps: float = 1e-8,
                       return_pre_max: bool = False):
    m, pre_t, pre_v = mention_repr(batch, sd, heads, idx_text, idx_image, keeps, p, return_pre_max=True)
    e = entity_repr(batch, sd)
    dot = (m[:, None, :] * e).sum(-1)
    scores = dot / (m.norm(dim=-1).clamp_min(eps)[:, None] * e.norm(dim=-1).clamp_min(eps))
    return (scores, pre_t, pre_v) if return_pre_max else scores
