"""The GHMFC forward restated from scratch in plain torch at whatever dtype its inputs have (the tests use float64): explicit
matrix products, softmax and layer norm on a state dict - no nn.Module, no torch attention call.  The yardstick for the errors
of drin_ghmfc_forward (tests/test_gpu_ghmfc.py) and itself checked against the reference's goldens (tests/test_ghmfc_host.py).
"""
from __future__ import annotations

import math

import torch

FUSION = "mention_encoder.intermediate_layer."


def softmax_attention(q, k, v, keep, heads: int):
    """q [B, Lq, E], k, v [B, Lk, E] already projected; keep: bool [B, Lk] or None.  A query with no kept key gets zero weights."""
    B, Lq, E = q.shape
    Lk, dh = k.shape[1], E // heads
    qh = q.reshape(B, Lq, heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, heads, dh).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, heads, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    top = s.max(-1, keepdim=True).values
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    e = torch.exp(s - top)
    den = e.sum(-1, keepdim=True)
    w = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    return (w @ vh).permute(0, 2, 1, 3).reshape(B, Lq, E)


def layer_norm(x, weight, bias, eps: float = 1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * weight + bias


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def cross_attention(sd, prefix: str, seq_a, keep_a, seq_b, keep_b, heads: int):
    g = lambda n: sd[prefix + n]   # noqa: E731
    E = seq_a.shape[-1]
    bias = g("a2b_attention.in_proj_bias")
    q = seq_a @ g("a2b_attention.q_proj_weight").T + bias[:E]
    k = seq_b @ g("a2b_attention.k_proj_weight").T + bias[E:2 * E]
    v = seq_b @ g("a2b_attention.v_proj_weight").T + bias[2 * E:]
    x = softmax_attention(q, k, v, keep_b, heads) @ g("a2b_attention.out_proj.weight").T + g("a2b_attention.out_proj.bias")
    x = layer_norm(x, g("layernorms.0.weight"), g("layernorms.0.bias"))
    x = layer_norm(x @ g("a2b_ffn.weight").T + g("a2b_ffn.bias") + x, g("layernorms.1.weight"), g("layernorms.1.bias"))
    w, bias = g("b2a_attention.in_proj_weight"), g("b2a_attention.in_proj_bias")
    q = x @ w[:E].T + bias[:E]
    k = seq_a @ w[E:2 * E].T + bias[E:2 * E]
    v = seq_a @ w[2 * E:].T + bias[2 * E:]
    y = softmax_attention(q, k, v, keep_a, heads) @ g("b2a_attention.out_proj.weight").T + g("b2a_attention.out_proj.bias")
    y = layer_norm(y, g("layernorms.2.weight"), g("layernorms.2.bias"))
    return layer_norm(y @ g("b2a_ffn.weight").T + g("b2a_ffn.bias") + y, g("layernorms.3.weight"), g("layernorms.3.bias"))


def mention_repr(batch, sd, heads: int):
    text, mask, image = batch[0], batch[1], batch[4]
    keep = mask != 0
    t = cross_attention(sd, FUSION + "t2v_attention.", text, keep, image, None, heads).max(1).values
    t = gelu(t @ sd[FUSION + "text_linear.weight"].T + sd[FUSION + "text_linear.bias"])
    v = cross_attention(sd, FUSION + "v2t_attention.", image, None, text, keep, heads).max(1).values
    v = gelu(v @ sd[FUSION + "image_linear.weight"].T + sd[FUSION + "image_linear.bias"])
    z = torch.cat([t, v], 1) @ sd[FUSION + "score_linear.weight"].T + sd[FUSION + "score_linear.bias"]
    z = torch.exp(z - z.max(1, keepdim=True).values)
    s = z / z.sum(1, keepdim=True)
    return s[:, :1] * t + s[:, 1:] * v


def entity_repr(batch, sd):
    ef, emask = batch[5], batch[6]
    if ef.dim() == 4:   # WikiMEL: the mean of tokens 1 : ntok - 1 (an empty slice gives NaN, as torch.mean does)
        T = ef.shape[2]
        ntok = emask.sum(-1)
        pos = torch.arange(T, device=ef.device)
        inside = ((pos >= 1) & (pos[None, None, :] < (ntok - 1)[:, :, None])).to(ef.dtype)
        ef = (ef * inside[..., None]).sum(2) / inside.sum(2)[..., None]
    return ef @ sd["entity_encoder.final_layer.weight"].T + sd["entity_encoder.final_layer.bias"]


def ghmfc_scores(batch, sd, heads: int, eps: float = 1e-8, return_mention: bool = False):
    m = mention_repr(batch, sd, heads)
    e = entity_repr(batch, sd)
    dot = (m[:, None, :] * e).sum(-1)
    scores = dot / (m.norm(dim=-1).clamp_min(eps)[:, None] * e.norm(dim=-1).clamp_min(eps))
    return (scores, m) if return_mention else scores
