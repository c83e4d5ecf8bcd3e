"""GHMFC's other mention encoders restated in plain torch at the inputs' dtype (the tests use float64), built on
tests/ghmfc_train_restatement.py: explicit products, softmax, layer norm and dropout on a state dict - no nn.Module.  The same
two hooks as there:

- `idx` [B, D] (int64): when given, the max over the sequence becomes a gather at those positions (the library's own).
- `keeps`: the bool keep masks of the draws, in draw order, and the rate `p`.  Transformer: four per layer - attention weights
  [B, H, L, L], then drop1 [B L, 1, 1, D], drop [B L, 1, 1, ffn], drop2 [B L, 1, 1, D].  "text": the two attention masks.
"""
from __future__ import annotations

import torch

from tests.ghmfc_restatement import entity_repr, gelu, layer_norm
from tests.ghmfc_train_restatement import cross_attention, pick, softmax_attention
from tests.ghmfc_variant_inputs import CROSS, TRANSFORMER


def drop_rows(t, keep, p: float):
    """t keep / (1 - p) with a dropped element exactly 0; keep: bool with t's element count, or None"""
    if keep is None:
        return t
    return torch.where(keep.reshape(t.shape), t / (1.0 - p), torch.zeros_like(t))


def transformer_encoder(sd, x, keep_key, heads: int, layers: int, act: str, keeps=None, p: float = 0.0, prefix: str = TRANSFORMER):
    """nn.TransformerEncoder of post-norm nn.TransformerEncoderLayers (batch_first, no final norm); keep_key: bool [B, L]"""
    E = x.shape[-1]
    fn = gelu if act == "gelu" else torch.relu
    for i in range(layers):
        g = lambda n: sd[f"{prefix}layers.{i}.{n}"]   # noqa: E731
        k4 = keeps[4 * i:4 * i + 4] if keeps is not None else (None, None, None, None)
        w, b = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
        q, k, v = x @ w[:E].T + b[:E], x @ w[E:2 * E].T + b[E:2 * E], x @ w[2 * E:].T + b[2 * E:]
        a = softmax_attention(q, k, v, keep_key, heads, k4[0], p) @ g("self_attn.out_proj.weight").T + g("self_attn.out_proj.bias")
        x = layer_norm(x + drop_rows(a, k4[1], p), g("norm1.weight"), g("norm1.bias"))
        h = drop_rows(fn(x @ g("linear1.weight").T + g("linear1.bias")), k4[2], p)
        h = drop_rows(h @ g("linear2.weight").T + g("linear2.bias"), k4[3], p)
        x = layer_norm(x + h, g("norm2.weight"), g("norm2.bias"))
    return x


def span_mean(x, begin, end):
    """mean of x[b, begin[b] : end[b]] with Python's slice clipping; an empty span gives 0 / 0 = NaN, as torch.mean does"""
    L = x.shape[1]
    clip = lambda t: torch.where(t < 0, (t + L).clamp_min(0), t).clamp_max(L)   # noqa: E731
    s, e = clip(begin.long()), clip(end.long())
    pos = torch.arange(L, device=x.device)
    inside = ((pos[None, :] >= s[:, None]) & (pos[None, :] < e[:, None])).to(x.dtype)
    return (x * inside[..., None]).sum(1) / inside.sum(1)[:, None]


def variant_mention(batch, sd, enc: str, rep: str, heads: int, layers: int = 0, act: str = "gelu", idx=None, keeps=None, p: float = 0.0,
                    return_pre: bool = False):
    """(mention representation [B, D], the sequence under the final representation)"""
    text, mask, begin, end, image = batch[:5]
    keep = mask != 0
    if enc == "transformer":
        x = transformer_encoder(sd, text, keep, heads, layers, act, keeps, p)
    elif enc == "text":
        x = cross_attention(sd, CROSS, text, keep, image, None, heads, keeps or (None, None), p)
    else:
        x = text
    if enc == "linear":
        m = span_mean(x, begin, end) @ sd["mention_encoder.final_layer.linear.weight"].T + sd["mention_encoder.final_layer.linear.bias"]
    else:
        m = pick(x, idx) if rep == "max" else span_mean(x, begin, end)
    return (m, x) if return_pre else m


def variant_scores(batch, sd, enc: str, rep: str, heads: int, layers: int = 0, act: str = "gelu", idx=None, keeps=None, p: float = 0.0,
                   eps: float = 1e-8, return_pre: bool = False):
    m, pre = variant_mention(batch, sd, enc, rep, heads, layers, act, idx, keeps, p, return_pre=True)
    e = entity_repr(batch, sd)
    dot = (m[:, None, :] * e).sum(-1)
    scores = dot / (m.norm(dim=-1).clamp_min(eps)[:, None] * e.norm(dim=-1).clamp_min(eps))
    return (scores, m, pre) if return_pre else scores
