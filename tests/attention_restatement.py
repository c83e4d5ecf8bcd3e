"""A plain restatement of multi-head softmax attention in torch, differentiable and in any dtype: the yardstick of the
trainable attention (`drin_amd/attention.py`).  `tests/test_attention_host.py` holds it against torch's own
`nn.MultiheadAttention` in float64 (output and every gradient to 1e-10), which is what makes it one.

A query row with no kept key has zero weights (as `attention_fp64` of tests/test_gpu_ghmfc.py and the library's kernel):
zero output, no gradient through it.
"""
import math

import torch


def core_weights(q, k, key_mask, num_heads):
    """softmax weights [B, H, Lq, Lk] of q [B, Lq, E], k [B, Lk, E]; key_mask [B, Lk] nonzero = keep, or None."""
    B, Lq, E = q.shape
    dh = E // num_heads
    qh = q.reshape(B, Lq, num_heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, -1, num_heads, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if key_mask is None:
        return torch.softmax(s, -1)
    keep = (key_mask != 0)[:, None, None, :]
    some = keep.any(-1, keepdim=True)                                 # [B, 1, 1, 1]: the mention has a key at all
    s = torch.where(some, s.masked_fill(~keep, float("-inf")), torch.zeros_like(s))
    return torch.softmax(s, -1) * some.to(s.dtype)


def attention_core(q, k, v, key_mask, num_heads):
    """out [B, Lq, E] = per head softmax(q k^T / sqrt(dh) over the kept keys) v."""
    B, Lq, E = q.shape
    vh = v.reshape(B, -1, num_heads, E // num_heads).permute(0, 2, 1, 3)
    return (core_weights(q, k, key_mask, num_heads) @ vh).permute(0, 2, 1, 3).reshape(B, Lq, E)


def multihead_attention(sd, query, key, value, key_padding_mask, num_heads):
    """nn.MultiheadAttention(batch_first=True)(query, key, value, key_padding_mask)[0] in eval mode, on its state dict `sd`
    (packed `in_proj_weight` or `q_proj_weight` / `k_proj_weight` / `v_proj_weight`; biases optional).
    key_padding_mask: bool [B, Lk], True = drop (torch's convention), or None."""
    E = query.shape[-1]
    if "in_proj_weight" in sd:
        wq, wk, wv = sd["in_proj_weight"][:E], sd["in_proj_weight"][E:2 * E], sd["in_proj_weight"][2 * E:]
    else:
        wq, wk, wv = sd["q_proj_weight"], sd["k_proj_weight"], sd["v_proj_weight"]
    b = sd.get("in_proj_bias")
    bq, bk, bv = (None, None, None) if b is None else (b[:E], b[E:2 * E], b[2 * E:])
    lin = torch.nn.functional.linear
    keep = None if key_padding_mask is None else (~key_padding_mask).to(torch.int64)
    ctx = attention_core(lin(query, wq, bq), lin(key, wk, bk), lin(value, wv, bv), keep, num_heads)
    return lin(ctx, sd["out_proj.weight"], sd.get("out_proj.bias"))
