"""GHMFC's entity side (baselines/ghmfc.py:237-250) restated in plain torch at whatever dtype its inputs have, with the two
settings of `common/args.py:15-16`: the token pooling ("avg" | "max" over tokens 1 : ntok - 1, Python's slice rules) and the final
layer ("linear" | "none" = Identity: the state dict then holds no entity keys).  The mention side is the restatements' of
tests/ghmfc_train_restatement.py (the default encoder) and tests/ghmfc_variant_restatement.py ("linear", "none").
"""
from __future__ import annotations

import torch

from tests.ghmfc_train_restatement import mention_repr
from tests.ghmfc_variant_restatement import variant_mention


def token_slice(emask, T: int):
    """bool [B, N, T]: the positions of 1 : ntok - 1 (ntok == 0: the stop -1 counts from the end; 1 or 2: empty)"""
    ntok = emask.sum(-1)
    stop = ntok - 1
    stop = torch.where(stop < 0, stop + T, stop).clamp(0, T)
    pos = torch.arange(T, device=emask.device)
    return (pos >= 1) & (pos[None, None, :] < stop[:, :, None])


def pooled_entities(ef, emask, pooling: str):
    """[B, N, D] of token features [B, N, T, D]; an empty slice gives a NaN row under either pooling (the mean's 0 / 0; the
    reference's max raises IndexError there - the library's stated answer is the NaN row)."""
    inside = token_slice(emask, ef.shape[2])
    if pooling == "avg":
        w = inside.to(ef.dtype)
        return (ef * w[..., None]).sum(2) / w.sum(2)[..., None]
    # where, not masked_fill on a copy: the gradient of a maximum goes to the position that attains it
    top = torch.where(inside[..., None], ef, torch.full_like(ef, float("-inf"))).max(2).values
    return torch.where(inside.any(-1)[..., None], top, torch.full_like(top, float("nan")))


def entity_repr(batch, sd, pooling: str = "avg"):
    """the entity encoder's output [B, N, D]; the final layer is Identity when `sd` holds no entity weight"""
    ef, emask = batch[5], batch[6]
    if ef.dim() == 4:
        ef = pooled_entities(ef, emask, pooling)
    w = sd.get("entity_encoder.final_layer.weight")
    return ef if w is None else ef @ w.T + sd["entity_encoder.final_layer.bias"]


def entity_case_scores(batch, sd, enc: str, rep: str, pooling: str, heads: int, eps: float = 1e-8, idx_text=None, idx_image=None):
    """(scores [B, N], mention_repr [B, D], entity_repr [B, N, D]); enc: "bi" (the default fusion) | "linear" | "none";
    idx_text / idx_image: the positions the default encoder's two maxima are taken at (a model's `max_indices`), else the argmax"""
    m = mention_repr(batch, sd, heads, idx_text, idx_image) if enc == "bi" else variant_mention(batch, sd, enc, rep, heads)
    e = entity_repr(batch, sd, pooling)
    dot = (m[:, None, :] * e).sum(-1)
    return dot / (m.norm(dim=-1).clamp_min(eps)[:, None] * e.norm(dim=-1).clamp_min(eps)), m, e
