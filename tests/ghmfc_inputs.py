"""Deterministic GHMFC batches for the golden cases (tools/gen_ghmfc_golden.py) and the tests that read them: numpy Philox
streams keyed by the case name, so a batch is regenerated bit for bit anywhere; the weights come from `torch.manual_seed(seed)`.

The cases cover what the forward can get wrong: mention masks of length 1, L and in between, a mention whose mask is all zero
(zero attention weights wherever the text is the key: finite scores), a mention with a scaled PADDED token row (padded query
positions take part in the max over the sequence: the generator checks that one wins), WikiMEL token blocks with 2 .. T tokens
(tokens 1 : ntok - 1 of a 2-token entity are an empty slice: a NaN row, in the golden too), head dims 5 and 9, single token /
region / candidate, key lengths past one wave and one key tile, a batch past the 256-mention chunk, and the reference widths.
"""
from __future__ import annotations

import numpy as np

TINY = dict(D=16, R=32, H=2, L=12, P=3, N=4)
FULL = dict(D=768, R=2048, H=8, L=128, P=49, N=11)

# name -> B, weight seed, dataset ("wd" WikiDiverse [B, N, D] | "wm" WikiMEL [B, N, T, D]), geometry, mask layout
CASES = {
    "wd_b1": dict(B=1, seed=1, masks="mixed"),
    "wd_b5": dict(B=5, seed=2, masks="corners"),
    "wm_b3": dict(B=3, seed=3, masks="mixed", T=6),
    "heads_5_9": dict(B=3, seed=4, masks="mixed", geom=dict(D=20, R=36, H=4, L=12, P=3, N=4)),
    "ones": dict(B=2, seed=5, masks="full", geom=dict(D=16, R=32, H=2, L=1, P=1, N=1)),
    "long_200": dict(B=2, seed=6, masks="mixed", geom=dict(D=16, R=32, H=2, L=200, P=3, N=4)),
    "long_512": dict(B=2, seed=7, masks="mixed", geom=dict(D=16, R=32, H=2, L=512, P=3, N=4)),
    "b300": dict(B=300, seed=8, masks="mixed"),
    "full_b4": dict(B=4, seed=9, masks="mixed", geom=FULL),
    "full_b64": dict(B=64, seed=10, masks="mixed", geom=FULL),
}
# rows of wd_b5: mask length 1, length L, all zero, a padded token row scaled to win the max, random
ALL_ZERO_ROW, PADDED_MAX_ROW = 2, 3
PADDED_MAX_LEN, PADDED_MAX_TOKEN, PADDED_MAX_SCALE = 5, 8, 6.0

KEYS_PER_CROSS = (["a2b_attention.q_proj_weight", "a2b_attention.k_proj_weight", "a2b_attention.v_proj_weight",
                   "a2b_attention.in_proj_bias", "a2b_attention.out_proj.weight", "a2b_attention.out_proj.bias", "a2b_ffn.weight",
                   "a2b_ffn.bias", "b2a_attention.in_proj_weight", "b2a_attention.in_proj_bias", "b2a_attention.out_proj.weight",
                   "b2a_attention.out_proj.bias", "b2a_ffn.weight", "b2a_ffn.bias"]
                  + [f"layernorms.{i}.{n}" for i in range(4) for n in ("weight", "bias")])
_FUSION = "mention_encoder.intermediate_layer."
KEYS = ([_FUSION + "t2v_attention." + k for k in KEYS_PER_CROSS] + [_FUSION + "v2t_attention." + k for k in KEYS_PER_CROSS]
        + [_FUSION + f"{m}.{n}" for m in ("text_linear", "image_linear", "score_linear") for n in ("weight", "bias")]
        + ["entity_encoder.final_layer.weight", "entity_encoder.final_layer.bias"])


def geometry(name: str) -> dict:
    return CASES[name].get("geom", TINY)


def dataset_of(name: str) -> str:
    return "wikimel" if "T" in CASES[name] else "wikidiverse"


def _rng(name: str, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)), stream]))


def mask_lengths(name: str) -> np.ndarray:
    case, g = CASES[name], geometry(name)
    B, L = case["B"], g["L"]
    r = _rng(name, 2)
    if case["masks"] == "full":
        return np.full(B, L, dtype=np.int64)
    mlen = r.integers(1, L + 1, size=B)
    if case["masks"] == "corners":
        mlen[0], mlen[1], mlen[ALL_ZERO_ROW], mlen[PADDED_MAX_ROW] = 1, L, 0, PADDED_MAX_LEN
    return mlen.astype(np.int64)


def ghmfc_inputs(name: str):
    """The 8-item offline batch of case `name`: numpy float32 / int64 arrays; begin / end (not read) are int64 [B], entity_image
    is the loader's scalar 0, entity_mask the scalar 0 on WikiDiverse."""
    case, g = CASES[name], geometry(name)
    B, D, R, L, P, N = case["B"], g["D"], g["R"], g["L"], g["P"], g["N"]
    r = _rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32))
    mlen = mask_lengths(name)
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    if case["masks"] == "corners":
        mf[PADDED_MAX_ROW, PADDED_MAX_TOKEN] *= PADDED_MAX_SCALE
    begin, end = np.ones(B, dtype=np.int64), np.full(B, 2, dtype=np.int64)
    if "T" in case:
        T = case["T"]
        ef = r.standard_normal((B, N, T, D), dtype=np.float32)
        ntok = 2 + (np.arange(B * N) % (T - 1)).reshape(B, N)          # 2 .. T: the first entity's slice 1 : 1 is empty
        emask = (np.arange(T)[None, None, :] < ntok[:, :, None]).astype(np.int64)
    else:
        ef = r.standard_normal((B, N, D), dtype=np.float32)
        emask = 0
    return [mf, mmask, begin, end, mimage, ef, emask, 0]
