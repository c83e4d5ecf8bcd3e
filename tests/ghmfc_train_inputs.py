"""Deterministic GHMFC batches for the training tests beyond tests/ghmfc_inputs.py's cases, generated the same way (numpy
Philox streams keyed by the case name; weights from `torch.manual_seed(seed)`):

- `wm_t6`: WikiMEL token blocks [B, N, 6, D] whose entities all have 3 .. 6 tokens, so no row is NaN (`wm_b3` has 2-token
  entities, whose empty token slice is a NaN row in the reference too) and every gradient is finite;
- `gates`: B = 8, L = 128, P = 49, D = 128, R = 256, H = 2 - row counts and widths at which the linear products cross the
  split-bf16 size gates of the GEMM module;
- `full_b2`: the reference widths at B = 2;
- `adam_b16`: the tiny geometry at B = 16 with mixed masks, for the optimiser trajectory.
"""
from __future__ import annotations

import numpy as np

from tests.ghmfc_inputs import FULL, TINY, _rng

WM_CASE = dict(B=3, seed=13, geom=TINY, T=6)
TRAIN_CASES = {
    "wm_t6": WM_CASE,
    "gates": dict(B=8, seed=14, geom=dict(D=128, R=256, H=2, L=128, P=49, N=4)),
    "full_b2": dict(B=2, seed=15, geom=FULL),
    "adam_b16": dict(B=16, seed=16, geom=TINY),
}


def train_inputs(name: str):
    """The 8-item offline batch of TRAIN_CASES[name], laid out as tests/ghmfc_inputs.ghmfc_inputs does."""
    case = TRAIN_CASES[name]
    g = case["geom"]
    B, D, R, L, P, N = case["B"], g["D"], g["R"], g["L"], g["P"], g["N"]
    r = _rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32))
    mlen = _rng(name, 2).integers(1, L + 1, size=B).astype(np.int64)
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    begin, end = np.ones(B, dtype=np.int64), np.full(B, 2, dtype=np.int64)
    if "T" in case:
        T = case["T"]
        ef = r.standard_normal((B, N, T, D), dtype=np.float32)
        ntok = 3 + (np.arange(B * N) % (T - 2)).reshape(B, N)          # 3 .. T: tokens 1 : ntok - 1 are never empty
        emask = (np.arange(T)[None, None, :] < ntok[:, :, None]).astype(np.int64)
    else:
        ef = r.standard_normal((B, N, D), dtype=np.float32)
        emask = 0
    return [mf, mmask, begin, end, mimage, ef, emask, 0]


def wikimel_no_nan_batch():
    return train_inputs("wm_t6")
