"""Deterministic MELHI batches for the golden cases (tools/gen_melhi_golden.py) and the tests that read them: numpy Philox
streams keyed by the case name, so a batch is regenerated bit for bit anywhere.  The cases cover the extraction rule's
corners: B = 1 (the row is the true last output), tie-heavy orders at B = 64 and 300 (ties at the longest length too),
all-placeholder sides, an empty mention span (a NaN row), and image masks all on, all off and mixed.

A case runs at the TINY widths, at the reference's (`full`), or at a geometry of its own (`geom`: the shape cases of
tests/golden/melhi_shapes.npz - widths off the GEMM tiles, one candidate and one region, L = 3 and L = 300 contexts, the
validated maximum left length, D = 1024)."""
from __future__ import annotations

import numpy as np
import torch

KEYS = ["image_map_text.weight", "image_map_text.bias", "mention_encoder.mention_lstm.weight_ih_l0",
        "mention_encoder.mention_lstm.weight_hh_l0", "mention_encoder.mention_lstm.bias_ih_l0",
        "mention_encoder.mention_lstm.bias_hh_l0", "mention_encoder.mention_final_map.weight",
        "mention_encoder.mention_final_map.bias", "entity_final_map.weight", "entity_final_map.bias"]

TINY = dict(D=16, R=32, L=12, P=3, N=4)
FULL = dict(D=768, R=2048, L=128, P=49, N=11)

# name -> B, weight seed, layout of the spans, thresholds; "mixed" = half of the mentions get an image that passes the mask
CASES = {
    "b1": dict(B=1, seed=1, spans="random"),
    "b1_placeholder": dict(B=1, seed=2, spans="placeholder"),
    "b4": dict(B=4, seed=3, spans="random", image="mixed"),
    "b64_ties": dict(B=64, seed=4, spans="ties", image="mixed"),
    "b300_ties": dict(B=300, seed=5, spans="ties", image="mixed"),
    "b64_top_ties": dict(B=64, seed=6, spans="top_ties"),
    "b32_all_placeholder": dict(B=32, seed=7, spans="placeholder", image="mixed"),
    "b16_empty_span": dict(B=16, seed=8, spans="empty_span"),
    "b16_mask_on": dict(B=16, seed=9, spans="random", thres=(-2.0, -2.0)),
    "b16_mask_off": dict(B=16, seed=10, spans="random", thres=(2.0, 2.0)),
    "full_b4": dict(B=4, seed=11, spans="random", image="mixed", full=True),
    "full_b64": dict(B=64, seed=12, spans="ties", image="mixed", full=True),
    # shape cases: one geometry each
    "odd_w": dict(B=64, seed=13, spans="ties", image="mixed", geom=dict(D=20, R=36, L=12, P=1, N=1)),
    "short_L": dict(B=300, seed=14, spans="short", image="mixed", geom=dict(D=32, R=260, L=3, P=5, N=3)),
    "long_lanes": dict(B=8, seed=15, spans="long_lanes", image="mixed", geom=dict(D=32, R=64, L=300, P=2, N=4)),
    "max_len_nan": dict(B=64, seed=16, spans="max_len_nan", image="mixed", geom=dict(D=20, R=36, L=12, P=3, N=4)),
    "wide_D": dict(B=128, seed=17, spans="ties", image="mixed", geom=dict(D=1024, R=128, L=16, P=2, N=8)),
}
SHAPE_CASES = [n for n, c in CASES.items() if "geom" in c]
# gradient goldens in full for the small shape widths, in the checksum form of melhi_full.npz for wide_D, none for a case
# whose scores hold NaN
SHAPE_CHECKSUM = ("wide_D",)
SHAPE_FORWARD_ONLY = ("max_len_nan",)


def geometry(name: str) -> dict:
    """D, R, L, P, N of case `name`."""
    case = CASES[name]
    return case["geom"] if "geom" in case else (FULL if case.get("full", False) else TINY)


def _rng(name: str, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)), stream]))


def grad_weights(name: str, shape) -> np.ndarray:
    return _rng(name, 99).standard_normal(size=tuple(shape), dtype=np.float32)


def melhi_inputs(name: str, sd: dict):
    """The 8-item batch of case `name` (numpy float32 / int64 arrays; entity_mask is the int 0 of the WikiDiverse loader).
    `sd`: the case's state dict, used to aim the "mixed" images at the mask's thresholds."""
    case = CASES[name]
    g = geometry(name)
    B, D, R, L, P, N = case["B"], g["D"], g["R"], g["L"], g["P"], g["N"]
    r = _rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32))
    ef = r.standard_normal((B, N, D), dtype=np.float32)
    eimage = r.standard_normal((B, N, R), dtype=np.float32)
    spans = case["spans"]
    mlen = r.integers(2, L + 1, size=B)
    if spans == "random":
        s = r.integers(0, L - 2, size=B)
        e = s + r.integers(1, 3, size=B)
    elif spans == "ties":      # many left placeholders (start <= 1) and repeated right lengths
        s = np.where(r.random(B) < 0.4, 0, r.integers(1, 4, size=B))
        e = s + 1
        mlen = np.minimum(e + 1 + r.integers(0, 3, size=B), L)
    elif spans == "top_ties":  # several sequences of the longest length on both sides
        s = np.where(r.random(B) < 0.5, L - 4, r.integers(0, 3, size=B))
        e = np.minimum(s + 1, L - 2)
        mlen = np.where(r.random(B) < 0.5, L, e + 2)
    elif spans == "short":     # L = 3: every context has length <= 1, real ones on both sides
        s = r.integers(0, 2, size=B)   # start 1 (left placeholder) or 2 (left token 1)
        e = s + 1
        mlen = np.where(s == 0, r.integers(2, 4, size=B), L)   # start 1, end 2 with a full mask: right token 2
    elif spans in ("long_lanes", "max_len_nan"):   # "ties", plus the longest contexts the validation admits
        s = np.where(r.random(B) < 0.4, 0, r.integers(1, 4, size=B))
        e = s + 1
        mlen = np.minimum(e + 1 + r.integers(0, 3, size=B), L)
        if spans == "long_lanes":
            s[0], e[0] = L - 2, L - 1                   # start L - 1, end L: left context 1 .. L - 2
            s[1], e[1], mlen[1] = 0, 1, L               # start 1, end 2, full mask: right context 2 .. L - 1
        else:
            s[::11] = e[::11] = L - 1                   # start = end = L: left length L - 1, an empty span (a NaN row)
    elif spans == "placeholder":   # both contexts empty everywhere
        s = np.zeros(B, dtype=np.int64)
        e = s + 1
        mlen = e.copy()
    elif spans == "empty_span":
        s = r.integers(0, L - 3, size=B)
        e = s + r.integers(1, 3, size=B)
        e[::5] = s[::5]          # start == end after the +1 shift: torch.mean of an empty slice is NaN
    else:
        raise ValueError(spans)
    mlen = np.clip(mlen, 1, L)
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    start, end = (s + 1).astype(np.int64), (e + 1).astype(np.int64)   # baselines/data.py applies the CLS shift
    if case.get("image") == "mixed":
        # half of the mentions: token 0 along the mapped mention image and one candidate image along the mention image
        w = np.asarray(sd["image_map_text.weight"], dtype=np.float32)
        b = np.asarray(sd["image_map_text.bias"], dtype=np.float32)
        on = np.arange(B) % 2 == 0
        mimg = mimage.mean(1)
        mf[on, 0] = (mimg @ w.T + b)[on] + 0.3 * mf[on, 0]
        n1 = min(1, N - 1)
        eimage[on, n1] = mimg[on] + 0.1 * eimage[on, n1]
    return [mf, mmask, torch.from_numpy(start), torch.from_numpy(end), mimage, ef, 0, eimage]
