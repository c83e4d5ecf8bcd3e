"""Deterministic batches for the golden cases of GHMFC's entity encoder settings (tools/gen_ghmfc_entity_golden.py:
`entity_final_pooling` "max", `entity_final_layer_name` "none") and the tests that read them, in the style of
tests/ghmfc_variant_inputs.py: numpy Philox streams keyed by the case name; the weights come from `torch.manual_seed(seed)`.

The tiny WikiMEL cases share one token-count table: 0 tokens (the Python slice 1 : -1), 3 (one row), T, values in between, and
one pair whose mask is no prefix (only its sum counts).  No golden case holds 1 or 2 tokens: the reference raises IndexError on
an empty max (the library writes a NaN row there; tests/test_gpu_ghmfc_entity.py builds that batch itself).
"""
from __future__ import annotations

import numpy as np

from tests.ghmfc_inputs import KEYS as BI_KEYS
from tests.ghmfc_variant_inputs import ENTITY_KEYS, TINY, keys_for

# name -> B, weight seed, mention encoder ("bi" | "linear" | "none"), its final representation, the two entity names, T (WikiMEL
# tokens; absent: WikiDiverse), geometry
CASES = {
    "wm_max_linear": dict(B=3, seed=51, enc="bi", repr="max", pooling="max", layer="linear", T=8),
    "wm_max_none": dict(B=3, seed=52, enc="bi", repr="max", pooling="max", layer="none", T=8),
    "wm_avg_none": dict(B=3, seed=53, enc="bi", repr="max", pooling="avg", layer="none", T=8),
    "wm_lin_max_linear": dict(B=3, seed=54, enc="linear", repr="avg", pooling="max", layer="linear", T=8),
    "wm_bare_max_none": dict(B=3, seed=55, enc="none", repr="avg", pooling="max", layer="none", T=8),     # no parameter at all
    "wd_avg_none": dict(B=3, seed=56, enc="bi", repr="max", pooling="avg", layer="none"),
    # 320 entity rows: past the 256-row split-bf16 gate of the product; T = 20: two unrolled 8-row trips and a remainder
    "gate_max_linear": dict(B=8, seed=57, enc="bi", repr="max", pooling="max", layer="linear", T=20,
                            geom=dict(D=128, R=32, H=2, L=12, P=3, N=40, layers=2, ffn=24)),
    "full_max_linear": dict(B=2, seed=58, enc="bi", repr="max", pooling="max", layer="linear", T=64,
                            geom=dict(D=768, R=2048, H=8, L=128, P=49, N=101, layers=8, ffn=512)),
}
TINY_CASES = [n for n, c in CASES.items() if "geom" not in c]
GOLDEN_FILE = "ghmfc_entity.npz"

# the tiny WikiMEL cases (B * N = 12 pairs, T = 8): tokens per pair, and the pair whose mask is not a prefix
TINY_NTOK = [0, 3, 8, 4, 5, 6, 7, 3, 8, 5, 4, 6]
SCATTERED_PAIR, SCATTERED_MASK = 3, [1, 0, 1, 1, 0, 1, 0, 0]


def geometry(name: str) -> dict:
    return CASES[name].get("geom", TINY)


def dataset_of(name: str) -> str:
    return "wikimel" if "T" in CASES[name] else "wikidiverse"


def reference_names(name: str) -> dict:
    """the names of common/args.py that select this case's encoders"""
    case = CASES[name]
    enc = case["enc"]
    return dict(mention_final_layer_name="multimodal" if enc == "bi" else enc, mention_multimodal_attention="bi",
                mention_final_representation="max pool" if case["repr"] == "max" else "avg extract", transformer_ffn_activation="gelu",
                entity_final_layer_name=case["layer"], entity_final_pooling=case["pooling"])


def case_keys(name: str) -> list:
    """the reference's state-dict keys, in order: 52 (50 without the entity Linear) for the default mention encoder"""
    case = CASES[name]
    keys = list(BI_KEYS) if case["enc"] == "bi" else keys_for(case["enc"], 0)
    return keys if case["layer"] == "linear" else [k for k in keys if k not in ENTITY_KEYS]


def _rng(name: str, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)), stream]))


def token_counts(name: str) -> np.ndarray:
    """[B, N] tokens per pair of a WikiMEL case"""
    case, g = CASES[name], geometry(name)
    B, N, T = case["B"], g["N"], case["T"]
    if "geom" not in case:
        return np.array(TINY_NTOK, dtype=np.int64).reshape(B, N)
    return (3 + (np.arange(B * N) % (T - 2))).reshape(B, N).astype(np.int64)          # 3 .. T


def entity_inputs(name: str):
    """The 8-item offline batch of case `name`: numpy float32 / int64 arrays; mention_image is the loader's scalar 0 unless the
    mention encoder is the default one, entity_image the scalar 0, entity_mask the scalar 0 on WikiDiverse."""
    case, g = CASES[name], geometry(name)
    B, D, R, L, P, N = case["B"], g["D"], g["R"], g["L"], g["P"], g["N"]
    r = _rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32)) if case["enc"] == "bi" else 0
    mlen = _rng(name, 2).integers(1, L + 1, size=B).astype(np.int64)
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    r3 = _rng(name, 3)
    begin = r3.integers(0, L, size=B).astype(np.int64)
    end = (begin + r3.integers(1, 5, size=B)).astype(np.int64)                          # (end may pass L: clipped)
    if "T" in case:
        T = case["T"]
        ef = r.standard_normal((B, N, T, D), dtype=np.float32)
        emask = (np.arange(T)[None, None, :] < token_counts(name)[:, :, None]).astype(np.int64)
        if "geom" not in case:
            emask.reshape(B * N, T)[SCATTERED_PAIR] = SCATTERED_MASK
            assert (emask.sum(-1) == token_counts(name)).all()
    else:
        ef = r.standard_normal((B, N, D), dtype=np.float32)
        emask = 0
    return [mf, mmask, begin, end, mimage, ef, emask, 0]
