"""Deterministic batches for the golden cases of GHMFC's other mention encoders (tools/gen_ghmfc_variant_golden.py) and the
tests that read them, in the style of tests/ghmfc_inputs.py: numpy Philox streams keyed by the case name; the weights come from
`torch.manual_seed(seed)`.

The cases cover what the variants add: the four encoders with both final representations, relu and gelu FFNs, mask lengths 1,
L and in between, a padded token row scaled so that a padded position wins the max (the generator checks that one does), spans
of length 1, reaching into the padding, the full sentence, `end > L` and an EMPTY span (a NaN row, in the golden too), an
all-zero mask row for the "text" encoder (never for the transformer: torch has two answers there), WikiMEL token entities, head
dim 5, a key length past one tile, products past the 256-row split-bf16 gate, and the reference widths with 8 layers.
"""
from __future__ import annotations

import numpy as np

TINY = dict(D=16, R=32, H=2, L=12, P=3, N=4, layers=2, ffn=24)
FULL = dict(D=768, R=2048, H=8, L=128, P=49, N=11, layers=8, ffn=512)

# name -> B, weight seed, encoder ("transformer" | "text" | "linear" | "none"), repr ("max" | "avg"), FFN activation, mask and
# span layouts, geometry, T (WikiMEL tokens)
CASES = {
    "tr_max_b3": dict(B=3, seed=31, enc="transformer", repr="max", act="gelu", masks="corners", spans="simple"),
    "tr_avg_b5": dict(B=5, seed=32, enc="transformer", repr="avg", act="relu", masks="mixed", spans="forms"),
    "tr_wm_t6": dict(B=3, seed=33, enc="transformer", repr="max", act="gelu", masks="mixed", spans="simple", T=6),
    "text_max_b3": dict(B=3, seed=34, enc="text", repr="max", masks="zero_row", spans="simple"),
    "text_avg_b3": dict(B=3, seed=35, enc="text", repr="avg", masks="zero_row", spans="simple"),
    "linear_b5": dict(B=5, seed=36, enc="linear", repr="avg", masks="mixed", spans="forms"),
    "none_max_b3": dict(B=3, seed=37, enc="none", repr="max", masks="mixed", spans="simple"),
    "none_avg_b3": dict(B=3, seed=38, enc="none", repr="avg", masks="mixed", spans="simple"),
    "tr_heads_5": dict(B=3, seed=39, enc="transformer", repr="max", act="gelu", masks="mixed", spans="simple",
                       geom=dict(D=20, R=36, H=4, L=12, P=3, N=4, layers=2, ffn=28)),
    "tr_long_200": dict(B=2, seed=40, enc="transformer", repr="avg", act="gelu", masks="mixed", spans="simple",
                        geom=dict(D=16, R=32, H=2, L=200, P=3, N=4, layers=2, ffn=24)),
    "tr_gates": dict(B=8, seed=41, enc="transformer", repr="max", act="gelu", masks="mixed", spans="simple",
                     geom=dict(D=128, R=32, H=2, L=128, P=3, N=4, layers=2, ffn=256)),
    "tr_full_max_b2": dict(B=2, seed=42, enc="transformer", repr="max", act="gelu", masks="mixed", spans="simple", geom=FULL),
    "tr_full_avg_b2": dict(B=2, seed=43, enc="transformer", repr="avg", act="gelu", masks="mixed", spans="simple", geom=FULL),
}
TINY_CASES = [n for n, c in CASES.items() if "geom" not in c]
SHAPE_CASES = ["tr_heads_5", "tr_long_200", "tr_gates"]
FULL_CASES = ["tr_full_max_b2", "tr_full_avg_b2"]
GOLDEN_FILE = {**{n: "ghmfc_variants_tiny.npz" for n in TINY_CASES}, **{n: "ghmfc_variants_shapes.npz" for n in SHAPE_CASES},
               **{n: "ghmfc_variants_full.npz" for n in FULL_CASES}}

# "corners" (tr_max_b3): mask length 1, length L, and a padded token row scaled to win the max
PADDED_MAX_ROW, PADDED_MAX_LEN, PADDED_MAX_TOKEN, PADDED_MAX_SCALE = 2, 5, 8, 6.0
ZERO_MASK_ROW = 1                        # "zero_row" (the text cases): this mention's mask is all zero
# "forms" (B = 5, L = 12): (mask length, begin, end) - a span of length 1, one reaching into the padding, the full sentence,
# end > L, and an empty one
SPAN_FORMS = [(7, 1, 2), (5, 3, 9), (12, 0, 12), (10, 8, 20), (6, 4, 4)]
EMPTY_SPAN_ROW = 4

_LAYER_KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
               "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
               "norm2.bias"]
_CROSS_KEYS = (["a2b_attention.q_proj_weight", "a2b_attention.k_proj_weight", "a2b_attention.v_proj_weight",
                "a2b_attention.in_proj_bias", "a2b_attention.out_proj.weight", "a2b_attention.out_proj.bias", "a2b_ffn.weight",
                "a2b_ffn.bias", "b2a_attention.in_proj_weight", "b2a_attention.in_proj_bias", "b2a_attention.out_proj.weight",
                "b2a_attention.out_proj.bias", "b2a_ffn.weight", "b2a_ffn.bias"]
               + [f"layernorms.{i}.{n}" for i in range(4) for n in ("weight", "bias")])
TRANSFORMER = "mention_encoder.intermediate_layer.transformer."
CROSS = "mention_encoder.intermediate_layer."
ENTITY_KEYS = ["entity_encoder.final_layer.weight", "entity_encoder.final_layer.bias"]


# no goldens: the ten-Adam-step test's batch (tr_avg_b5's encoder at B = 16)
TRAIN_CASES = {"tr_adam_b16": dict(B=16, seed=44, enc="transformer", repr="avg", act="relu", masks="mixed", spans="simple")}


def case_of(name: str) -> dict:
    return CASES[name] if name in CASES else TRAIN_CASES[name]


def geometry(name: str) -> dict:
    return case_of(name).get("geom", TINY)


def dataset_of(name: str) -> str:
    return "wikimel" if "T" in case_of(name) else "wikidiverse"


def reference_names(name: str) -> dict:
    """the names of common/args.py that select this case's encoder"""
    case = case_of(name)
    enc = case["enc"]
    return dict(mention_final_layer_name="multimodal" if enc == "text" else enc, mention_multimodal_attention="text" if enc == "text" else "bi",
                mention_final_representation="max pool" if case["repr"] == "max" else "avg extract",
                transformer_ffn_activation=case.get("act", "gelu"))


def keys_for(enc: str, layers: int) -> list:
    """the reference's state-dict keys of an encoder, in order"""
    if enc == "transformer":
        return [f"{TRANSFORMER}layers.{i}.{k}" for i in range(layers) for k in _LAYER_KEYS] + ENTITY_KEYS
    if enc == "text":
        return [CROSS + k for k in _CROSS_KEYS] + ENTITY_KEYS
    if enc == "linear":
        return ["mention_encoder.final_layer.linear.weight", "mention_encoder.final_layer.linear.bias"] + ENTITY_KEYS
    return list(ENTITY_KEYS)


def case_keys(name: str) -> list:
    return keys_for(case_of(name)["enc"], geometry(name)["layers"])


def _rng(name: str, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)), stream]))


def mask_lengths(name: str) -> np.ndarray:
    case, L = case_of(name), geometry(name)["L"]
    mlen = _rng(name, 2).integers(1, L + 1, size=case["B"])
    if case["masks"] == "corners":
        mlen[0], mlen[1], mlen[PADDED_MAX_ROW] = 1, L, PADDED_MAX_LEN
    elif case["masks"] == "zero_row":
        mlen[ZERO_MASK_ROW] = 0
    if case["spans"] == "forms":
        mlen[:] = [f[0] for f in SPAN_FORMS]
    return mlen.astype(np.int64)


def spans(name: str):
    case, L = case_of(name), geometry(name)["L"]
    if case["spans"] == "forms":
        return (np.array([f[1] for f in SPAN_FORMS], dtype=np.int64), np.array([f[2] for f in SPAN_FORMS], dtype=np.int64))
    r = _rng(name, 3)
    begin = r.integers(0, L, size=case["B"])
    return begin.astype(np.int64), (begin + r.integers(1, 5, size=case["B"])).astype(np.int64)     # (end may pass L: clipped)


def variant_inputs(name: str):
    """The 8-item offline batch of case `name`: numpy float32 / int64 arrays; mention_image is the loader's scalar 0 unless the
    encoder is "text", entity_image the scalar 0, entity_mask the scalar 0 on WikiDiverse."""
    case, g = case_of(name), geometry(name)
    B, D, R, L, P, N = case["B"], g["D"], g["R"], g["L"], g["P"], g["N"]
    r = _rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32)) if case["enc"] == "text" else 0
    mlen = mask_lengths(name)
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    if case["masks"] == "corners":
        mf[PADDED_MAX_ROW, PADDED_MAX_TOKEN] *= PADDED_MAX_SCALE
    begin, end = spans(name)
    if "T" in case:
        T = case["T"]
        ef = r.standard_normal((B, N, T, D), dtype=np.float32)
        ntok = 3 + (np.arange(B * N) % (T - 2)).reshape(B, N)          # 3 .. T tokens: every slice 1 : ntok - 1 holds a token
        emask = (np.arange(T)[None, None, :] < ntok[:, :, None]).astype(np.int64)
    else:
        ef = r.standard_normal((B, N, D), dtype=np.float32)
        emask = 0
    return [mf, mmask, begin, end, mimage, ef, emask, 0]
