"""Deterministic inputs of the GHMFC table-form tests (tests/test_gpu_ghmfc_table.py, tests/test_ghmfc_table_host.py): numpy
Philox streams keyed by the case name, as tests/ghmfc_inputs.py does it, so every array is regenerated bit for bit anywhere.

A case is a mention side in the reference's offline layout, an entity table `[E, T, D]` + mask `[E, T]` (or pooled `[E, D]`,
`T = 0`) and candidate rows `[B, N]` that repeat an entity within a mention and across mentions, in unsorted order.  `nan_row`:
entity 0 has two tokens - tokens 1 : 1 are an empty slice, a NaN row, as in the reference.
"""
from __future__ import annotations

import json
import os

import numpy as np

TINY = dict(D=16, R=32, H=2, L=12, P=3, N=4)
REFERENCE = dict(D=768, R=2048, H=8, L=128, P=49, N=101)

TABLE_CASES = {
    "tiny_b3": dict(B=3, seed=21, geom=TINY, E=9, T=6, nan_row=True),
    "tiny_b300": dict(B=300, seed=22, geom=TINY, E=9, T=6, nan_row=True),        # past the 256-mention chunk
    "tiny_pooled_b3": dict(B=3, seed=23, geom=TINY, E=9, T=0),
    "tiny_pooled_b300": dict(B=300, seed=24, geom=TINY, E=9, T=0),
    "tiny_clean_b3": dict(B=3, seed=25, geom=TINY, E=9, T=6),                     # no NaN row: the training steps
    "reference_b2": dict(B=2, seed=26, geom=REFERENCE, E=150, T=64),
}


def rng(name: str, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)), stream]))


def entity_table(name: str, E: int, T: int, D: int, nan_row: bool = False):
    """(text [E, T, D] float32, mask [E, T] int64) with 3 .. T tokens per entity, or (text [E, D], None) for T = 0."""
    r = rng(name, 11)
    if T == 0:
        return r.standard_normal((E, D), dtype=np.float32), None
    text = r.standard_normal((E, T, D), dtype=np.float32)
    ntok = 3 + (np.arange(E) * 5) % (T - 2)
    if nan_row:
        ntok[0] = 2
    return text, (np.arange(T)[None, :] < ntok[:, None]).astype(np.int64)


def candidate_rows(name: str, B: int, N: int, E: int) -> np.ndarray:
    """[B, N] int64 in [0, E - 1]: random, with an entity repeated inside mention 0 and shared by mentions 0 and B - 1."""
    cand = rng(name, 12).integers(0, E, size=(B, N)).astype(np.int64)
    cand[0, N - 1] = cand[0, 0]
    cand[B - 1, 0] = cand[0, 0]
    if N > 2:
        cand[0, 1] = E - 1
    return cand


def table_case(name: str):
    """(mention: the five mention-side items, text, mask or None, candidates) of TABLE_CASES[name] as numpy arrays."""
    case = TABLE_CASES[name]
    g, B = case["geom"], case["B"]
    D, R, L, P, N = g["D"], g["R"], g["L"], g["P"], g["N"]
    r = rng(name, 1)
    mf = r.standard_normal((B, L, D), dtype=np.float32)
    mimage = np.abs(r.standard_normal((B, P, R), dtype=np.float32))
    mlen = r.integers(1, L + 1, size=B)
    mlen[0] = L
    mmask = (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64)
    begin = np.ones(B, dtype=np.int64)
    end = np.minimum(mlen, 3).astype(np.int64) + 1                     # the mention span 1 : end (avg extract)
    text, mask = entity_table(name, case["E"], case["T"], D, case.get("nan_row", False))
    return [mf, mmask, begin, end, mimage], text, mask, candidate_rows(name, B, N, case["E"])


def gathered(mention, text, mask, cand):
    """The reference's 8-item batch: what the loader's qid2idx gather delivers."""
    return list(mention) + [text[cand], mask[cand] if mask is not None else 0, 0]


# ---- a tiny dataset in the files ghmfc_shim.GhmfcData reads (WikiMEL layout) ---------------------------------------------
def write_wikimel_dataset(root: str, sizes=(7, 3, 2), N: int = 4, D: int = 16, R: int = 32, L: int = 12, P: int = 3, E: int = 9, T: int = 6,
                          entity_features: bool = True) -> dict:
    """Writes the split files and the shared table; returns {"qids": [...], "pick": {split: [m, N] table rows}}.
    `entity_features=False` leaves `entity-attr-feature.npy` out: a loader that opens it fails."""
    os.makedirs(root, exist_ok=True)
    save = lambda name, a: np.save(os.path.join(root, name), a)   # noqa: E731
    text, mask = entity_table("dataset", E, T, D)
    if entity_features:
        save("entity-attr-feature.npy", text)
    save("entity-attr-mask.npy", mask)
    qids = [f"Q{1000 + 13 * i}" for i in range(E)]
    order = list(rng("dataset", 13).permutation(E))                     # qid2idx is not the identity on the QID order
    with open(os.path.join(root, "qid2idx.json"), "w") as f:
        json.dump({qids[i]: int(order[i]) for i in range(E)}, f)
    picks = {}
    for k, (split, m) in enumerate(zip(("train", "valid", "test"), sizes)):
        r = rng("dataset", 20 + k)
        save(f"mention-text-feature_{split}.npy", r.standard_normal((m, L, D), dtype=np.float32))
        mlen = r.integers(1, L + 1, size=m)
        save(f"mention-text-mask_{split}.npy", (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64))
        save(f"start-pos_{split}.npy", np.zeros(m, dtype=np.int64))
        save(f"end-pos_{split}.npy", np.minimum(mlen, 2).astype(np.int64))
        save(f"mention-image-feature_{split}.npy", np.abs(r.standard_normal((m, P, R), dtype=np.float32)))
        save(f"answer_{split}.npy", r.integers(0, N, size=m).astype(np.int64))
        pick = r.integers(0, E, size=(m, N))
        save(f"entity-name-raw_{split}.npy", np.array(qids)[pick].reshape(-1))
        picks[split] = np.asarray(order, dtype=np.int64)[pick]
    return {"qids": qids, "pick": picks}
