"""What the summed-cosine top-k computes, restated plainly on the host in fp64: the score
`sum_s w_s cos(x_s[b], rows_s[e])`, the combine's formula, the fp32 chain the returned scores are held to bit for bit, and the
small cases the host and the GPU tests share - drawn once per case, left unchanged.  The margins the selection rule relies on
(how many rows lie within the tolerance of the k-th score) are asserted on these fp64 scores alone, without a GPU."""
import functools

import numpy as np

from tests.test_gpu_table_topk import EPS, cosine64

BAR = {"bf16x3": 1e-4, "f32": 1e-5}                       # the project's score bars (DESIGN.md sections 15, 22, 23), once per term


def tol_of(weights, precision: str) -> float:
    return float(sum(abs(w) for w in weights)) * BAR[precision]


def sum64(xs, tables, weights) -> np.ndarray:
    """[B, E] fp64: sum_s w_s cos(x_s[b], rows_s[e]), each norm clamped at eps; a term of weight 0 is not read"""
    total = None
    for x, rows, w in zip(xs, tables, weights):
        if w == 0:
            continue
        term = float(w) * cosine64(x, rows)
        total = term if total is None else total + term
    return total


def chain32(cosines, weights) -> np.ndarray:
    """the fp32 chain of the returned scores over the LIVE terms in order: acc = w_0 c_0; acc = acc + w_s c_s, every multiply and
    add rounded to fp32 on its own (numpy float32 arithmetic does exactly that)"""
    acc = None
    for c, w in zip(cosines, weights):
        if w == 0:
            continue
        term = np.float32(w) * c.astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


def combine64(blocks, invs, scales, weights) -> np.ndarray:
    """the combine kernel's formula in fp64: out[c, b] = sum_s block_s[c, b] inv_s[c] scale_s[b] w_s (blocks entity-major [cols, ld])"""
    out = np.zeros(blocks[0].shape, dtype=np.float64)
    for blk, inv, sc, w in zip(blocks, invs, scales, weights):
        out += blk.astype(np.float64) * inv.astype(np.float64)[:, None] * sc.astype(np.float64)[None, :] * float(w)
    return out


def combine32(blocks, invs, scales, weights) -> np.ndarray:
    """the same sum with the kernel's own roundings: ((block inv) (scale w)), summed in term order, all in fp32"""
    acc = None
    for blk, inv, sc, w in zip(blocks, invs, scales, weights):
        term = (blk * inv[:, None]).astype(np.float32) * (sc * np.float32(w)).astype(np.float32)[None, :]
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


def near_threshold(ref: np.ndarray, k: int, tol: float) -> int:
    """the largest number, over the mentions, of OTHER rows whose fp64 score lies within tol of the k-th largest"""
    worst = 0
    for row in ref:
        t = np.sort(row)[::-1][k - 1]
        worst = max(worst, int((np.abs(row - t) <= tol).sum()) - 1)
    return worst


# name -> (E, B, widths, weights, k, chunks, cap on the rows within tol of the k-th, seed).  The first five are the issue's table;
# "four" and "b1" add four live terms and B = 1 (Bp = 4).  N(0, 1) rows; the seeds were picked on the CPU, inside the caps at
# the wider (bf16x3) tolerance - test_table_topk_sum_host.py asserts it.
CASES = {
    "e300": (300, 3, (16, 8, 8), (1.0, 1.0, 1.0), 20, (64,), 2, 0),
    "e1500": (1500, 4, (32, 16, 16), (1.0, 0.5, 2.0), 64, (256,), 2, 0),
    "e700": (700, 9, (16, 260), (1.0, 1.0), 65, (0,), 2, 0),
    "e7": (7, 5, (4, 4), (1.0, -1.0), 7, (0,), 2, 0),
    "e2000": (2000, 5, (768, 512, 512), (1.0, 1.0, 1.0), 100, (0, 512), 6, 0),
    "four": (400, 3, (16, 8, 8, 12), (1.0, 0.5, -0.25, 2.0), 20, (128,), 2, 0),
    "b1": (500, 1, (8, 8), (1.0, 1.0), 10, (0,), 2, 0),
}


def draw(name: str, seed: int):
    E, B, widths, weights, k, chunks, cap, _ = CASES[name]
    g = np.random.default_rng(seed)
    xs = [g.standard_normal((B, d)).astype(np.float32) for d in widths]
    tables = [g.standard_normal((E, d)).astype(np.float32) for d in widths]
    return xs, tables


@functools.lru_cache(maxsize=None)
def sum_case(name: str):
    """dict(xs, tables, weights, k, chunks, cap, ref [B, E] fp64) of a case, computed once"""
    E, B, widths, weights, k, chunks, cap, seed = CASES[name]
    xs, tables = draw(name, seed)
    return dict(xs=xs, tables=tables, weights=weights, k=k, chunks=chunks, cap=cap, ref=sum64(xs, tables, weights), E=E, B=B,
                widths=widths)


__all__ = ["BAR", "CASES", "EPS", "chain32", "combine32", "combine64", "draw", "near_threshold", "sum64", "sum_case", "tol_of"]
