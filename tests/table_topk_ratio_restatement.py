"""What the image-image edge as a term of the summed top-k computes, restated plainly on the host: the fp64
double loop of `model.py:84-92` per (mention, entity); the rows `q`, `u` and masses `S`, `T` it factors into; the combine with a
RATIO term in fp64 and with the kernel's own fp32 roundings; and the cases the host and the GPU tests share - drawn once per case,
left unchanged.  The chain of the returned scores is `chain32` of tests/table_topk_sum_restatement.py over one more entry: `c_s`
of a RATIO term is `drin_ratio_rows_indexed_fwd`'s.  A ratio term is a score-weighted mean of cosines, |ii| <= 1: the project's
per-term bar (`BAR`, `tol_of`) applies to it as to a cosine."""
import functools

import numpy as np

from tests.table_topk_sum_restatement import BAR, chain32, near_threshold, sum64, tol_of

COS_EPS, MIEI_EPS = 1e-8, 1e-9                             # drin_config.cosine_eps, drin_config.miei_eps


def ii_loop64(mobj, ms, eobj, es, cos_eps=COS_EPS, miei_eps=MIEI_EPS) -> np.ndarray:
    """[B, E] fp64, model.py:84-92 for every (mention b, entity e): sum_{i, j} cos(mobj[b, i], eobj[e, j]) ms[b, i] es[e, j] /
    (sum_{i, j} ms[b, i] es[e, j] + miei_eps), each norm of the cosine clamped at cos_eps on its own - the double loop, i then j"""
    mobj, ms, eobj, es = (np.asarray(a, dtype=np.float64) for a in (mobj, ms, eobj, es))
    B, Km, _ = mobj.shape
    E, Ke, _ = eobj.shape
    sim, wsum = np.zeros((B, E)), np.zeros((B, E))
    for i in range(Km):
        xn = np.maximum(np.linalg.norm(mobj[:, i], axis=1), cos_eps)                 # [B]
        for j in range(Ke):
            yn = np.maximum(np.linalg.norm(eobj[:, j], axis=1), cos_eps)             # [E]
            cos = (mobj[:, i] @ eobj[:, j].T) / (xn[:, None] * yn[None, :])
            w = ms[:, i][:, None] * es[:, j][None, :]
            sim += cos * w
            wsum += w
    return sim / (wsum + miei_eps)


def object_rows64(obj, score, eps=COS_EPS):
    """(rows [n, R], mass [n]) fp64: rows[r] = sum_j score[r, j] obj[r, j] / max(|obj[r, j]|, eps), mass[r] = sum_j score[r, j]"""
    obj, score = np.asarray(obj, dtype=np.float64), np.asarray(score, dtype=np.float64)
    norm = np.maximum(np.linalg.norm(obj, axis=2), eps)                              # [n, K]
    return ((score / norm)[:, :, None] * obj).sum(1), score.sum(1)


def mass32(score) -> np.ndarray:
    """the ascending fp32 sum of the scores, as the kernel adds them"""
    score = np.asarray(score, dtype=np.float32)
    m = np.zeros(score.shape[0], dtype=np.float32)
    for j in range(score.shape[1]):
        m = (m + score[:, j]).astype(np.float32)
    return m


def ratio64(q, S, u, T, eps=MIEI_EPS) -> np.ndarray:
    """[B, E] fp64: (q[b] . u[e]) / (S[b] T[e] + eps) - the factored form of ii_loop64"""
    q, S, u, T = (np.asarray(a, dtype=np.float64) for a in (q, S, u, T))
    return (q @ u.T) / (S[:, None] * T[None, :] + eps)


def ratio32(dot, x_mass, row_mass, eps) -> np.ndarray:
    """the RATIO step on fp32 dot products [B, N] with the kernels' roundings: d = x_mass[b] row_mass[b, n]; d = d + eps; dot / d -
    numpy float32 arithmetic rounds each operation on its own and divides correctly rounded (x_mass [B], row_mass [B, N] gathered)"""
    d = (x_mass.astype(np.float32)[:, None] * row_mass.astype(np.float32)).astype(np.float32)
    d = (d + np.float32(eps)).astype(np.float32)
    return (dot.astype(np.float32) / d).astype(np.float32)


def combine_forms64(blocks, invs, scales, weights, forms) -> np.ndarray:
    """the combine in fp64 (blocks entity-major [cols, ld]); forms[s]: None for a cosine - block inv[c] scale[b] w - or
    (x_mass [ld], row_mass [cols], eps) for a RATIO term - w block / (row_mass[c] x_mass[b] + eps)"""
    out = np.zeros(blocks[0].shape, dtype=np.float64)
    for blk, inv, sc, w, form in zip(blocks, invs, scales, weights, forms):
        if form is None:
            out += blk.astype(np.float64) * inv.astype(np.float64)[:, None] * sc.astype(np.float64)[None, :] * float(w)
        else:
            xm, rm, eps = form
            out += float(w) * blk.astype(np.float64) / (rm.astype(np.float64)[:, None] * xm.astype(np.float64)[None, :] + float(np.float32(eps)))
    return out


def combine_forms32(blocks, invs, scales, weights, forms) -> np.ndarray:
    """the same with the kernel's own roundings, all in fp32, summed in term order: a cosine term is ((block inv) (scale w)); a RATIO
    term is d = row_mass[c] x_mass[b]; d = d + eps; t = block / d; t = t w"""
    acc = None
    for blk, inv, sc, w, form in zip(blocks, invs, scales, weights, forms):
        if form is None:
            term = (blk * inv[:, None]).astype(np.float32) * (sc * np.float32(w)).astype(np.float32)[None, :]
        else:
            xm, rm, eps = form
            d = (rm.astype(np.float32)[:, None] * xm.astype(np.float32)[None, :]).astype(np.float32)
            d = (d + np.float32(eps)).astype(np.float32)
            term = ((blk / d).astype(np.float32) * np.float32(w)).astype(np.float32)
        term = term.astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


# name -> (E, B, cosine widths, R, Km, Ke, weights (tt, ti, it, ii), k, chunks, cap on the rows within tol of the k-th, seed): the
# issue's table.  Rows N(0, 1), scores 0.05 + 0.95 U[0, 1); planted: ms[0, 0] = 0, es[3, :] = 0 (mass 0: the term is exactly 0
# there), eobj[5, 0, :] = 0 (the norm clamp).  The seeds were picked on the CPU, inside the caps at the wider (bf16x3) tolerance -
# test_table_topk_ratio_host.py asserts it.
CASES = {
    "ii_e300": (300, 3, (16, 8, 8), 8, 3, 1, (1.0, 1.0, 1.0, 1.0), 20, (64,), 2, 0),
    "ii_only": (500, 1, (), 12, 3, 1, (0.0, 0.0, 0.0, 1.0), 10, (0,), 2, 0),
    "ii_e1500": (1500, 4, (32, 16, 16), 260, 4, 2, (1.0, 0.5, 2.0, -0.5), 64, (256,), 2, 0),
    "ii_e2000": (2000, 5, (768, 512, 512), 2048, 3, 1, (1.0, 1.0, 1.0, 1.0), 100, (0, 512), 6, 0),
}


def draw(name: str, seed: int):
    E, B, widths, R, Km, Ke, _w, _k, _chunks, _cap, _ = CASES[name]
    g = np.random.default_rng(seed)
    xs = [g.standard_normal((B, d)).astype(np.float32) for d in widths]
    tables = [g.standard_normal((E, d)).astype(np.float32) for d in widths]
    mobj = g.standard_normal((B, Km, R)).astype(np.float32)
    eobj = g.standard_normal((E, Ke, R)).astype(np.float32)
    ms = (0.05 + 0.95 * g.random((B, Km))).astype(np.float32)
    es = (0.05 + 0.95 * g.random((E, Ke))).astype(np.float32)
    ms[0, 0] = 0.0
    es[3, :] = 0.0
    eobj[5, 0, :] = 0.0
    return xs, tables, mobj, ms, eobj, es


def score64(xs, tables, mobj, ms, eobj, es, weights) -> np.ndarray:
    """[B, E] fp64: the three weighted cosines and w_ii x the DOUBLE LOOP (not the factored form)"""
    ref = float(weights[3]) * ii_loop64(mobj, ms, eobj, es)
    cosines = sum64(xs, tables, weights[:len(xs)]) if xs else None
    return ref if cosines is None else cosines + ref


@functools.lru_cache(maxsize=None)
def ratio_case(name: str):
    """dict of a case, computed once: the draws, q / S / u / T in fp64, ref [B, E] fp64 by the double loop"""
    E, B, widths, R, Km, Ke, weights, k, chunks, cap, seed = CASES[name]
    xs, tables, mobj, ms, eobj, es = draw(name, seed)
    q, S = object_rows64(mobj, ms)
    u, T = object_rows64(eobj, es)
    return dict(xs=xs, tables=tables, mobj=mobj, ms=ms, eobj=eobj, es=es, weights=weights, k=k, chunks=chunks, cap=cap, E=E, B=B, R=R,
                widths=widths, q=q, S=S, u=u, T=T, ii=ii_loop64(mobj, ms, eobj, es), ref=score64(xs, tables, mobj, ms, eobj, es, weights))


__all__ = ["BAR", "CASES", "COS_EPS", "MIEI_EPS", "chain32", "combine_forms32", "combine_forms64", "draw", "ii_loop64", "mass32",
           "near_threshold", "object_rows64", "ratio32", "ratio64", "ratio_case", "score64", "tol_of"]
