"""What DRIN behind a first stage computes, restated plainly on the host: the two CLIP edges as fp64
cosines, the ordering contract of include/drin_hip.h with the slot rule of `drin_rank_rows`, and the fp64 oracle
(`oracle.drin_oracle.forward`) on the gathered batch.  Also the small CPU cases the host and the GPU tests share - the margins
the link test relies on are asserted on the oracle's scores alone, without a GPU."""
import functools

import numpy as np
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig
from drin_amd.model import EntityTable
from oracle import drin_oracle as O
from oracle.cases import TINY

TOL = {"bf16x3": 1e-4, "f32": 1e-5}                       # the project's score bars (DESIGN.md sections 15, 22)


# ---- the CLIP edges ---------------------------------------------------------------------------------------------------
def cos64(x: torch.Tensor, rows: torch.Tensor, index: torch.Tensor, scale: float, eps: float) -> torch.Tensor:
    """`scale * cos(x[b], rows[clamp(index[b, n])])` in fp64, each norm clamped at eps (nn.CosineSimilarity, torch >= 2)."""
    x, y = x.double(), rows.double()[index.clamp(0, rows.shape[0] - 1)]
    xn = x.norm(dim=-1).clamp_min(eps)[:, None]
    yn = y.norm(dim=-1).clamp_min(eps)
    return scale * (x[:, None, :] * y).sum(-1) / (xn * yn)


# ---- the ordering contract with the slot rule ----------------------------------------------------------------------------
def rank_order(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The permutation that sorts one mention's (score, row) pairs: higher score first, NaN below -inf and all NaNs equal,
    -0.0 == +0.0, the lower row between equal scores, the lower slot between equal scores on equal rows."""
    nan = np.isnan(scores)
    slots = np.arange(scores.shape[0])
    keys = -np.where(nan, np.float32(0.0), scores).astype(np.float64)                     # (NaNs replaced before the widening cast)
    return np.lexsort((slots, rows, keys, nan))                                           # the LAST key is the primary one


def canonical(scores: np.ndarray) -> np.ndarray:
    """float32 scores as the library returns keys: +0.0 for -0.0, one quiet NaN (0x7FC00000); as uint32 bit patterns"""
    s = np.asarray(scores, dtype=np.float32).copy()
    s[s == 0] = 0.0
    bits = s.view(np.uint32).copy()
    bits[np.isnan(s)] = 0x7FC00000
    return bits


def expected_rank(scores: np.ndarray, rows: np.ndarray, k: int):
    """`(score bits [B, k], rows [B, k], slots [B, k])` of `drin_rank_rows` on `scores [B, n]` float32 / `rows [B, n]` int64"""
    order = np.stack([rank_order(scores[b], rows[b])[:k] for b in range(scores.shape[0])])
    take = lambda a: np.take_along_axis(a, order, 1)   # noqa: E731
    return canonical(take(scores)), take(rows), order.astype(np.int32)


# ---- the small model cases ---------------------------------------------------------------------------------------------
WM = DrinConfig(dataset_name="wikimel", num_candidates_data=12, max_entity_attr_token_len=6, **TINY)   # N = 13, token-level
WD = DrinConfig(**TINY)                                                                                  # N = 11, pooled text
# name -> (cfg, table rows E, seed): the smallest geometries tests/test_gpu_routing.py reaches each route with - folded over the
# index ("wm", "wd"), off the folded path so that the rows are gathered for the layers ("wm3"); the cache is a switch on the table
CASES = {"wm": (WM, 30, 5), "wm3": (WM.with_(num_gcn_layers=3), 30, 6), "wd": (WD, 30, 7)}
B_CASE, CLIP_WIDTH, K_LINK = 3, 64, 4


@functools.lru_cache(maxsize=None)
def link_case(name: str):
    """Everything of a case on the CPU, drawn once and left unchanged: cfg, state dict, the `EntityTable` (with CLIP rows), the
    seven mention tensors, candidates [B, N] without a repeated row inside a mention, the mentions' CLIP rows, and the fp64
    oracle's scores [B, N] on the gathered batch with fp64 similarities."""
    cfg, E, seed = CASES[name]
    tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1, object_topk_entity=1), 1, seed)
    token_level = tab[7].dim() == 4
    table = EntityTable(tab[7][0], tab[8][0] if token_level else None, tab[9][0], tab[10][0], tab[11][0])
    men = synth.make_batch(cfg, B_CASE, seed + 1)[:7]
    t_text, t_image, m_image, m_text = synth.make_clip_rows(E, B_CASE, CLIP_WIDTH, seed)
    table.set_clip(t_text, t_image)
    g = torch.Generator().manual_seed(seed)
    cand = torch.stack([torch.randperm(E, generator=g)[:cfg.num_candidates_model] for _ in range(B_CASE)])
    sd = synth.make_state_dict(cfg, 8)
    miet = cos64(m_image, t_text, cand, cfg.clip_logit_scale, cfg.cosine_eps)
    mtei = cos64(m_text, t_image, cand, cfg.clip_logit_scale, cfg.cosine_eps)
    ref = O.forward(sd, men + table.gather(cand) + [miet, mtei], dtype=torch.float64, **O.config_kwargs(cfg))
    return dict(cfg=cfg, sd=sd, table=table, mention=men, candidates=cand, clip_image=m_image, clip_text=m_text, miet=miet, mtei=mtei,
                ref=ref)


def near_threshold(ref: torch.Tensor, k: int, tol: float) -> int:
    """The largest number, over the mentions, of OTHER candidates whose oracle score lies within `tol` of the k-th largest."""
    worst = 0
    for row in ref:
        t = torch.sort(row, descending=True).values[k - 1]
        worst = max(worst, int(((row - t).abs() <= tol).sum()) - 1)
    return worst
