"""The model-agnostic operations on a device-resident entity table: what DRIN's `Model.link` and GHMFC's
table form both stand on, in a module that imports neither of them.

* the link primitives `row_inv_norms`, `cosine_rows_indexed`, `table_topk`, `table_topk_sum` and `cross_modal_edges`.  Each has ONE
  body - checks, workspace query, allocation, the call, the result - for table rows stored as float32 or as bfloat16 read in place
  (DESIGN.md section 34); the storage decides only which spelling of the entry point is called (float32 rows keep the old one, whose
  name the library's error texts carry) and whether the row dtype is among its arguments;
* the image-image edge as a term of `table_topk_sum`: `object_rows`, `ratio_rows_indexed` and `RatioTerm`;
* `IndexWatch`: the status words into which the kernels report a candidate row outside the table, their asynchronous read-backs and
  the check that turns them into an `IndexError` - one instance per model, which supplies the message.

GPU only; no gradient flows through any of these."""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import _ptr, _stream
from .attention import PRECISIONS

MAX_CALL_MENTIONS = 32768          # mentions per library call (`Model.MAX_CALL_MENTIONS`): more run in slices


class LinkResult(NamedTuple):
    """`model.link`: `scores [B, k]` float32 and `rows [B, k]` int64 table rows, best first (the ordering contract of
    include/drin_hip.h: higher score first, the lower row between equal scores, NaN last)."""
    scores: torch.Tensor
    rows: torch.Tensor


def _row_dtype(who: str, rows: torch.Tensor) -> int:
    """`FEAT_F32` / `FEAT_BF16` of table rows that a link primitive reads IN PLACE: contiguous float32, or
    contiguous bfloat16 - widened exactly inside the kernels, never copied."""
    if not torch.is_tensor(rows) or rows.dtype not in (torch.float32, torch.bfloat16) or not rows.is_contiguous():
        raise ValueError(f"{who}: rows must be a contiguous float32 or bfloat16 tensor, read in place "
                         f"(got {getattr(rows, 'dtype', type(rows).__name__)})")
    return _lib.FEAT_BF16 if rows.dtype == torch.bfloat16 else _lib.FEAT_F32


def _check_f32(who: str, name: str, t: torch.Tensor) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")


def _entry(name: str, stored_bf16: bool):
    """The entry point `name` for float32 rows, its `_ex` twin - which takes the row dtype(s) as well - for bfloat16 ones."""
    return getattr(_lib.load(), name + "_ex" if stored_bf16 else name)


def _topk_buffers(nbytes: int, B: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(workspace, scores [B, k], rows [B, k]) of a top-k call; a size query that refused (0 bytes) raises the library's reason."""
    if nbytes == 0:
        _lib.check(_lib.E_SHAPE)
    return (torch.empty(nbytes, dtype=torch.uint8, device=device), torch.empty(B, k, dtype=torch.float32, device=device),
            torch.empty(B, k, dtype=torch.int64, device=device))


def row_inv_norms(rows: torch.Tensor, eps: float) -> torch.Tensor:
    """`[E]` float32 = 1 / max(|rows[e]|, eps) by `drin_row_inv_norms`; bfloat16 `rows` are read in place (`drin_row_inv_norms_ex`:
    the bits of the float32 call on `rows.float()`)."""
    dtype = _row_dtype("row_inv_norms", rows)
    stored = dtype == _lib.FEAT_BF16
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    _lib.check(_entry("drin_row_inv_norms", stored)(_ptr(rows), *((dtype,) if stored else ()), rows.shape[0], rows.shape[1], eps, _ptr(out),
                                                    _stream(rows.device)))
    return out


def cosine_rows_indexed(x: torch.Tensor, rows: torch.Tensor, index: torch.Tensor, eps: float,
                        status: Optional[torch.Tensor]) -> torch.Tensor:
    """`[B, N]` = cos(x[b], rows[index[b, n]]) by `drin_cosine_rows_indexed_fwd`; no gradient.  `rows`: float32, or bfloat16 read
    in place (`drin_cosine_rows_indexed_fwd_ex`: the bits of the float32 call on `rows.float()`); `x` float32."""
    who = "cosine_rows_indexed"
    dtype = _row_dtype(who, rows)
    stored = dtype == _lib.FEAT_BF16
    x = x.detach().contiguous()
    _check_f32(who, "x", x)
    B, N = index.shape
    out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    _lib.check(_entry("drin_cosine_rows_indexed_fwd", stored)(_ptr(x), _ptr(rows), *((dtype,) if stored else ()), _ptr(index), rows.shape[0],
                                                              _ptr(out), B, N, x.shape[1], eps, _ptr(status), _stream(x.device)))
    return out


def table_topk(x: torch.Tensor, rows: torch.Tensor, inv_norms: torch.Tensor, k: int, eps: float, precision: str,
               chunk_entities: int = 0) -> LinkResult:
    """The k best of `rows [E, D]` for every `x [B, D]` by cosine (`drin_table_topk`); `inv_norms`: `row_inv_norms(rows, eps)`.
    bfloat16 `rows` are read in place (`drin_table_topk_ex`): they link exactly as `rows.float()` would; `x`
    and `inv_norms` stay float32."""
    who = "table_topk"
    dtype = _row_dtype(who, rows)
    stored = dtype == _lib.FEAT_BF16
    _check_f32(who, "x", x)
    _check_f32(who, "inv_norms", inv_norms)
    (B, D), E, prec = x.shape, rows.shape[0], PRECISIONS[precision]
    nbytes = _entry("drin_table_topk_workspace_bytes", stored)(B, E, D, k, chunk_entities, *((dtype, prec) if stored else ()))
    ws, scores, best = _topk_buffers(nbytes, B, k, x.device)
    _lib.check(_entry("drin_table_topk", stored)(_ptr(x), _ptr(rows), *((dtype,) if stored else ()), _ptr(inv_norms), E, B, D, k, eps, prec,
                                                 chunk_entities, _ptr(ws), nbytes, _ptr(scores), _ptr(best), _stream(x.device)))
    return LinkResult(scores, best)


class RatioTerm(NamedTuple):
    """A term of `table_topk_sum` in the RATIO form: `weight * (x[b] . rows[e]) / (x_mass[b] * row_mass[e] +
    eps)`.  `x [B, R]`, `x_mass [B]`, `rows [E, R]`, `row_mass [E]`: contiguous float32 on the GPU - for DRIN's image-image edge the
    two results of `object_rows` per side, with `eps = cfg.miei_eps`."""
    x: Optional[torch.Tensor]
    x_mass: Optional[torch.Tensor]
    rows: Optional[torch.Tensor]
    row_mass: Optional[torch.Tensor]
    weight: float
    eps: float


def object_rows(objects: torch.Tensor, scores: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """`(rows [n, R], mass [n])` float32 by `drin_object_rows`: `rows[r] = sum_j scores[r, j] objects[r, j] / max(|objects[r, j]|,
    eps)`, `mass[r] = sum_j scores[r, j]` - one side of the image-image edge (`model.py:84-92`).  `objects
    [n, K, R]` and `scores [n, K]` share one storage, float32 or bfloat16 read in place (the bits of the float32 call on the widened
    values); `1 <= K <= 16`.  No gradient."""
    who = "object_rows"
    dtype = _row_dtype(who, objects)
    if not torch.is_tensor(scores) or scores.dtype != objects.dtype or not scores.is_contiguous() or scores.device != objects.device:
        raise ValueError(f"{who}: scores must be a contiguous {objects.dtype} tensor on the objects' device "
                         f"(got {getattr(scores, 'dtype', type(scores).__name__)})")
    if objects.dim() != 3 or tuple(scores.shape) != tuple(objects.shape[:2]):
        raise ValueError(f"{who}: objects {tuple(objects.shape)} / scores {tuple(scores.shape)} must be [n, K, R] and [n, K]")
    n, K, R = objects.shape
    rows = torch.empty(n, R, dtype=torch.float32, device=objects.device)
    mass = torch.empty(n, dtype=torch.float32, device=objects.device)
    if n > 0:
        _lib.check(_lib.load().drin_object_rows(_ptr(objects), _ptr(scores), dtype, n, K, R, eps, _ptr(rows), _ptr(mass),
                                                _stream(objects.device)))
    return rows, mass


def ratio_rows_indexed(x: torch.Tensor, x_mass: torch.Tensor, rows: torch.Tensor, row_mass: torch.Tensor, index: torch.Tensor, eps: float,
                       status: Optional[torch.Tensor]) -> torch.Tensor:
    """`[B, N]` = (x[b] . rows[index[b, n]]) / (x_mass[b] * row_mass[index[b, n]] + eps) by `drin_ratio_rows_indexed_fwd`: the
    re-score of a `RatioTerm`; all float32, no gradient.  A row outside the table is clamped and reported into `status`."""
    who = "ratio_rows_indexed"
    x = x.detach().contiguous()
    for name, t in (("x", x), ("x_mass", x_mass), ("rows", rows), ("row_mass", row_mass)):
        _check_f32(who, name, t)
    B, N = index.shape
    if (x.dim() != 2 or rows.dim() != 2 or x.shape[1] != rows.shape[1] or x.shape[0] != B or tuple(x_mass.shape) != (B,)
            or tuple(row_mass.shape) != (rows.shape[0],) or index.dtype != torch.int64 or not index.is_contiguous()):
        raise ValueError(f"{who}: x {tuple(x.shape)}, x_mass {tuple(x_mass.shape)}, rows {tuple(rows.shape)}, row_mass {tuple(row_mass.shape)} "
                         f"must be [B = {B}, R], [B], [E, R], [E] and index contiguous int64 [B, N]")
    out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().drin_ratio_rows_indexed_fwd(_ptr(x), _ptr(x_mass), _ptr(rows), _ptr(row_mass), _ptr(index), rows.shape[0], _ptr(out),
                                                       B, N, x.shape[1], eps, _ptr(status), _stream(x.device)))
    return out


def table_topk_sum(terms: Sequence, k: int, eps: float, precision: str, chunk_entities: int = 0) -> LinkResult:
    """The k best table rows for every mention by a SUM of cosines (`drin_table_topk_sum`):
    `score(b, e) = sum_s weight_s * cos(x_s[b], rows_s[e])`.  `terms`: 1 to 4 of `(x [B, D_s], rows [E, D_s], inv_norms [E],
    weight)` - contiguous float32 tensors on one GPU, `inv_norms = row_inv_norms(rows, eps)`; the terms share `B` and `E`, not
    their width.  `rows` alone may be contiguous bfloat16 instead, term by term, read in place (`drin_table_topk_sum_ex`,
    DESIGN.md section 34: such a term links exactly as `rows.float()` would).  A term of weight 0 is dropped before any launch and
    its three tensors may be `None`.  The returned scores are the fp32 chain `w_0 c_0 + w_1 c_1 + ...` over `cosine_rows_indexed`
    of each live term on the returned rows, bit for bit.

    A term may instead be a `RatioTerm(x, x_mass, rows, row_mass, weight, eps)` (all float32): it contributes
    `weight * (x[b] . rows[e]) / (x_mass[b] * row_mass[e] + eps)`, `c_s` of the chain is then `ratio_rows_indexed`'s, and the call goes
    through `drin_table_topk_sum_forms`.  A call with 4-tuples only takes exactly the route above."""
    lib = _lib.load()
    terms = list(terms)
    arr = (_lib.DrinTopkTermC * max(len(terms), 1))()
    dtypes = (C.c_int32 * max(len(terms), 1))()
    forms = (_lib.DrinTopkFormC * max(len(terms), 1))()
    live, ratios = None, False
    for s, term in enumerate(terms[:len(arr)]):
        if isinstance(term, RatioTerm):
            x, rows, inv, weight = term.x, term.rows, None, term.weight
            arr[s].weight = float(weight)
            if float(weight) == 0.0:
                continue
            for name, t in (("x", x), ("x_mass", term.x_mass), ("rows", rows), ("row_mass", term.row_mass)):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
                    raise ValueError(f"table_topk_sum: term {s}: {name} must be a contiguous float32 tensor on the GPU")
            if live is None:
                live = (x.shape[0], rows.shape[0], x.device)
            if (x.dim() != 2 or rows.dim() != 2 or x.shape[1] != rows.shape[1] or x.shape[0] != live[0] or rows.shape[0] != live[1]
                    or tuple(term.x_mass.shape) != (live[0],) or tuple(term.row_mass.shape) != (live[1],)
                    or any(t.device != live[2] for t in (x, rows, term.x_mass, term.row_mass))):
                raise ValueError(f"table_topk_sum: term {s}: x {tuple(x.shape)}, x_mass {tuple(term.x_mass.shape)}, rows {tuple(rows.shape)}, "
                                 f"row_mass {tuple(term.row_mass.shape)} must be [B = {live[0]}, R], [B], [E = {live[1]}, R], [E] on one device")
            arr[s].x, arr[s].rows, arr[s].width = x.data_ptr(), rows.data_ptr(), x.shape[1]
            forms[s].form, forms[s].x_mass, forms[s].row_mass, forms[s].eps = _lib.TOPK_RATIO, term.x_mass.data_ptr(), term.row_mass.data_ptr(), term.eps
            ratios = True
            continue
        x, rows, inv, weight = term
        arr[s].weight = float(weight)
        if float(weight) == 0.0:
            continue
        # the library trusts the extents it is given: what the kernels index is settled here
        for name, t in (("x", x), ("rows", rows), ("inv_norms", inv)):
            stored = (torch.float32, torch.bfloat16) if name == "rows" else (torch.float32,)   # rows alone may be stored as bf16
            if not torch.is_tensor(t) or t.dtype not in stored or not t.is_contiguous() or t.device.type != "cuda":
                raise ValueError(f"table_topk_sum: term {s}: {name} must be a contiguous float32 tensor on the GPU"
                                 + (" (rows: or bfloat16, read in place)" if name == "rows" else ""))
        dtypes[s] = _lib.FEAT_BF16 if rows.dtype == torch.bfloat16 else _lib.FEAT_F32
        if live is None:
            live = (x.shape[0], rows.shape[0], x.device)
        if (x.dim() != 2 or rows.dim() != 2 or x.shape[1] != rows.shape[1] or x.shape[0] != live[0] or rows.shape[0] != live[1]
                or tuple(inv.shape) != (live[1],) or any(t.device != live[2] for t in (x, rows, inv))):
            raise ValueError(f"table_topk_sum: term {s}: x {tuple(x.shape)}, rows {tuple(rows.shape)}, inv_norms {tuple(inv.shape)} must be "
                             f"[B = {live[0]}, D], [E = {live[1]}, D], [E] on one device")
        arr[s].x, arr[s].rows, arr[s].row_inv_norms, arr[s].width = x.data_ptr(), rows.data_ptr(), inv.data_ptr(), x.shape[1]
    if live is None:                                                       # no live term, or none at all: the library names the reason
        _lib.check(lib.drin_table_topk_sum(arr, len(terms), 1, 1, k, eps, PRECISIONS[precision], chunk_entities, None, 0, None, None, None))
        raise _lib.DrinError(_lib.E_SHAPE, "drin_table_topk_sum: no live term")
    (B, E, dev), prec = live, PRECISIONS[precision]
    if ratios:                                                             # a live RATIO term: the entry points that take the forms
        nbytes = lib.drin_table_topk_sum_forms_workspace_bytes(arr, dtypes, forms, len(terms), B, E, k, chunk_entities, prec)
        ws, scores, best = _topk_buffers(nbytes, B, k, dev)
        _lib.check(lib.drin_table_topk_sum_forms(arr, dtypes, forms, len(terms), E, B, k, eps, prec, chunk_entities, _ptr(ws), nbytes,
                                                 _ptr(scores), _ptr(best), _stream(dev)))
        return LinkResult(scores, best)
    stored = any(d == _lib.FEAT_BF16 for d in dtypes)
    head = (arr, dtypes) if stored else (arr,)
    nbytes = _entry("drin_table_topk_sum_workspace_bytes", stored)(*head, len(terms), B, E, k, chunk_entities, *((prec,) if stored else ()))
    ws, scores, best = _topk_buffers(nbytes, B, k, dev)
    _lib.check(_entry("drin_table_topk_sum", stored)(*head, len(terms), E, B, k, eps, prec, chunk_entities, _ptr(ws), nbytes, _ptr(scores),
                                                     _ptr(best), _stream(dev)))
    return LinkResult(scores, best)


def cross_modal_edges(clip_image: torch.Tensor, clip_text: torch.Tensor, table_clip_text: torch.Tensor, table_clip_image: torch.Tensor,
                      index: torch.Tensor, scale: float, eps: float, status: Optional[torch.Tensor],
                      step: int = MAX_CALL_MENTIONS) -> Tuple[torch.Tensor, torch.Tensor]:
    """`(miet, mtei)`, each `[B, N]` float32: `miet[b, n] = scale cos(clip_image[b], table_clip_text[index[b, n]])`, `mtei[b, n] =
    scale cos(clip_text[b], table_clip_image[index[b, n]])` by `drin_cross_modal_edges`.  `clip_image`, `clip_text`: `[B, C]`
    float32; the two tables `[E, C]` share one storage, float32 or bfloat16 read in place (`drin_cross_modal_edges_ex`: the bits of
    the float32 call on the widened rows); `index [B, N]` int64.  More than `step` mentions run in slices; an empty `index` gives
    empty matrices.  A row outside the tables is clamped and reported into `status` (int32[4], or None: clamped silently)."""
    who = "cross_modal_edges"
    dtype = _row_dtype(who, table_clip_text)
    if _row_dtype(who, table_clip_image) != dtype:
        raise ValueError(f"{who}: the two tables differ in dtype ({table_clip_text.dtype}, {table_clip_image.dtype})")
    stored = dtype == _lib.FEAT_BF16
    xi, xt, index = clip_image.detach().contiguous(), clip_text.detach().contiguous(), index.detach().contiguous()
    _check_f32(who, "clip_image", xi)
    _check_f32(who, "clip_text", xt)
    if index.dtype != torch.int64 or index.dim() != 2:
        raise ValueError(f"{who}: index must be int64 [B, N] (got {index.dtype} {tuple(index.shape)})")
    (B, N), (E, width), dev = index.shape, table_clip_text.shape, index.device
    miet = torch.empty(B, N, dtype=torch.float32, device=dev)
    mtei = torch.empty(B, N, dtype=torch.float32, device=dev)
    if N > 0:
        call = _entry("drin_cross_modal_edges", stored)
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            _lib.check(call(_ptr(xi[sl]), _ptr(xt[sl]), _ptr(table_clip_text), _ptr(table_clip_image), *((dtype,) if stored else ()),
                            _ptr(index[sl]), E, sl.stop - b0, N, width, scale, eps, _ptr(miet[sl]), _ptr(mtei[sl]), _ptr(status), _stream(dev)))
    return miet, mtei


# ---- candidate rows outside the table ------------------------------------------------------------------------------------------
def decode_status(words) -> Tuple[int, int, int]:
    """`(flag, pair, row)` of the four status words the kernels leave (`report_bad_index`: flag, pair, value low / high): the
    row is the signed 64-bit value of its two halves."""
    w = [int(x) for x in words]
    value = ((w[3] & 0xFFFFFFFF) << 32 | (w[2] & 0xFFFFFFFF))
    value -= (1 << 64) if value >= (1 << 63) else 0
    return w[0], w[1], value


class IndexWatch:
    """The index watch of one model: per device the four status words its table-form calls hand to the kernels (sticky: the first
    reporter's), the asynchronous read-backs of calls still in flight and the pool of landed (pinned host words, event) pairs they
    re-use.  `raise_bad(words)` raises the owner's `IndexError`.  Per-process bookkeeping, not state: a copy or a pickle starts
    empty."""

    def __init__(self, raise_bad: Callable):
        self.raise_bad = raise_bad
        self.status = {}                                      # device -> int32[4]
        self.in_flight, self.pool = [], []

    def __getstate__(self):
        return {"raise_bad": self.raise_bad}

    def __setstate__(self, state):
        self.__init__(state["raise_bad"])

    def words(self, device) -> torch.Tensor:
        t = self.status.get(device)
        if t is None:
            t = self.status[device] = torch.zeros(4, dtype=torch.int32, device=device)
        return t

    def pending(self) -> bool:
        """read-backs are in flight: the next call looks at those that have landed (`check(wait=False)`)"""
        return bool(self.in_flight)

    def clear(self) -> None:
        """forget the read-backs in flight (the status words stay)"""
        self.in_flight.clear()

    def after_call(self, device, eager: bool) -> None:
        """After a table-form call: raise at once when checking eagerly (`validate_indices`), else start an asynchronous read-back
        of the status words that the next call / `check(wait=False)` looks at once it has landed - no synchronisation is added."""
        if torch.cuda.is_current_stream_capturing():          # inside a graph capture: no read-back, no event (the status words are still
            return                                            # written by the replayed kernels: check() after a replay sees them)
        if eager:
            self.check()
            return
        host, ev = self.pool.pop() if self.pool else (torch.empty(4, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
        host.copy_(self.words(device), non_blocking=True)
        ev.record(torch.cuda.current_stream(device))
        self.in_flight.append((host, ev))

    def check(self, wait: bool = True) -> None:
        """`raise_bad` if a call since the last check reported a row.  `wait=True` synchronises with the device and zeroes the
        words that reported; `wait=False` looks only at read-backs that have landed, and zeroes every word when one reported."""
        bad = None
        if wait:
            self.in_flight.clear()
            for t in self.status.values():
                w = t.cpu()
                if int(w[0]) != 0:
                    bad = bad or w.tolist()
                    t.zero_()
        else:
            while self.in_flight and self.in_flight[0][1].query():
                host, ev = self.in_flight.pop(0)
                if int(host[0]) != 0 and bad is None:
                    bad = host.tolist()
                self.pool.append((host, ev))                  # pinned words and event are re-used by the next call
            if bad is not None:
                self.in_flight.clear()
                for t in self.status.values():
                    t.zero_()
        if bad is not None:
            self.raise_bad(bad)


def in_slices(count: int, step: int, call: Callable) -> torch.Tensor:
    """`call(slice)` over `[0, count)` in slices of `step`, the results concatenated along dim 0 (one slice: its result itself)."""
    parts = [call(slice(b0, min(count, b0 + step))) for b0 in range(0, count, step)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)
