"""GHMFC in table form: the candidates of a mention are int64 rows of a device-resident
`drin_amd.model.EntityTable` instead of gathered features - what `baselines/data.py`'s `qid2idx` gather delivers per mention
(19.9 MB at the reference widths) never leaves the device.  `TableForm` is mixed into the three GHMFC models
(`ghmfc.Model`, `ghmfc_train.TrainableModel`, `ghmfc_variants.VariantModel`):

* `GhmfcIndexedBatch(mention, table, candidates)`, or - after `model.attach_entity_table(table)` - the reference's 8-item
  batch whose item 5 is the integer tensor `[B, N]` of rows (what `ghmfc_data.IndexedGhmfcData` yields);
* `eval()`: `drin_ghmfc_forward_table` (the variants: the indexed row kernels behind their own mention encoder) - the bits of
  the model on the gathered batch; `enable_entity_cache()` scores against per-entity rows `final_layer(pool(text[e]))`
  instead, rebuilt whenever the entity weights, the precision or the table change;
* `train()`: every entity's tokens are pooled once per table version, a step gathers `[B, N, D]` pooled rows
  (`drin_gather_rows`) and runs the gathered step's `entity_scores` on them - the same bits, scores and gradients.

`model.link(batch, k)` ranks every mention against the WHOLE table instead of a candidate list: the k best
rows by cosine (`drin_table_topk` on the per-entity rows), scores with the bits of the cached table-form scoring.

A row outside the table is clamped by the kernels and reported: `check_indices()` / `validate_indices` raise `IndexError`.
GPU only, fp32 tables; the table is an input and gets no gradient.  The link primitives (`row_inv_norms`, `cosine_rows_indexed`,
`table_topk`, `table_topk_sum`, `LinkResult`) and the index watch live in `drin_amd.table_ops`, which imports no model; they are
re-exported here.  They also read `rows` STORED as bfloat16 in place - DRIN's `Model.link` uses that; GHMFC's
own token tables stay fp32.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import _ptr, _stream
from .attention import PRECISIONS
from .model import EntityTable
from .table_ops import (IndexWatch, LinkResult, _check_f32, _row_dtype, cosine_rows_indexed, decode_status,  # noqa: F401 (re-exported)
                        row_inv_norms, table_topk, table_topk_sum)


class GhmfcIndexedBatch:
    """A GHMFC batch in table form: the five mention-side items of the reference's offline batch (mention_feature,
    mention_mask, begin, end, mention_image), the device-resident `EntityTable` (text `[E, T, D]` + mask `[E, T]`, or pooled
    `[E, D]`; image, object and object_score are None) and `candidates [B, N]` int64 rows of it."""

    def __init__(self, mention: Sequence, table: EntityTable, candidates: torch.Tensor):
        if len(mention) != 5:
            raise ValueError("mention part must be the first 5 items of the offline batch (baselines/data.py: mention_feature, "
                             "mention_mask, begin, end, mention_image)")
        self.mention, self.table, self.candidates = list(mention), table, candidates

    def gathered(self) -> list:
        """The equivalent 8-item batch (entity rows materialised with torch indexing, as the loader's gather)."""
        t, idx = self.table, self.candidates
        return self.mention + [t.text[idx], t.mask[idx] if t.text.dim() == 3 else 0, 0]


def check_table(table: EntityTable, embed_dim: int, on_gpu: bool = True) -> None:
    """The refusals of the table form: GPU (`on_gpu`), fp32, `[E, T, D]` + mask `[E, T]` or pooled `[E, D]`."""
    if not isinstance(table, EntityTable):
        raise TypeError(f"ghmfc table form: {type(table).__name__} is not a drin_amd.model.EntityTable")
    text, mask = table.text, table.mask
    if on_gpu and (text.device.type != "cuda" or (text.dim() == 3 and mask is not None and mask.device != text.device)):
        raise RuntimeError("ghmfc table form runs on the GPU only (no CPU fallback): move the table with EntityTable.to(device)")
    if text.dtype != torch.float32:
        raise NotImplementedError(f"ghmfc table form: a {text.dtype} entity table is not implemented (only torch.float32; DESIGN.md "
                                  "section 23)")
    if text.dim() not in (2, 3) or text.shape[-1] != embed_dim or text.shape[0] < 1:
        raise ValueError(f"ghmfc table form: table text {tuple(text.shape)} is neither [E, T, {embed_dim}] nor [E, {embed_dim}]")
    if text.dim() == 3 and (mask is None or tuple(mask.shape) != tuple(text.shape[:2])):
        raise ValueError(f"ghmfc table form: table mask {None if mask is None else tuple(mask.shape)} does not match text "
                         f"{tuple(text.shape)}")


def raise_bad_index(words) -> None:
    """IndexError from the four status words the kernels leave (`report_bad_index`: flag, pair, value low / high)."""
    _flag, pair, value = decode_status(words)
    raise IndexError(f"GhmfcIndexedBatch.candidates: row {value} at pair {pair} (b * N + n) is outside the entity table (it was "
                     f"clamped: the scores of that call are of the WRONG entity there); the reference's fancy index, "
                     f"baselines/data.py's qid2idx gather, raises here too")


def _table_tensors(table: EntityTable):
    """(text, mask or None, tokens) contiguous, mask int64"""
    text = table.text.contiguous()
    if text.dim() == 2:
        return text, None, 0
    return text, table.mask.to(torch.int64).contiguous(), text.shape[1]


def gather_rows(rows: torch.Tensor, index: torch.Tensor, status: Optional[torch.Tensor]) -> torch.Tensor:
    """`rows[index]` for `rows [E, W]` fp32 and int64 `index [...]` by `drin_gather_rows`: `[..., W]`."""
    out = torch.empty(*index.shape, rows.shape[1], dtype=torch.float32, device=rows.device)
    _lib.check(_lib.load().drin_gather_rows(_ptr(rows), _ptr(index), rows.shape[0], _ptr(out), index.numel(), rows.shape[1],
                                            _ptr(status), _stream(rows.device)))
    return out


def pooled_candidates(table: EntityTable, index: torch.Tensor, status: Optional[torch.Tensor], pooling: str = "avg") -> torch.Tensor:
    """`[B, N, D]`: the token mean of every candidate's table row (`drin_entity_token_mean_indexed`; `pooling` "max": the maximum,
    `drin_entity_token_pool_indexed`), or the gathered rows of a pooled table - what `entity_token_pool` gives on the gathered
    block, bit for bit."""
    text, mask, tokens = _table_tensors(table)
    if tokens == 0:
        return gather_rows(text, index, status)
    lib = _lib.load()
    out = torch.empty(*index.shape, text.shape[2], dtype=torch.float32, device=text.device)
    if pooling == "avg":
        _lib.check(lib.drin_entity_token_mean_indexed(_ptr(text), _ptr(mask), _ptr(index), text.shape[0], _ptr(out), index.numel(),
                                                      tokens, text.shape[2], _ptr(status), _stream(text.device)))
    else:
        _lib.check(lib.drin_entity_token_pool_indexed(_ptr(text), _ptr(mask), _ptr(index), text.shape[0], _ptr(out), index.numel(),
                                                      tokens, text.shape[2], _lib.ENTITY_POOLINGS[pooling], _ptr(status), _stream(text.device)))
    return out


class _TableState:
    """What a model keeps for its table form (per process: not part of the state dict)."""

    def __init__(self):
        self.table: Optional[EntityTable] = None
        self.cache_on = False
        self.rows: Optional[torch.Tensor] = None      # per-entity rows [E, D] of the cache
        self.rows_key = None
        self.rows_builds = 0
        self.inv: Optional[torch.Tensor] = None       # 1 / norm of every row of `rows` [E], under rows_key (link)
        self.inv_key = None
        self.pooled: Optional[torch.Tensor] = None    # per-entity token means [E, D] of train()
        self.pooled_key = None
        self.watch = IndexWatch(raise_bad_index)      # the status words per device and their read-backs (table_ops.py)


class TableForm:
    """Mixin of the GHMFC models: the table form described in this module's docstring.  The model supplies `cfg`, `precision`
    and `entity_encoder` (its `final_layer` and `param_list()`)."""

    @property
    def validate_indices(self) -> bool:
        """check after every table-form call (one synchronisation each): what was assigned, else DRIN_VALIDATE=1"""
        v = self.__dict__.get("_validate_indices")
        return os.environ.get("DRIN_VALIDATE", "") not in ("", "0") if v is None else v

    @validate_indices.setter
    def validate_indices(self, on: bool) -> None:
        self.__dict__["_validate_indices"] = bool(on)

    @property
    def _tf(self) -> _TableState:
        st = self.__dict__.get("_table_state")
        if st is None:
            st = self.__dict__["_table_state"] = _TableState()
        return st

    def __getstate__(self):
        state = self.__dict__.copy()          # events, pinned words and caches are per-process bookkeeping: a copy starts without
        state.pop("_table_state", None)
        return state

    # ---- the public surface ---------------------------------------------------------------------------------------
    def attach_entity_table(self, table: Optional[EntityTable]):
        """Read 8-item batches whose item 5 is an integer tensor `[B, N]` as candidate rows of `table` (None detaches).  A table
        attached on another device than the model's (the reference's driver builds `Model()` on the host and moves it later)
        follows the model: the first call moves it once; a call with the model on the host is refused like any other."""
        if table is not None:
            check_table(table, self.cfg.embed_dim, on_gpu=False)
        st = self._tf
        st.table, st.rows, st.rows_key, st.pooled, st.pooled_key = table, None, None, None, None
        st.inv, st.inv_key = None, None
        return self

    @property
    def entity_table(self) -> Optional[EntityTable]:
        return self._tf.table

    def enable_entity_cache(self, on: bool = True):
        """Let `eval()` calls in table form score against per-entity rows `final_layer(pool(text[e]))`
        (`drin_ghmfc_entity_rows`: `E x D` floats), built by the first call and rebuilt by the first call after the entity
        weights (an optimizer step, `load_state_dict`, an in-place edit), the precision or the table changed.  Scores then
        agree with the uncached ones to the rounding of one product, not bit for bit."""
        st = self._tf
        st.cache_on = bool(on)
        if not on:
            st.rows, st.rows_key, st.inv, st.inv_key = None, None, None, None
        return self

    @property
    def entity_cache_builds(self) -> int:
        """how many times the per-entity rows were built"""
        return self._tf.rows_builds

    @torch.no_grad()
    def link(self, batch, k: int, table: Optional[EntityTable] = None) -> LinkResult:
        """Rank every mention of `batch` against the WHOLE `table` (default: the attached one): `(scores [B, k], rows [B, k])`,
        the k best table rows by the model's cosine, best first.  `batch`: the five mention-side items, a `GhmfcIndexedBatch`
        or any 8-item batch (items 5-7 are not read).  The mention representation is the mention half alone, the entity side
        the per-entity rows `final_layer(pool(text[e]))` (built as for `enable_entity_cache()`, whether or not it is enabled,
        and rebuilt when the entity weights, the precision or the table change), so `scores` are, bit for bit, what the cached
        table form scores on `rows`.  `eval()` only, no gradient, GPU only; 1 <= k <= min(256, E)."""
        if self.training:
            raise RuntimeError("ghmfc link: ranking against the table is eval() only (no gradient flows through a top-k): call .eval()")
        mention = batch.mention if isinstance(batch, GhmfcIndexedBatch) else list(batch)[:5]
        if len(mention) != 5:
            raise ValueError("ghmfc link: batch must hold the five mention-side items (mention_feature, mention_mask, begin, end, "
                             "mention_image), optionally followed by the three entity-side ones")
        attached = table is None
        table = self._tf.table if attached else table
        if table is None:
            raise ValueError("ghmfc link: no table given and none attached: call model.attach_entity_table(table)")
        check_table(table, self.cfg.embed_dim, on_gpu=False)
        k, E = int(k), table.text.shape[0]
        if k < 1 or k > _lib.TOPK_MAX_K:
            raise ValueError(f"ghmfc link: k = {k} is not in [1, {_lib.TOPK_MAX_K}]")
        if k > E:
            raise ValueError(f"ghmfc link: k = {k} exceeds the table's {E} entities")
        dev = self._device(table.text)
        if dev.type != "cuda":
            raise RuntimeError("ghmfc link runs on the GPU only (no CPU fallback): move the model and the batch with .cuda()")
        if table.text.device != dev:
            table = table.to(dev)
            if attached:
                self.attach_entity_table(table)
        check_table(table, self.cfg.embed_dim)
        x = self._mention_only(mention).contiguous()
        st, rows = self._tf, self._entity_rows(table)
        if st.inv is None or st.inv_key != st.rows_key:
            st.inv = None
            st.inv, st.inv_key = row_inv_norms(rows, self.cfg.cosine_eps), st.rows_key
        return table_topk(x, rows, st.inv, k, self.cfg.cosine_eps, self.precision)

    def check_indices(self, wait: bool = True) -> None:
        """Raise `IndexError` if any table-form call since the last check met a candidate row outside `[0, E - 1]`, naming the
        row and the pair.  `wait=True` synchronises with the device; `wait=False` only looks at read-backs that have landed.
        `model.validate_indices = True` (or `DRIN_VALIDATE=1`) checks after every call instead."""
        self._tf.watch.check(wait)

    # ---- what the models' forwards call ---------------------------------------------------------------------------
    def _table_form(self, batch) -> Optional[GhmfcIndexedBatch]:
        """`batch` as a `GhmfcIndexedBatch` when it is in table form, else None."""
        if isinstance(batch, GhmfcIndexedBatch):
            check_table(batch.table, self.cfg.embed_dim)
            tb = batch
        else:
            item = batch[5] if len(batch) > 5 else None
            if not (isinstance(item, torch.Tensor) and not item.is_floating_point() and not item.is_complex() and item.dim() == 2):
                return None
            if self._tf.table is None:
                raise ValueError("ghmfc: item 5 of the batch is an integer tensor [B, N] (candidate rows) but no entity table is attached: "
                                 "call model.attach_entity_table(table)")
            dev = self._device(batch[0])
            if dev.type != "cuda":
                raise RuntimeError("ghmfc table form runs on the GPU only (no CPU fallback): move the model and the batch with .cuda()")
            if self._tf.table.text.device != dev:
                self.attach_entity_table(self._tf.table.to(dev))
            check_table(self._tf.table, self.cfg.embed_dim)
            tb = GhmfcIndexedBatch(batch[:5], self._tf.table, item)
        cand, dev = tb.candidates, tb.table.text.device
        if cand.device.type != "cuda":
            raise RuntimeError("ghmfc table form runs on the GPU only (no CPU fallback): move the candidates with .cuda()")
        if cand.dim() != 2 or cand.shape[1] != self.cfg.num_candidates:
            raise ValueError(f"ghmfc table form: candidates {tuple(cand.shape)} are not [B, {self.cfg.num_candidates}]")
        if self._device(tb.table.text) != dev or cand.device != dev:
            raise RuntimeError(f"ghmfc table form: the model, the candidates and the table must be on one device (table: {dev})")
        if self._tf.watch.pending() and not torch.cuda.is_current_stream_capturing():
            self.check_indices(wait=False)
        return GhmfcIndexedBatch(tb.mention, tb.table, cand.detach().to(torch.int64).contiguous())

    def _device(self, *like) -> torch.device:
        """the model's device (`ghmfc.model_device`): a model without parameters is where `like` is"""
        from .ghmfc import model_device
        return model_device(self, *like)

    def _status_words(self, device) -> torch.Tensor:
        return self._tf.watch.words(device)

    def _watch_indices(self, device) -> None:
        """After a table-form call (`IndexWatch.after_call`): the eager check, or an asynchronous read-back of the status words."""
        self._tf.watch.after_call(device, self.validate_indices)

    def _entity_key(self, table: EntityTable):
        """what the per-entity rows depend on: the entity weights' versions (none for an Identity final layer), the pooling, the
        precision and the table"""
        weights = tuple(x for p in self.entity_encoder.param_list() for x in (p.data_ptr(), p._version))
        return (weights, self.cfg.entity_final_pooling, self.precision, table._table_key())

    @torch.no_grad()
    def _entity_rows(self, table: EntityTable) -> torch.Tensor:
        """The per-entity rows of the cache, (re)built when the entity weights' versions, the precision or the table's key moved."""
        st, key = self._tf, self._entity_key(table)
        if st.rows is None or st.rows_key != key:
            lib = _lib.load()
            text, mask, tokens = _table_tensors(table)
            E, D = text.shape[0], text.shape[-1]
            w, b = [p.detach().contiguous() for p in self.entity_encoder.param_list()] or (None, None)
            nbytes = lib.drin_ghmfc_entity_rows_workspace_bytes(E, tokens, D)
            if nbytes == 0 and tokens > 0:
                _lib.check(_lib.E_SHAPE)
            st.rows = None                                                     # release the stale one before allocating
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=text.device)
            rows = torch.empty(E, D, dtype=torch.float32, device=text.device)
            if self.cfg.entity_default:
                _lib.check(lib.drin_ghmfc_entity_rows(_ptr(text), _ptr(mask), E, tokens, D, _ptr(w), _ptr(b), PRECISIONS[self.precision],
                                                      _ptr(rows), _ptr(ws), nbytes, _stream(text.device)))
            else:                                                              # "max" and / or an Identity final layer (w, b None)
                _lib.check(lib.drin_ghmfc_entity_rows_ex(_ptr(text), _ptr(mask), E, tokens, D, _lib.ENTITY_POOLINGS[self.cfg.entity_final_pooling],
                                                         _ptr(w), _ptr(b), PRECISIONS[self.precision], _ptr(rows), _ptr(ws), nbytes,
                                                         _stream(text.device)))
            st.rows, st.rows_key = rows, key
            st.rows_builds += 1
        return st.rows

    @torch.no_grad()
    def _pooled_table(self, table: EntityTable) -> torch.Tensor:
        """`[E, D]`: every entity's token mean or maximum (`drin_entity_token_mean` / `drin_entity_token_pool`, the gathered step's
        kernel on the same rows), once per table version and pooling - pooling depends on no weight; a pooled table is its own."""
        text, mask, tokens = _table_tensors(table)
        if tokens == 0:
            return text
        pooling = self.cfg.entity_final_pooling
        st, key = self._tf, (table._table_key(), pooling)
        if st.pooled is None or st.pooled_key != key:
            lib = _lib.load()
            E, T, D = text.shape
            st.pooled = None
            pooled = torch.empty(E, D, dtype=torch.float32, device=text.device)
            step = 1 << 20
            for e0 in range(0, E, step):
                n = min(E, e0 + step) - e0
                args = _ptr(text[e0:e0 + n]), _ptr(mask[e0:e0 + n]), _ptr(pooled[e0:e0 + n]), n, T, D
                if pooling == "avg":
                    _lib.check(lib.drin_entity_token_mean(*args, _stream(text.device)))
                else:
                    _lib.check(lib.drin_entity_token_pool(*args, _lib.ENTITY_POOLINGS[pooling], _stream(text.device)))
            st.pooled, st.pooled_key = pooled, key
        return st.pooled

    def _train_candidates(self, tb: GhmfcIndexedBatch) -> torch.Tensor:
        """`[B, N, D]` pooled candidate rows of a training step (an input: no gradient)."""
        dev = tb.candidates.device
        ent = gather_rows(self._pooled_table(tb.table), tb.candidates, self._status_words(dev))
        self._watch_indices(dev)
        return ent

    def _eval_scores(self, tb: GhmfcIndexedBatch, mention: torch.Tensor) -> torch.Tensor:
        """Scores of an `eval()` call from the mention representation `[B, D]` (the variants; `ghmfc.Model` scores through
        `drin_ghmfc_forward_table`): against the cached per-entity rows, or `entity_scores` on the indexed token means."""
        from .ghmfc_train import entity_scores
        dev = tb.candidates.device
        status = self._status_words(dev)
        if self._tf.cache_on:
            scores = cosine_rows_indexed(mention, self._entity_rows(tb.table), tb.candidates, self.cfg.cosine_eps, status)
        else:
            pooled = pooled_candidates(tb.table, tb.candidates, status, self.cfg.entity_final_pooling)
            scores = entity_scores(mention, pooled, None, self.entity_encoder.final_layer, self.cfg, self.precision)
        self._watch_indices(dev)
        return scores
