"""Drop-in `Model` for the reference's `drin/model.py:156-209`, running on hand-written HIP kernels.

Same constructor side effects (parameter creation order, hence same-seed initial weights,
`train.py:134-136`), same `state_dict` keys, same `forward(batch)` signature
(the 14-sequence of `drin/data.py:110-126` already on the device, `train.py:33`) and the same
`[B, N]` fp32 result.  The arithmetic itself happens in `libdrin_hip.so` behind the C ABI of
`include/drin_hip.h`; PyTorch only owns memory, the stream and the autograd graph edge.

There is no eager/PyTorch fallback: if the library is missing or the tensors are not on an
AMD GPU, `forward` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import nn

from . import _lib, row_ops
from .config import DrinConfig, default_config
from .table_ops import (MAX_CALL_MENTIONS, IndexWatch, LinkResult, RatioTerm, cross_modal_edges, decode_status, in_slices, object_rows,
                        row_inv_norms, table_topk, table_topk_sum)


# ---- parameter containers mirroring the reference's module tree (keys of SURVEY.md §8b) -------------
class _AvgLinear(nn.Module):  # baselines/ghmfc.py:63-69
    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.linear = nn.Linear(in_dim, out_dim)


class _MentionEncoder(nn.Module):  # baselines/ghmfc.py:152-175 (offline branch): the parameters of args.py:28's three encoders
    def __init__(self, cfg: DrinConfig):
        super().__init__()
        dim = cfg.bert_embed_dim
        if cfg.mention_final_layer_name == "linear":
            self.final_layer = _AvgLinear(dim, dim)
        elif cfg.mention_final_layer_name == "transformer":            # ghmfc.py:166-167; "none" owns nothing (ghmfc.py:174-175)
            from .drin_encoders import MultilayerTransformer
            self.intermediate_layer = MultilayerTransformer(cfg)


class _EntityEncoder(nn.Module):  # baselines/ghmfc.py:202-214 (linear / offline branch)
    def __init__(self, dim: int):
        super().__init__()
        self.final_layer = nn.Linear(dim, dim)


class VertexEncoder(nn.Module):  # drin/model.py:13-24
    def __init__(self, cfg: DrinConfig):
        super().__init__()
        self.mention_text_encoder = _MentionEncoder(cfg)
        self.entity_text_encoder = _EntityEncoder(cfg.bert_embed_dim)
        self.mention_image_linear = nn.Linear(cfg.resnet_embed_dim, cfg.gcn_embed_dim)
        self.entity_image_linear = nn.Linear(cfg.resnet_embed_dim, cfg.gcn_embed_dim)


class GCNLayer(nn.Module):  # drin/model.py:109-119 (scaler edges: w_m is Identity and owns nothing)
    def __init__(self, cfg: DrinConfig):
        super().__init__()
        d = cfg.gcn_embed_dim
        vector = cfg.gcn_edge_feature == "vector"
        self.w_h = nn.Linear(d, d)
        if vector:
            self.w_m = nn.Linear(d, d)                                      # model.py:112
        self.w_u, self.w_v = [nn.Linear(d, d // 2 if vector else d) for _ in range(2)]   # model.py:113-116
        self.layer_norm = nn.LayerNorm(d)


# precisions that are modes of the fused inference path only: whatever else they meet (training, the per-entity cache,
# geometries off the fused path, traced forwards) runs split-bf16
_FUSED_ONLY = (_lib.PREC_BF16X3_IF16,)
_PLANES = (_lib.PREC_BF16X3, _lib.PREC_BF16X3_ALL, _lib.PREC_BF16X3_IF16)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _param_list(model: "Model") -> List[torch.Tensor]:
    ve = model.vertex_encoder
    ps = [
        ve.mention_text_encoder.final_layer.linear.weight, ve.mention_text_encoder.final_layer.linear.bias,
        ve.entity_text_encoder.final_layer.weight, ve.entity_text_encoder.final_layer.bias,
        ve.mention_image_linear.weight, ve.mention_image_linear.bias,
        ve.entity_image_linear.weight, ve.entity_image_linear.bias,
    ]
    for layer in model.gcn_layers:
        ps += [layer.w_h.weight, layer.w_h.bias, layer.w_u.weight, layer.w_u.bias, layer.w_v.weight, layer.w_v.bias,
               layer.layer_norm.weight, layer.layer_norm.bias]
        if hasattr(layer, "w_m"):
            ps += [layer.w_m.weight, layer.w_m.bias]
    return ps


def _fill_params(struct, tensors: Sequence[Optional[torch.Tensor]], per_layer: int = 8) -> None:
    """`per_layer`: 8 tensors per GCN layer, 10 with vector edges (w_m, b_m appended)."""
    names = ("w_mention_text", "b_mention_text", "w_entity_text", "b_entity_text",
             "w_mention_image", "b_mention_image", "w_entity_image", "b_entity_image")
    for n, t in zip(names, tensors[:8]):
        setattr(struct, n, _ptr(t))
    lnames = ("w_h", "b_h", "w_u", "b_u", "w_v", "b_v", "ln_weight", "ln_bias", "w_m", "b_m")[:per_layer]
    for l in range((len(tensors) - 8) // per_layer):
        for j, n in enumerate(lnames):
            setattr(struct.layer[l], n, _ptr(tensors[8 + per_layer * l + j]))


@torch.no_grad()
def _pool_tokens(text: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Masked token mean of `ghmfc.py:245-249` for `text [..., T, D]` (fp32 or bf16, read in place) and
    `mask [..., T]` -> `[..., D]` fp32, by the library's pooling kernel (`drin_pool_fwd`)."""
    lib = _lib.load()
    lead, (T, D) = text.shape[:-2], text.shape[-2:]
    text = text.contiguous().view(-1, T, D)
    if text.dtype not in (torch.float32, torch.bfloat16):
        text = text.to(torch.float32)
    mask = mask.to(torch.int64).contiguous().view(-1, T)
    E = text.shape[0]
    pooled = torch.empty(E, D, dtype=torch.float32, device=text.device)
    c = _lib.DrinConfigC()
    _lib.check(lib.drin_default_config(C.byref(c)))
    c.num_candidates, c.embed_dim, c.entity_tokens = 1, D, T
    c.feature_dtype = _lib.FEAT_BF16 if text.dtype == torch.bfloat16 else _lib.FEAT_F32
    stream = torch.cuda.current_stream(text.device).cuda_stream
    step = 1 << 20
    for e0 in range(0, E, step):                                      # one launch per 2^20 rows
        e1 = min(E, e0 + step)
        c.batch = e1 - e0
        b = _lib.DrinBatchC()
        b.entity_text, b.entity_text_mask = text[e0:e1].data_ptr(), mask[e0:e1].data_ptr()
        _lib.check(lib.drin_pool_fwd(C.byref(c), C.byref(b), pooled[e0:e1].data_ptr(), None, None, stream))
    return pooled.view(*lead, D)


class EntityTable:
    """The WikiMEL entity tables of `drin/data.py:163-175`, resident on the device: text features
    `[E, T, D]` (+ mask `[E, T]`) or pooled `[E, D]`, image `[E, (1,) R]`, object `[E, Ke, (1,) R]`, object
    score `[E, Ke]`.  With it a batch carries candidate INDICES instead of 22 MB of gathered features."""

    def __init__(self, text, mask, image, object, object_score):
        self.text, self.mask, self.image, self.object, self.object_score = text, mask, image, object, object_score
        self.cache_enabled = False
        self.cache_format = "f32"
        self.cache_format_forced = False
        self.cache_format_used: Optional[str] = None          # row format of the cache that is built right now
        self._scale_scan = None
        self._fmt_key = None
        self._cache: Optional[torch.Tensor] = None
        self._cache_key = None
        self._pooled = None
        self._object_rows = None
        # stored CLIP embeddings [E, C] of the entities (set_clip): what the two CLIP edges of candidates chosen at run time are
        # formed from (IndexedBatch.from_clip); the per-entity cache does not depend on them - not part of _table_key
        self.clip_text: Optional[torch.Tensor] = None
        self.clip_image: Optional[torch.Tensor] = None

    def set_clip(self, clip_text: torch.Tensor, clip_image: torch.Tensor) -> "EntityTable":
        """The entities' projected CLIP embeddings (`CLIPModel`'s `text_embeds` / `image_embeds`, preprocess/clip.py:158-172):
        `[E, C]` float32 each, `C % 4 == 0`, moved to the table's device.  `IndexedBatch.from_clip` and `Model.link` read them.
        Both may be bfloat16 instead (`C % 8 == 0`): stored rows that the link kernels read in place and
        widen exactly - they link as their float32 copies would, and no float32 copy is ever made."""
        E = self.num_entities
        for name, t in (("clip_text", clip_text), ("clip_image", clip_image)):
            if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"EntityTable.set_clip: {name} must be a float32 (or bfloat16) tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)})")
            if t.dim() != 2 or t.shape[0] != E:
                raise ValueError(f"EntityTable.set_clip: {name} has shape {tuple(t.shape)}, expected [{E}, C]")
            if t.shape[1] == 0 or t.shape[1] % 4 != 0:
                raise ValueError(f"EntityTable.set_clip: {name} has width {t.shape[1]}: C must be a positive multiple of 4")
        if clip_text.shape[1] != clip_image.shape[1]:
            raise ValueError(f"EntityTable.set_clip: clip_text and clip_image differ in width ({clip_text.shape[1]}, {clip_image.shape[1]})")
        if clip_text.dtype != clip_image.dtype:
            raise ValueError(f"EntityTable.set_clip: clip_text and clip_image differ in dtype ({clip_text.dtype}, {clip_image.dtype}): "
                             "both float32 or both bfloat16")
        if clip_text.dtype == torch.bfloat16 and clip_text.shape[1] % 8 != 0:
            raise ValueError(f"EntityTable.set_clip: bfloat16 rows of width {clip_text.shape[1]}: C must be a multiple of 8 (16-byte rows)")
        dev = self.text.device
        self.clip_text, self.clip_image = clip_text.detach().to(dev).contiguous(), clip_image.detach().to(dev).contiguous()
        return self

    # a row whose largest |x| exceeds this many times the median row's can dominate a mention's mean_n(ii ei): the mixed-f16
    # format is then not used for the table (see enable_cache)
    MIXED_F16_MAX_ROW_RATIO = 8.0

    def enable_cache(self, on: bool = True, format: str = "f32", force: bool = False) -> "EntityTable":
        """Let inference calls score from a per-entity precompute cache (`drin_build_entity_cache`):
        23.5 KB per entity at D=768 / R=2048, rebuilt by the first inference call after any weight change.
        `format="mixed_f16"` (`DRIN_CACHE_MIXED_F16`): the operands of per-pair scalars - the two edge-update rows and the object
        row - are stored as fp16 under a power-of-two scale per row and field, the vertex contractions and the CLS row stay
        fp32: 16.4 KB per entity, scores within ~2e-7 of the fp32 rows' (`oracle/precision_emulation.py`).
        The format holds a per-pair scalar (edge logit, image-image edge) to ~1e-5 and relies on the mention aggregates
        `mean_n(edge x vertex)` (`model.py:143-144`) averaging that over the candidates.  ONE candidate whose image row is orders of
        magnitude larger than the others' dominates the mean instead (measured: 1e-5 .. 7e-5 on the scores with rows x 1e6 - inside
        the 1e-4 bar, outside the 1e-5 guard).  So the format is used only for tables it is safe for BY CONSTRUCTION: the cache
        build scans the image table once per table version, and when any row's largest |x| exceeds `MIXED_F16_MAX_ROW_RATIO` (8) x
        the median row's - a share of at most 8 / (8 + N - 1) of a mention's aggregate: <= 6e-6 at N = 101 - the table gets
        fp32 rows, with a `UserWarning` saying so (`cache_format_used` tells which format a built cache has).
        `force=True` keeps the fp16 fields whatever the scan finds (the emulation tests that pin the format's limit use it)."""
        if format not in _lib.CACHE_FORMATS:
            raise ValueError(f"cache format {format!r}: one of {sorted(_lib.CACHE_FORMATS)}")
        self.cache_enabled = on
        if not on or format != self.cache_format or force != self.cache_format_forced:
            self._cache, self._cache_key = None, None
        self.cache_format, self.cache_format_forced = format, force
        return self

    def _rows_far_off_scale(self):
        """`(far, rows)`: how many image rows have a largest |x| above MIXED_F16_MAX_ROW_RATIO x the median row's.  One pass over
        the image table per table VERSION (no copy of it: max(amax, -amin); one host read-back), not per cache build."""
        img = self.image
        key = (img.data_ptr(), img._version, tuple(img.shape))
        if self._scale_scan is None or self._scale_scan[0] != key:
            flat = img.reshape(img.shape[0], -1)
            m = torch.maximum(flat.amax(1), -flat.amin(1)).float()
            finite = m[torch.isfinite(m) & (m > 0)]
            far = int((finite > self.MIXED_F16_MAX_ROW_RATIO * finite.median()).sum()) if finite.numel() else 0
            self._scale_scan = (key, far, int(m.numel()))
        return self._scale_scan[1], self._scale_scan[2]

    def _effective_cache_format(self) -> str:
        if self.cache_format != "mixed_f16":
            return self.cache_format
        far, rows = self._rows_far_off_scale()
        if far == 0:
            return "mixed_f16"
        import warnings
        if self.cache_format_forced:
            warnings.warn(f"EntityTable cache format mixed_f16 (forced): {far} of {rows} entity image rows are more than "
                          f"{self.MIXED_F16_MAX_ROW_RATIO:g} x the median row's magnitude; mentions that list such an entity may score up to "
                          f"~1e-4 from the fp32 rows", UserWarning, stacklevel=4)
            return "mixed_f16"
        warnings.warn(f"EntityTable cache format mixed_f16: {far} of {rows} entity image rows are more than {self.MIXED_F16_MAX_ROW_RATIO:g} x "
                      f"the median row's magnitude - such a row can dominate a mention's aggregate and carry its one fp16 edge's rounding "
                      f"(up to ~1e-4) into the scores; this table gets fp32 cache rows instead (format='f32')", UserWarning, stacklevel=4)
        return "f32"

    def invalidate(self) -> "EntityTable":
        """Drop the per-entity cache, the pooled-text copy and the rows of `object_rows`.  Needed only after the tables were edited
        through a path PyTorch's version counters do not see (`t.data.copy_(...)`, an external kernel writing the storage): in-place torch
        ops on the tensors and replaced tensors are detected by themselves."""
        self._cache, self._cache_key, self._pooled, self._scale_scan, self._object_rows = None, None, None, None, None
        return self

    def _table_key(self):
        return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (self.text, self.mask, self.image, self.object, self.object_score)
                     if t is not None)

    def _get_cache(self, call: "_Call", key, pc, prepared: torch.Tensor) -> torch.Tensor:
        fmt = self.cache_format_used if (self._cache is not None and self._fmt_key == (self.cache_format, self.cache_format_forced, self._table_key())) \
            else self._effective_cache_format()
        self._fmt_key = (self.cache_format, self.cache_format_forced, self._table_key())
        self.cache_format_used = fmt
        call.cfg.cache_format = _lib.CACHE_FORMATS[fmt]
        key = (key, call.cfg.precision, call.cfg.num_entities, call.cfg.cache_format, self._table_key())
        if key != self._cache_key or self._cache is None:
            lib = _lib.load()
            n = lib.drin_entity_cache_bytes(C.byref(call.cfg))
            if n == 0:
                raise _lib.DrinError(_lib.E_UNSUPPORTED, lib.drin_last_error().decode())
            self._cache = None                                        # release the stale one before allocating
            cache = torch.empty(n, dtype=torch.uint8, device=call.device)
            ws = call.byte_buffer(lib.drin_entity_cache_build_workspace_bytes(C.byref(call.cfg)))
            _lib.check(lib.drin_build_entity_cache(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), prepared.data_ptr(),
                                                   cache.data_ptr(), n, ws.data_ptr(), ws.numel(), call.stream()))
            self._cache, self._cache_key = cache, key
        return self._cache

    @property
    def num_entities(self) -> int:
        return self.text.shape[0]

    @torch.no_grad()
    def pooled_text(self, cfg: DrinConfig):
        """`(pooled [E, D], cls [E, D])` of a token-level table: the masked token mean of `ghmfc.py:245-249` and the
        token-0 row of `model.py:73-75`, per ENTITY.  Neither depends on the weights, so training in table form pools
        every entity once (library kernel, same arithmetic as the per-pair pooling of a gathered batch: identical
        values) instead of gathering and pooling 197 KB of tokens per candidate per step."""
        if self.text.dim() != 3:
            raise ValueError("pooled_text: the table already holds pooled text [E, D]")
        key = (self.text.data_ptr(), self.text._version, self.mask.data_ptr(), self.mask._version)
        if self._pooled is None or self._pooled[0] != key:
            text = self.text.contiguous()
            self._pooled = (key, _pool_tokens(text, self.mask), text[:, 0, :].contiguous())   # [E, D] each
        return self._pooled[1], self._pooled[2]

    @torch.no_grad()
    def object_rows(self, cfg: DrinConfig):
        """`(u [E, R], T [E])` float32: the entity side of the image-image edge (`model.py:84-92`) per ENTITY,
        `u[e] = sum_j es[e, j] eobj[e, j] / max(|eobj[e, j]|, cfg.cosine_eps)` and `T[e] = sum_j es[e, j]` by `drin_object_rows`.
        Neither depends on the weights: built once per version of `object` / `object_score` (the rule of `pooled_text`;
        `invalidate()` drops them).  The two tables share one storage, float32 or bfloat16 read in place; `u` is float32 either way."""
        obj, score = self.object, self.object_score
        if obj is None or score is None:
            raise ValueError("EntityTable.object_rows: the table has no object rows (`object` / `object_score` is None)")
        if obj.dim() == 4 and obj.shape[2] == 1:
            obj = obj[:, :, 0, :]                                         # the mean over one region row is that row
        if obj.dim() != 3 or tuple(score.shape) != tuple(obj.shape[:2]):
            raise NotImplementedError(f"EntityTable.object_rows: object {tuple(self.object.shape)} / object_score {tuple(score.shape)} must be "
                                      "[E, Ke, (1,) R] and [E, Ke] (a region mean over more than one row is not built)")
        key = (self.object.data_ptr(), self.object._version, tuple(self.object.shape), score.data_ptr(), score._version, cfg.cosine_eps)
        if self._object_rows is None or self._object_rows[0] != key:
            self._object_rows = None                                      # release the stale rows before allocating
            u, mass = object_rows(obj.detach().contiguous(), score.detach().contiguous(), cfg.cosine_eps)
            self._object_rows = (key, u, mass)
        return self._object_rows[1], self._object_rows[2]

    def to(self, device) -> "EntityTable":
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        moved = EntityTable(mv(self.text), mv(self.mask), mv(self.image), mv(self.object), mv(self.object_score))
        moved.cache_enabled, moved.cache_format, moved.cache_format_forced = self.cache_enabled, self.cache_format, self.cache_format_forced
        moved.clip_text, moved.clip_image = mv(self.clip_text), mv(self.clip_image)
        return moved

    def gather(self, index: torch.Tensor):
        """Per-pair tensors exactly as `MELData.__getitem__` + collate would deliver them (data.py:87-93)."""
        mask = self.mask[index] if self.mask is not None else torch.zeros(index.shape[0], dtype=torch.int64, device=index.device)
        return [self.text[index], mask, self.image[index], self.object[index], self.object_score[index]]


class IndexedBatch:
    """A batch in table form: the seven mention-side tensors of the 14-sequence, the device-resident
    `EntityTable`, `candidates [B, N]` int64 rows of it, the two CLIP similarity matrices `[B, N]`."""

    def __init__(self, mention: Sequence[torch.Tensor], table: EntityTable, candidates: torch.Tensor,
                 miet_similarity: torch.Tensor, mtei_similarity: torch.Tensor):
        if len(mention) != 7:
            raise ValueError("mention part must be the first 7 tensors of the 14-sequence (drin/data.py:110-117)")
        self.mention, self.table, self.candidates = list(mention), table, candidates
        self.miet_similarity, self.mtei_similarity = miet_similarity, mtei_similarity

    @classmethod
    @torch.no_grad()
    def from_clip(cls, mention: Sequence[torch.Tensor], table: EntityTable, candidates: torch.Tensor, clip_image: torch.Tensor,
                  clip_text: torch.Tensor, *, model: Optional["Model"] = None) -> "IndexedBatch":
        """An `IndexedBatch` whose two CLIP edges are formed HERE, for candidates chosen at run time (`Model.link`, a first stage's
        rows): `miet[b, n] = s cos(clip_image[b], table.clip_text[candidates[b, n]])`, `mtei[b, n] = s cos(clip_text[b],
        table.clip_image[candidates[b, n]])` by `drin_cross_modal_edges` - `CLIPModel`'s `logits_per_image` / `logits_per_text`
        (preprocess/clip.py:158-172) from stored embeddings, `s = cfg.clip_logit_scale`.  `clip_image`, `clip_text`: the mentions'
        projected CLIP embeddings `[B, C]` float32; `table` needs `set_clip` (its rows float32, or bfloat16 read in place by
        `drin_cross_modal_edges_ex`: the bits of the float32 call on the widened rows).  GPU only.  More than `Model.MAX_CALL_MENTIONS`
        mentions run in slices; `B = 0` gives empty matrices.  A candidate outside the table is clamped and reported: with `model`
        into its status words, watched as its forward watches them (`check_indices`, `validate_indices`) - `model` also supplies
        `cfg`; without a model the check is made here, at one synchronisation."""
        cfg = model.cfg if model is not None else default_config()
        if table.clip_text is None or table.clip_image is None:
            raise ValueError("IndexedBatch.from_clip: the table has no CLIP rows: call table.set_clip(clip_text, clip_image)")
        if candidates.dim() != 2:
            raise ValueError(f"IndexedBatch.from_clip: candidates has shape {tuple(candidates.shape)}, expected [B, N]")
        (B, N), width = candidates.shape, table.clip_text.shape[1]
        for name, t in (("clip_image", clip_image), ("clip_text", clip_text)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, width):
                raise ValueError(f"IndexedBatch.from_clip: {name} must be float32 [{B}, {width}] (got {getattr(t, 'dtype', None)} "
                                 f"{tuple(getattr(t, 'shape', ()))})")
        dev = candidates.device
        if dev.type != "cuda":
            raise RuntimeError("IndexedBatch.from_clip runs on an AMD GPU only (no CPU / eager fallback); move the batch to 'cuda'")
        if any(t.device != dev for t in (clip_image, clip_text, table.clip_text, table.clip_image)):
            raise RuntimeError("IndexedBatch.from_clip: the candidates, the mentions' CLIP rows and the table's must be on one device")
        launches = B > 0 and N > 0
        status = None
        if launches:
            status = model._status_words(dev) if model is not None else torch.zeros(4, dtype=torch.int32, device=dev)
        miet, mtei = cross_modal_edges(clip_image, clip_text, table.clip_text, table.clip_image, candidates.detach().to(torch.int64),
                                       cfg.clip_logit_scale, cfg.cosine_eps, status,
                                       (type(model) if model is not None else Model).MAX_CALL_MENTIONS)
        if launches:
            if model is not None:
                model._watch_indices(dev)
            elif not torch.cuda.is_current_stream_capturing():
                words = status.cpu()
                if int(words[0]) != 0:
                    Model._raise_bad_index(words.tolist())
        return cls(mention, table, candidates, miet, mtei)

    def gathered(self) -> List[torch.Tensor]:
        """The equivalent 14-sequence (entity rows materialised with torch indexing)."""
        return self.mention + self.table.gather(self.candidates) + [self.miet_similarity, self.mtei_similarity]

    def gathered_pooled(self, cfg: DrinConfig):
        """`(14-sequence with pooled entity text [B, N, D], cls rows [B, N, D])`: what a training step needs of a
        token-level table - 22 KB per candidate instead of 219 KB, and no per-step token pooling."""
        t, idx = self.table, self.candidates
        pooled, cls = t.pooled_text(cfg)
        dummy = torch.zeros(idx.shape[0], dtype=torch.int64, device=idx.device)
        seq = self.mention + [pooled[idx], dummy, t.image[idx], t.object[idx], t.object_score[idx],
                              self.miet_similarity, self.mtei_similarity]
        return seq, cls[idx]


def _split_mentions(batch, step: int):
    """Slices of at most `step` mentions of a 14-sequence or an `IndexedBatch` (views, nothing is copied)."""
    if isinstance(batch, IndexedBatch):
        B = batch.candidates.shape[0]
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            yield IndexedBatch([t[sl] for t in batch.mention], batch.table, batch.candidates[sl],
                               batch.miet_similarity[sl], batch.mtei_similarity[sl])
    else:
        B = batch[0].shape[0]
        for b0 in range(0, B, step):
            sl = slice(b0, min(B, b0 + step))
            yield [t[sl] if torch.is_tensor(t) and t.dim() > 0 and t.shape[0] == B else t for t in batch]


class _Call:
    """One forward's C structs; keeps the tensors they point into alive."""

    def __init__(self, cfg: DrinConfig, batch: Sequence[torch.Tensor], precision: int,
                 entity_index: Optional[torch.Tensor] = None, keep_bf16: bool = False,
                 entity_text_cls: Optional[torch.Tensor] = None, index_status: Optional[torch.Tensor] = None):
        """`keep_bf16`: the caller will take a path that reads bf16-stored features in place (fused inference);
        otherwise bf16 features are widened to fp32 here (exact) - e.g. for training.
        `entity_text_cls` `[B, N, D]`: the token-0 rows of the text-text edge when `entity_text_feature` holds token
        means pooled ahead of time (`EntityTable.pooled_text`)."""
        self._describe(cfg, batch, precision, entity_index, keep_bf16, entity_text_cls, index_status)
        self.convert(precision if keep_bf16 else None)

    @classmethod
    def described(cls, cfg: DrinConfig, batch: Sequence[torch.Tensor], precision: int, **kw) -> "_Call":
        """The shape / config half of the constructor alone: `cfg` is complete - it is what the library's `drin_*_supported`
        predicates read - and no tensor is converted or copied yet; `convert` completes the call."""
        return cls.__new__(cls)._describe(cfg, batch, precision, **kw)

    _PARTLY_BF16 = ("bf16 feature storage: give all six feature tensors (mention text / image / object, entity "
                    "text / image / object) as bfloat16, or none")

    def _describe(self, cfg, batch, precision, entity_index=None, keep_bf16=False, entity_text_cls=None, index_status=None):
        if len(batch) not in (14, 15):
            raise ValueError(f"batch must be the 14-sequence of drin/data.py:110-126 (got {len(batch)} items)")
        (mtf, _mask, start, end, mimg, mobj, mscore, etf, emask, eimg, eobj, escore, miet, mtei) = batch[:14]
        dev = mtf.device
        if dev.type != "cuda":
            raise RuntimeError("drin_amd.Model runs on an AMD GPU only (no CPU / eager fallback); move the batch to 'cuda'")
        # bf16 feature storage (BASELINE configs 2-3): all six feature tensors, or none
        feats = (mtf, mimg, mobj, etf, eimg, eobj)
        self._n_bf16 = sum(t.dtype == torch.bfloat16 for t in feats)
        if keep_bf16 and 0 < self._n_bf16 < len(feats):
            raise ValueError(self._PARTLY_BF16)
        for t in feats + (mscore, escore, miet, mtei):
            if t.device != dev:
                raise RuntimeError("all batch tensors must be on the same device")
        (B, L, D), N, R = mtf.shape, cfg.num_candidates_model, mimg.shape[-1]
        table = entity_index is not None
        if table:
            # entity tensors are tables [E, ...]: give them the per-pair ranks by viewing E as (E, 1)
            E = etf.shape[0]
            if tuple(entity_index.shape) != (B, N):
                raise ValueError(f"candidates has shape {tuple(entity_index.shape)}, expected {(B, N)}")
            etf, eimg, eobj, escore = (t.unsqueeze(1) for t in (etf, eimg, eobj, escore))
            if emask is not None and torch.is_tensor(emask) and emask.dim() >= 2:
                emask = emask.unsqueeze(1)
            lead = (E, 1)
        else:
            lead = (B, N)
        token_level = etf.dim() == 4                                  # model.py:73-75
        if D != cfg.bert_embed_dim or R != cfg.resnet_embed_dim:
            raise ValueError(f"feature dims ({D}, {R}) do not match the config ({cfg.bert_embed_dim}, {cfg.resnet_embed_dim})")
        if tuple(etf.shape[:2]) != lead:
            raise ValueError(f"entity_text_feature leads with {tuple(etf.shape[:2])}, expected {lead}")
        if mobj.dim() not in (3, 4) or eobj.dim() not in (4, 5) or eimg.dim() not in (3, 4):
            raise ValueError("unexpected rank for object / image features (model.py:43-44,78-83)")
        Km, Ke = mobj.shape[1], eobj.shape[2]
        for name, t, shape in (
            ("mention_image_feature", mimg, (B, mimg.shape[1], R)),
            ("mention_object_score", mscore, (B, Km)),
            ("entity_object_score", escore, lead + (Ke,)),
            ("miet_similarity", miet, (B, N)),
            ("mtei_similarity", mtei, (B, N)),
            ("mention_start_pos", start, (B,)),
            ("mention_end_pos", end, (B,)),
        ):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
        if tuple(eimg.shape[0:2]) != lead or tuple(eobj.shape[0:2]) != lead or eimg.shape[-1] != R or eobj.shape[-1] != R or mobj.shape[-1] != R:
            raise ValueError("entity/mention image or object feature shape mismatch")
        if token_level:
            if tuple(emask.shape) != tuple(etf.shape[:3]):
                raise ValueError(f"entity_text_mask has shape {tuple(emask.shape)}, expected {tuple(etf.shape[:3])}")
        else:
            emask = None
        if entity_text_cls is not None:
            if token_level:
                raise ValueError("entity_text_cls goes with pooled entity text")
            if entity_text_cls.device != dev:
                raise RuntimeError("all batch tensors must be on the same device")
            want = (etf.shape[0], D) if table else (B, N, D)       # a table of token-0 rows, or per-pair rows
            if tuple(entity_text_cls.shape) != want:
                raise ValueError(f"entity_text_cls has shape {tuple(entity_text_cls.shape)}, expected {want}")
        if index_status is not None and (index_status.dtype != torch.int32 or index_status.numel() < 4 or index_status.device != dev):
            raise ValueError("index_status: int32[4] on the batch's device")
        self.keep = [mtf, start, end, mimg, mobj, mscore, etf, emask, eimg, eobj, escore, miet, mtei, entity_index,
                     entity_text_cls, index_status if table else None]
        self.device, self.B, self.N, self.D = dev, B, N, D
        c = _lib.DrinConfigC()
        _lib.check(_lib.load().drin_default_config(C.byref(c)))
        c.batch, c.num_candidates, c.embed_dim, c.image_dim = B, N, D, R
        c.mention_tokens, c.image_regions = L, mimg.shape[1]
        c.mention_objects, c.entity_objects = Km, Ke
        c.entity_tokens = etf.shape[2] if token_level else 0
        c.mention_object_inner = mobj.shape[2] if mobj.dim() == 4 else 0
        c.entity_image_inner = eimg.shape[2] if eimg.dim() == 4 else 0
        c.entity_object_inner = eobj.shape[3] if eobj.dim() == 5 else 0
        c.num_layers = cfg.num_gcn_layers
        c.dynamic_edges = 1 if cfg.gcn_edge_type == "dynamic" else 0
        for k in range(4):
            c.edge_enabled[k] = float(cfg.gcn_edge_enabled[k])
        c.layer_norm_eps, c.cosine_eps, c.miei_eps, c.clip_scale = (
            cfg.layer_norm_eps, cfg.cosine_eps, cfg.miei_eps, cfg.clip_logit_scale)
        c.precision = precision
        c.num_entities = etf.shape[0] if table else 0
        c.vector_edges = 1 if cfg.gcn_edge_feature == "vector" else 0
        c.feature_dtype = _lib.FEAT_F32                       # (bf16 kept in place: `convert` says so)
        c.vertex_activation = _lib.ACTIVATIONS[cfg.gcn_vertex_activation]
        c.edge_activation = _lib.ACTIVATIONS[cfg.gcn_edge_activation]
        self.per_layer = 10 if c.vector_edges else 8
        self.cfg = c
        # what `Model._score` / `Model._route` add for the autograd edge (a bare call scores and trains without them)
        self.owner: Optional["Model"] = None                  # whose gradient bucket and layers-ready hook backward uses
        self.input_roles: Sequence[str] = ()                  # batch tensors that follow the parameters into `_DrinScore.apply`
        self.params_ready: Optional[torch.cuda.Event] = None  # train.OverlappedStep: an update still running on a side stream
        self.token_block: Optional[torch.Tensor] = None       # a bf16 [B, N, T, D] block pooled in place, and its int64 mask
        self.token_mask: Optional[torch.Tensor] = None
        return self

    def convert(self, in_place: Optional[int] = None) -> "_Call":
        """The conversion half: fp32 / int64, contiguous, and the `drin_batch` that points at the results.  `in_place`: what
        `keep_bf16` gives the constructor - that precision, and features stored as bf16 (all six, or none) stay as they are."""
        if in_place is not None:
            if 0 < self._n_bf16 < 6:
                raise ValueError(self._PARTLY_BF16)
            self.cfg.precision, self.cfg.feature_dtype = in_place, _lib.FEAT_BF16 if self._n_bf16 else _lib.FEAT_F32
        f32 = lambda t: t.to(torch.float32).contiguous()  # noqa: E731
        feat = (lambda t: t.contiguous()) if self.cfg.feature_dtype == _lib.FEAT_BF16 else f32  # noqa: E731
        i64 = lambda t: t.to(device=self.device, dtype=torch.int64).contiguous()  # noqa: E731
        kinds = (feat, i64, i64, feat, feat, f32, feat, i64, feat, feat, f32, f32, f32, i64, f32, lambda t: t)
        self.keep = [None if t is None else kind(t) for kind, t in zip(kinds, self.keep)]
        b = _lib.DrinBatchC()
        for name, t in zip(("mention_text", "mention_start", "mention_end", "mention_image", "mention_object",
                            "mention_object_score", "entity_text", "entity_text_mask", "entity_image",
                            "entity_object", "entity_object_score", "miet_similarity", "mtei_similarity",
                            "entity_index", "entity_text_cls", "index_status"), self.keep):
            setattr(b, name, _ptr(t))
        self.batch = b
        return self

    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def scores(self) -> torch.Tensor:
        """Uninitialised `[B, N]` fp32 for the library to fill; of an empty batch, already the result."""
        return torch.empty(self.B, self.N, dtype=torch.float32, device=self.device)

    def byte_buffer(self, n: int) -> torch.Tensor:
        return torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)

    def workspace(self, training: bool) -> torch.Tensor:
        n = _lib.load().drin_workspace_bytes(C.byref(self.cfg), 1 if training else 0)
        if n == 0 and self.B > 0:
            raise _lib.DrinError(_lib.E_SHAPE, _lib.load().drin_last_error().decode())
        return self.byte_buffer(n)

    def param_struct(self, params: Sequence[torch.Tensor]):
        """`(tensors, drin_params)`: the parameters detached and contiguous, and the struct that points at them."""
        tensors = tuple(p.detach().contiguous() for p in params)
        pc = _lib.DrinParamsC()
        _fill_params(pc, tensors, self.per_layer)
        return tensors, pc


class _Prepared:
    """Weight-only products of the fused inference path (drin_prepare), cached per weight version."""

    def __init__(self):
        self.key = None
        self.buf: Optional[torch.Tensor] = None
        self.generation = 0          # bumped by every rebuild: what caches derived from the folds are keyed on

    def invalidate(self) -> None:
        self.key = None

    def get(self, call: "_Call", params: Sequence[torch.Tensor], pc) -> torch.Tensor:
        key = (call.cfg.embed_dim, call.cfg.image_dim, call.cfg.dynamic_edges) + tuple((p.data_ptr(), p._version) for p in params)
        if key != self.key or self.buf is None or self.buf.device != call.device:
            lib = _lib.load()
            n = lib.drin_prepared_bytes(C.byref(call.cfg))
            self.buf = torch.empty(n, dtype=torch.uint8, device=call.device)
            _lib.check(lib.drin_prepare(C.byref(call.cfg), C.byref(pc), self.buf.data_ptr(), n, call.stream()))
            self.key = key
            self.generation += 1
        return self.buf


def _dead_param_indices(n_params: int, per_layer: int, dynamic: bool) -> List[int]:
    """Positions in `_param_list` order of the parameters the score does not depend on (`.grad is None` in the reference)."""
    nl = (n_params - 8) // per_layer
    dead_layers = range(nl - 1, nl) if dynamic else range(nl)
    return [8 + per_layer * l + j for l in dead_layers for j in (2, 3, 4, 5) + ((8, 9) if per_layer == 10 else ())]


def _bucket_layout(params: Sequence[torch.Tensor], per_layer: int, dynamic: bool):
    """`(offsets, live_floats, total_floats)`: where each parameter of `_param_list` order sits in a flat fp32 bucket - the
    parameters that receive a gradient first (the all-reduced / Adam-stepped prefix), the dead ones behind them; every
    slot starts on a 256-byte boundary."""
    dead = set(_dead_param_indices(len(params), per_layer, dynamic))
    offsets, off = [0] * len(params), 0
    for want_dead in (False, True):
        for i, p in enumerate(params):
            if (i in dead) == want_dead:
                offsets[i] = off
                off += (p.numel() + 63) & ~63
        if not want_dead:
            live = off
    return offsets, live, off


# the floating-point batch tensors autograd reaches through the reference's plain-torch Model.forward (drin/model.py:164-209):
# drin_input_grads field -> position in _Call.keep (the tensors after _Call's conversions)
_INPUT_FIELDS = {"mention_text": 0, "mention_image": 3, "mention_object": 4, "mention_object_score": 5, "entity_text": 6,
                 "entity_image": 8, "entity_object": 9, "entity_object_score": 10, "miet_similarity": 11, "mtei_similarity": 12,
                 "entity_text_cls": 14}
_BATCH_FLOAT = (0, 4, 5, 6, 7, 9, 10, 11, 12, 13)      # float tensors of the 14-sequence (the mask and positions are integer)


def _feature_inputs(call: _Call, block: Optional[torch.Tensor] = None):
    """`(roles, tensors)`: the batch tensors of `call` that require grad (after `_Call`'s conversions, so that torch's own
    ToCopyBackward hands a bf16 leaf a bf16 gradient), plus a bf16 token block pooled in place (`block`, role "token_block")."""
    roles, feats = [], []
    for role, i in _INPUT_FIELDS.items():
        t = call.keep[i]
        if t is not None and t.requires_grad:
            roles.append(role)
            feats.append(t)
    if block is not None and block.requires_grad:
        roles.append("token_block")
        feats.append(block)
    return tuple(roles), tuple(feats)


def _batch_requires_grad(batch) -> bool:
    if isinstance(batch, IndexedBatch):
        t = batch.table
        ts = list(batch.mention) + [t.text, t.image, t.object, t.object_score, batch.miet_similarity, batch.mtei_similarity]
    else:
        ts = [batch[i] for i in _BATCH_FLOAT if i < len(batch)]
    return any(torch.is_tensor(x) and x.is_floating_point() and x.requires_grad for x in ts)


def _param_grads(call: _Call, params: Sequence[torch.Tensor]):
    """`(drin_param_grads, gradients to return)`: zeroed destinations for every parameter - views of the owner's flat bucket,
    or fresh tensors - with the positions the score does not depend on returned as None."""
    owner = call.owner
    if owner is not None and owner.grad_bucket_enabled:
        # every gradient is a view of ONE flat fp32 bucket, zeroed with one memset: autograd's AccumulateGrad adopts the
        # views as .grad, so the data-parallel all-reduce and the one-launch Adam run on the bucket itself, copy-free
        grads = owner._bucket_grads(params)
    else:
        grads = [torch.empty_like(p) for p in params]
        torch._foreach_zero_(grads)                               # one multi-tensor launch instead of 24 fills
    gc = _lib.DrinParamGradsC()
    _fill_params(gc, grads, call.per_layer)
    out = list(grads)
    # parameters the score does not depend on get no gradient at all in the reference (.grad is None):
    # the last layer's edge update is dead (model.py:130-134), and static edges never use w_u / w_v (/ w_m)
    for i in _dead_param_indices(len(params), call.per_layer, bool(call.cfg.dynamic_edges)):
        out[i] = None
    return gc, out


class _Route(NamedTuple):
    """What `Model._route` decides for one library call."""
    path: str                                      # "prepared" (drin_forward_prepared), "cached" (drin_forward_cached), "layers" (drin_forward_staged)
    call: _Call
    training: bool                                 # keep what backward reads; tensors that require grad join the autograd edge
    token_block: Optional[torch.Tensor] = None     # a bf16 [B, N, T, D] block that was pooled in place ahead of the call
    clamped: bool = False                          # table form: the candidate rows were clamped into the tables in Python


class _DrinScore(torch.autograd.Function):
    """Autograd edge around drin_forward_staged / drin_backward_ex (loss.backward() of train.py:33-34).  `call.input_roles`
    names the batch tensors that follow the parameters in `tensors` (drin_input_grads fields; "token_block": a bf16
    [B, N, T, D] block that was pooled in place, whose gradient drin_pool_bwd writes in bf16)."""

    @staticmethod
    def forward(ctx, call: _Call, prepared: Optional[_Prepared], training: bool, *tensors: torch.Tensor):
        lib = _lib.load()
        ctx.roles = call.input_roles
        versions = tensors[:len(tensors) - len(ctx.roles)]
        params, pc = call.param_struct(versions)
        if prepared is not None:
            # the route says "prepared": fused two-layer inference on weights folded once per weight version
            pbuf = prepared.get(call, versions, pc)
            ws = call.byte_buffer(lib.drin_fused_workspace_bytes(C.byref(call.cfg)))
            scores = call.scores()
            _lib.check(lib.drin_forward_prepared(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), pbuf.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), scores.data_ptr(), call.stream()))
            return scores
        ws, scores = call.workspace(training), call.scores()
        # train.OverlappedStep: the previous update is still running on a side stream.  The pooling passes and static edges
        # of THIS step run under it; the stream waits for the event before the first weight is read
        ready = call.params_ready
        _lib.check(lib.drin_forward_staged(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(),
                                           scores.data_ptr(), 1 if training else 0, None,
                                           None if ready is None else ready.cuda_event, call.stream()))
        ctx.call, ctx.ws, ctx.pc, ctx.params = call, ws, pc, params
        return scores

    @staticmethod
    def backward(ctx, grad_scores: torch.Tensor):
        lib = _lib.load()
        call, params, roles = ctx.call, ctx.params, ctx.roles
        dev, owner = call.device, call.owner
        needs = ctx.needs_input_grad[3 + len(params):]
        need_feats = [r for r, n in zip(roles, needs) if n]
        gc, out = None, [None] * len(params)
        if any(ctx.needs_input_grad[3:3 + len(params)]):
            gc, out = _param_grads(call, params)
        ig, feat_out = None, {}
        if need_feats:
            ig = _lib.DrinInputGradsC()
            for role in need_feats:
                if role != "token_block":
                    feat_out[role] = torch.empty(call.keep[_INPUT_FIELDS[role]].shape, dtype=torch.float32, device=dev)
            if "token_block" in need_feats:   # pooled and token-0 gradients first, then the block in bf16 (drin_pool_bwd)
                for role in ("entity_text", "entity_text_cls"):
                    feat_out.setdefault(role, torch.empty(call.keep[_INPUT_FIELDS[role]].shape, dtype=torch.float32, device=dev))
            for role, t in feat_out.items():
                setattr(ig, role, t.data_ptr())
            scratch = call.byte_buffer(lib.drin_input_grad_scratch_bytes(C.byref(call.cfg)))
            ig.scratch, ig.scratch_bytes = scratch.data_ptr(), scratch.numel()
        g = grad_scores.to(torch.float32).contiguous()
        stream = call.stream()
        # data-parallel overlap: the library records `ready` once the GCN layers' gradients are complete; the hook -
        # GradBucket's - starts their all-reduce behind it, under the vertex encoders' dW products
        hook = owner._layers_ready_hook if gc is not None and owner is not None and owner.grad_bucket_enabled else None
        staged = hook is not None and owner._grad_flat is not None and out[0].data_ptr() == owner._grad_flat.data_ptr()
        ready = None
        if staged:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))              # creates the hipEvent_t; the library records it again
        _lib.check(lib.drin_backward_ex(C.byref(call.cfg), C.byref(call.batch), C.byref(ctx.pc), ctx.ws.data_ptr(), ctx.ws.numel(),
                                        g.data_ptr(), None if gc is None else C.byref(gc), None if ig is None else C.byref(ig),
                                        ready.cuda_event if staged else None, stream))
        if staged:
            offsets, live, _total = owner.bucket_layout()
            hook(owner._grad_flat[:live], offsets[8], ready)          # [vertex encoders | GCN layers | dead]: the layers start at slot 8
        feats = [feat_out.get(role) if n else None for role, n in zip(roles, needs)]
        if "token_block" in need_feats:
            block = call.token_block
            gb = torch.empty(block.shape, dtype=torch.bfloat16, device=dev)
            c = _lib.DrinConfigC.from_buffer_copy(call.cfg)
            c.entity_tokens, c.feature_dtype = block.shape[2], _lib.FEAT_BF16
            _lib.check(lib.drin_pool_bwd(C.byref(c), call.token_mask.data_ptr(), feat_out["entity_text"].data_ptr(),
                                         feat_out["entity_text_cls"].data_ptr(), gb.data_ptr(), stream))
            feats[roles.index("token_block")] = gb
        return (None, None, None, *out, *feats)


class Attribution(NamedTuple):
    """What `Model.attribute` returns: `scores [B, N]`, the explained `candidate [B]` (None when `weights` was given) and, per
    float tensor of the batch, input x gradient summed over the feature axis - fp32, on the batch's device."""
    scores: torch.Tensor
    candidate: Optional[torch.Tensor]
    mention_text: torch.Tensor             # [B, L]
    mention_image: torch.Tensor            # [B, P]
    mention_object_score: torch.Tensor     # [B, Km]
    entity_text: torch.Tensor              # [B, N, T] for token-level entities, [B, N] for pooled
    entity_image: torch.Tensor             # [B, N], inner dims summed
    entity_object_score: torch.Tensor      # [B, N, Ke]
    miet_similarity: torch.Tensor          # [B, N]
    mtei_similarity: torch.Tensor          # [B, N]


# positions in the 14-sequence of the tensors `Model.attribute` explains, under their `_INPUT_FIELDS` names (the object feature
# rows, positions 5 and 10, enter only cosines: their gradient x input is identically 0 and is not formed)
_ATTRIBUTED = {0: "mention_text", 4: "mention_image", 6: "mention_object_score", 7: "entity_text", 9: "entity_image",
               11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}


def _feat_dtype(t: torch.Tensor) -> int:
    return _lib.FEAT_BF16 if t.dtype == torch.bfloat16 else _lib.FEAT_F32


def _stored(t: torch.Tensor) -> torch.Tensor:
    """`t` as the attribution kernels read it: contiguous, bf16 kept as it is, anything else fp32."""
    return t.detach().contiguous() if t.dtype in (torch.float32, torch.bfloat16) else t.detach().to(torch.float32).contiguous()


@torch.no_grad()
def _rows_dot(x: torch.Tensor, g: torch.Tensor, lead: int) -> torch.Tensor:
    """`(x * g).sum` over everything behind the first `lead` dims, by `drin_rows_dot`: `x` fp32 or bf16 (read in place), `g` fp32."""
    x, g = _stored(x), g.contiguous()
    shape = tuple(x.shape[:lead])
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if out.numel():
        _lib.check(_lib.load().drin_rows_dot(x.data_ptr(), _feat_dtype(x), g.data_ptr(), out.data_ptr(), out.numel(),
                                             x.numel() // out.numel(), torch.cuda.current_stream(x.device).cuda_stream))
    return out


def _invalidate_after_load(module, _incompatible_keys) -> None:
    module.invalidate()


class Model(nn.Module):
    """`model_module.Model()` of `train.py:136` (drin/model.py:156-162)."""

    # mentions per library call: larger batches are scored in slices of this many (mentions are independent; the candidate
    # grouping of the per-mention sums depends on the size of the call - csrc/fused_forward.hip: 16 / 48 / whole-list
    # workgroups - so a mention's scores in calls of different sizes agree to fp32 re-association, <= 5e-6, and are the same
    # bits every run within one call size); the one-workgroup-per-(mention, chunk) grids of the row kernels stop at 65 535 mentions
    MAX_CALL_MENTIONS = MAX_CALL_MENTIONS     # (table_ops.py: the primitives' default slice)
    flat_buckets = True       # flatten_parameters / grad_bucket / LibraryAdam's flat form are built (EncoderModel: not)

    def __new__(cls, cfg: Optional[DrinConfig] = None, *args, **kwargs):
        """`Model(cfg)` with `mention_final_layer_name` "transformer" or "none" (args.py:28) is a
        `drin_amd.drin_encoders.EncoderModel`; the linear encoder - the default - is this class, untouched."""
        if cls is Model and not (cfg or default_config()).linear_mention_encoder:
            from .drin_encoders import EncoderModel
            return super().__new__(EncoderModel)
        return super().__new__(cls)

    def __init__(self, cfg: Optional[DrinConfig] = None, precision: str = "bf16x3", fused: bool = True,
                 grad_bucket: bool = True):
        """`cfg`: None reads an importable reference `common.args` (the no-argument `Model()` of `train.py:136`), else the
        WikiDiverse defaults (`config.default_config`).
        `precision`: "bf16x3" (default: split-bf16 MFMA, fp32-equivalent - measured <= 1.4e-6 on the scores against the
        reference's fp32 forward, <= 6e-6 on trained weights, bar 1e-4; 2x the rate of exact fp32), "f32" (exact fp32 MFMA) or
        "bf16x3_if16" (precision by contraction: split-bf16 except the folded entity-image contraction, which runs ONE pass of the
        FP16 matrix instruction on the image rows the stream kernel hands over as fp16 under a power-of-two scale per row, where the
        candidate list is long enough - N >= 64 - for the mean over candidates behind it to average its rounding noise down:
        <= 4e-6 on the scores at N = 101 with freshly initialised weights, <= 2e-5 with trained ones - inside the bar either way;
        for per-pair (not table-form) fp32-stored image rows of large inference calls at D = 768 / R = 2048; shorter lists, small
        calls, bf16-stored features and every other path run "bf16x3" bit for bit);
        `fused`: let inference calls (no parameter needs a gradient) take the folded two-layer path;
        `grad_bucket`: backward writes every gradient into one flat bucket the `.grad`s are views of (like DDP's
        `gradient_as_bucket_view`: a `.grad` kept across `zero_grad(set_to_none=True)` + `backward()` is overwritten)."""
        super().__init__()
        self.cfg = cfg or default_config()
        self.cfg.validate()
        self._prepared = _Prepared() if fused else None
        self.grad_bucket_enabled = grad_bucket
        self._grad_flat: Optional[torch.Tensor] = None
        self._bucket_in_flight = False                       # handed out by a backward pass that is still running
        self._layers_ready_hook = None                       # set by train.GradBucket(overlap=True): see _DrinScore.backward
        self._params_ready = None                            # set by train.OverlappedStep: event behind an update still in flight
        self._param_flat: Optional[torch.Tensor] = None
        self._layout = None
        # table-form calls: where the kernels report a candidate row outside the entity tables (drin_batch.index_status)
        self.validate_indices = os.environ.get("DRIN_VALIDATE", "") not in ("", "0")
        self._index_watch = IndexWatch(Model._raise_bad_index)   # the status words per device and their read-backs (table_ops.py)
        self.register_load_state_dict_post_hook(_invalidate_after_load)
        modes = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16x3_all": _lib.PREC_BF16X3_ALL, "bf16x3_if16": _lib.PREC_BF16X3_IF16}
        if precision not in modes:
            # ("bf16" - every contraction in one bf16 pass, 5e-4 - and "bf16x3_i1" - the image contraction in one bf16 pass, 1.6e-4 on
            #  trained weights - were outside the path's 1e-4 bar and were removed in round 5)
            raise ValueError(f"precision {precision!r}: one of {sorted(modes)}")
        self.precision = modes[precision]
        self.vertex_encoder = VertexEncoder(self.cfg)          # model.py:159 (RNG order: ghmfc.py:165,211; model.py:23-24)
        self.gcn_layers = nn.ModuleList([GCNLayer(self.cfg) for _ in range(self.cfg.num_gcn_layers)])  # model.py:161

    def invalidate(self) -> "Model":
        """Forget the folded weights of the fused inference path (and with them every `EntityTable` cache keyed on them).
        The folds are keyed on `(data_ptr, _version)` of the parameters, so optimiser steps, `load_state_dict` and in-place
        torch ops are detected by themselves; writes PyTorch's version counter does not see - `p.data.copy_(...)`,
        `p.data.mul_(...)`, EMA / weight swapping through `.data`, an external kernel - need this call."""
        if self._prepared is not None:
            self._prepared.invalidate()
        self.__dict__.pop("_link_inv", None)                  # link's inverse row norms: the same rule for writes into `rows`
        self.__dict__.pop("_link_edges_inv", None)            # and into the three tables of first_stage="edges"
        return self

    # ---- flat buckets (one all-reduce per step; train.py:55-56: one Adam launch) -------------------------
    def bucket_layout(self):
        params = _param_list(self)
        key = tuple(p.numel() for p in params)
        if self._layout is None or self._layout[0] != key:
            pl = 10 if self.cfg.gcn_edge_feature == "vector" else 8
            self._layout = (key,) + _bucket_layout(params, pl, self.cfg.gcn_edge_type == "dynamic")
        return self._layout[1:]

    def _bucket_grads(self, params: Sequence[torch.Tensor]) -> List[Optional[torch.Tensor]]:
        """Views of the flat gradient bucket for `params` (`_param_list` order; the dead ones get their own slots behind
        the live prefix and are never returned to autograd), zeroed with one memset.  A bucket some `.grad` still aliases
        (gradient accumulation over several backward passes) is left alone and a fresh one is taken - and so is a bucket
        an EARLIER node of the backward pass that is running now has handed out (two scoring calls in one graph:
        `loss(model(b1)) + loss(model(b2))`, or a training batch above MAX_CALL_MENTIONS): its views sit in autograd's
        input buffers while every `.grad` is still None, and the engine sums the two nodes' gradients itself."""
        offsets, live, total = self.bucket_layout()
        dev = params[0].device
        flat = self._grad_flat
        if flat is not None and (flat.device != dev or flat.numel() != total):
            flat = None
        if flat is not None:
            base = flat.untyped_storage().data_ptr()
            if any(p.grad is not None and p.grad.untyped_storage().data_ptr() == base for p in self.parameters()):
                flat = None
        views = lambda f: [f[o:o + p.numel()].view(p.shape) for o, p in zip(offsets, params)]
        if self._bucket_in_flight:
            extra = torch.empty(total, dtype=torch.float32, device=dev)   # not the model's bucket: the sums will be new tensors
            extra[:live].zero_()
            return views(extra)
        if flat is None:
            flat = torch.empty(total, dtype=torch.float32, device=dev)
        self._grad_flat = flat
        flat[:live].zero_()
        self._bucket_in_flight = True
        try:                                                  # cleared when the engine finishes this backward pass
            torch.autograd.Variable._execution_engine.queue_callback(self._bucket_landed)
        except RuntimeError:                                  # not inside a backward pass (a direct call): nothing in flight
            self._bucket_in_flight = False
        return views(flat)

    def _bucket_landed(self) -> None:
        self._bucket_in_flight = False

    def grad_bucket(self) -> Optional[torch.Tensor]:
        """The live prefix of the flat gradient bucket when every current `.grad` is a view of it, else None."""
        flat = self._grad_flat
        if flat is None:
            return None
        offsets, live, _total = self.bucket_layout()
        base, seen = flat.data_ptr(), False
        for o, p in zip(offsets, _param_list(self)):
            if p.grad is None:
                continue
            if p.grad.data_ptr() != base + 4 * o or not p.grad.is_contiguous():
                return None
            seen = True
        return flat[:live] if seen else None

    def flatten_parameters(self) -> torch.Tensor:
        """Move every parameter into one flat fp32 bucket laid out like the gradient bucket (`p.data` become views; values,
        `state_dict` keys and `load_state_dict` are unaffected).  Returns the bucket; idempotent; redo after `.to(...)`."""
        params = _param_list(self)
        offsets, _live, total = self.bucket_layout()
        flat = self._param_flat
        ok = (flat is not None and flat.device == params[0].device and flat.numel() == total
              and all(p.data_ptr() == flat.data_ptr() + 4 * o and p.is_contiguous() for o, p in zip(offsets, params)))
        if not ok:
            flat = torch.zeros(total, dtype=torch.float32, device=params[0].device)
            with torch.no_grad():
                for o, p in zip(offsets, params):
                    view = flat[o:o + p.numel()].view(p.shape)
                    view.copy_(p.data)
                    p.data = view
            self._param_flat = flat
            self.invalidate()
        return flat

    def __getstate__(self):
        # copy.deepcopy / pickle of the Module: the index watch holds HIP events and pinned buffers of calls in flight - per-process
        # bookkeeping, not state (IndexWatch copies empty; the copy's first table-form call makes its own status words)
        state = self.__dict__.copy()
        state.pop("_link_inv", None)                          # (and link's norms cache holds the caller's `rows`)
        state.pop("_link_edges_inv", None)
        return state

    # ---- candidate rows outside the entity tables (drin/data.py:87-93 raises IndexError) ------------------------------
    def _status_words(self, device: torch.device) -> torch.Tensor:
        return self._index_watch.words(device)

    @staticmethod
    def _raise_bad_index(words) -> None:
        _flag, pair, value = decode_status(words)
        what = f"row {value} at pair {pair} (b * N + n)" if value != 0 else "a row of a training batch"
        raise IndexError(f"IndexedBatch.candidates: {what} is outside the entity tables (it was clamped: the scores of that call are of the "
                         f"WRONG entity there); the reference's fancy index, drin/data.py:87-93, raises here too")

    def _watch_indices(self, device: torch.device) -> None:
        """After a table-form call: raise at once when validating eagerly, else start an asynchronous read-back of the status
        words which `forward` / `check_indices` look at once it has landed (no synchronisation is added to the step)."""
        self._index_watch.after_call(device, self.validate_indices)

    def check_indices(self, wait: bool = True) -> None:
        """Raise `IndexError` if any table-form call since the last check met a candidate row outside `[0, E - 1]`.  `wait=True`
        synchronises with the device (call it where the loop synchronises anyway: `MELRunner.run_epoch` does, at the epoch's
        end); `wait=False` only looks at read-backs that have already landed.  `Model(...).validate_indices = True` (or
        `DRIN_VALIDATE=1`) checks after every call instead - the reference's behaviour, at one synchronisation per call."""
        self._index_watch.check(wait)

    def forward(self, batch) -> torch.Tensor:
        if self._index_watch.pending() and not torch.cuda.is_current_stream_capturing():
            self.check_indices(wait=False)
        B = batch.candidates.shape[0] if isinstance(batch, IndexedBatch) else batch[0].shape[0]
        if B > self.MAX_CALL_MENTIONS:
            return torch.cat([self._forward(part) for part in _split_mentions(batch, self.MAX_CALL_MENTIONS)], 0)
        return self._forward(batch)

    def _unfused_precision(self) -> int:
        """"bf16x3_if16" is a mode of the fused inference path; anything else it meets runs split-bf16."""
        return _lib.PREC_BF16X3 if self.precision in _FUSED_ONLY else self.precision

    def _route(self, batch, params) -> _Route:
        """THE place where the library path of one call is chosen (`_forward` runs what it returns).  Geometry is the library's
        to judge - `drin_fused_supported`, `drin_indexed_supported`, each asked at most once; what is tested here is what only
        this side knows.  Table form: the kernels read the tables through the candidate index on the folded and
        cached inference paths and when training on pooled tables; everything else (exact-fp32 precision, geometries off those
        paths, batch tensors that require grad) gathers the rows with torch indexing."""
        lib = _lib.load()
        # grad mode is already off inside Function.forward (and needs_input_grad ignores no_grad), so the caller's mode is read
        # here.  Any parameter or float batch tensor requiring grad: the layer-by-layer forward that keeps what backward reads
        feat_grad = torch.is_grad_enabled() and _batch_requires_grad(batch)
        training = feat_grad or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
        folds = not training and self._prepared is not None
        planes, unfused = self.precision in _PLANES, self._unfused_precision()
        fused = None

        def fused_supported(call: _Call) -> bool:      # asked once per route: gathering the rows does not change the answer
            nonlocal fused
            if fused is None:
                fused = lib.drin_fused_supported(C.byref(call.cfg)) == _lib.OK
            return fused
        seq, cls, block, clamped = batch, None, None, False
        if isinstance(batch, IndexedBatch):
            t = batch.table
            tables = lambda text, mask: batch.mention + [text, mask, t.image, t.object, t.object_score,  # noqa: E731
                                                         batch.miet_similarity, batch.mtei_similarity]
            if folds and (planes or t.cache_enabled):
                call = _Call.described(self.cfg, tables(t.text, t.mask), unfused, entity_index=batch.candidates,
                                       index_status=self._status_words(batch.candidates.device))
                if fused_supported(call):
                    if not t.cache_enabled:    # bf16-stored features are read in place (never widened: the table is large)
                        return _Route("prepared", call.convert(in_place=self.precision), False)
                    if t.text.dtype == torch.bfloat16:
                        raise ValueError("the per-entity cache is built from fp32 tables; give EntityTable fp32 features")
                    return _Route("cached", call.convert(), False)         # per-entity precompute cache
            batch, clamped = self._clamped(batch), True                # whatever follows trusts the index
            # training on a token-level table: every entity's tokens pooled once; the step then reads the pooled / token-0 /
            # image / object tables through the candidate index inside the kernels, or gathers those rows (always from a bf16
            # table, which `_Call` would widen whole).  With a batch tensor that requires grad the token rows themselves are
            # gathered: torch's indexing backward must reach them
            pooled = training and not feat_grad and t.text.dim() == 3
            if pooled and all(x.dtype == torch.float32 for x in (t.text, t.image, t.object)):
                text, rows0 = t.pooled_text(self.cfg)
                dummy = torch.zeros(batch.candidates.shape[0], dtype=torch.int64, device=batch.candidates.device)
                call = _Call.described(self.cfg, tables(text, dummy), unfused, entity_index=batch.candidates, entity_text_cls=rows0)
                if lib.drin_indexed_supported(C.byref(call.cfg)) == _lib.OK:
                    return _Route("layers", call.convert(), True, None, True)
            seq, cls = batch.gathered_pooled(self.cfg) if pooled else (batch.gathered(), None)
        if (cls is None and training and len(seq) >= 14 and seq[7].dtype == torch.bfloat16 and seq[7].dim() == 4
                and seq[7].is_cuda and seq[7].shape[0] > 0):
            # a training step on bf16-stored token blocks: pooled in place by the library - half the bytes, no widened copy of
            # the 197 KB per candidate - then the pooled-ahead form below
            etf, emask = seq[7], seq[8]
            seq = list(seq[:7]) + [_pool_tokens(etf, emask), torch.zeros(etf.shape[0], dtype=torch.int64, device=etf.device)] \
                + list(seq[9:])
            cls = etf[:, :, 0, :]
            if etf.requires_grad:
                # the block's gradient comes from drin_pool_bwd, written in bf16 (never widened): token 0 is not a graph input
                block, cls = etf, cls.detach()
        if cls is not None:
            # pooled-ahead batch: the layer-by-layer entry points (the fused path folds the pooling into its one pass)
            call = _Call(self.cfg, seq, unfused, entity_text_cls=cls)
            if block is not None:
                call.token_block, call.token_mask = block, emask.to(device=block.device, dtype=torch.int64).contiguous()
            return _Route("layers", call, True, block, clamped)
        call = _Call.described(self.cfg, seq, unfused)
        if folds and fused_supported(call):
            # features stored as bf16 are read in place by the fused inference path in split-bf16 precision; every
            # other path (training, exact fp32, geometries off the fused path) gets them widened to fp32 - exact
            return _Route("prepared", call.convert(in_place=self.precision if planes else None), False, None, clamped)
        return _Route("layers", call.convert(), training, None, clamped)

    def _forward(self, batch) -> torch.Tensor:
        params = _param_list(self)
        route = self._route(batch, params)
        call, indexed = route.call, route.call.cfg.num_entities > 0       # the kernels read the tables through the index
        if route.clamped and not indexed:
            self._watch_indices(call.device)                           # before scoring: with validate_indices, the raise
        if call.B == 0 and not (indexed and route.path == "prepared"):  # (that one goes on: the library validates its geometry)
            out = call.scores()
        elif route.path == "cached":
            out = self._forward_cached(call, batch.table, params)
        else:
            out = self._score(call, self._prepared if route.path == "prepared" else None, route.training, *params,
                              feats=_feature_inputs(call, route.token_block) if route.training else ((), ()))
        if indexed:
            self._watch_indices(call.device)                           # the kernels clamp and report: after their launches
        return out

    def attribute(self, batch, candidate: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None) -> Attribution:
        """Gradient x input of `sum(weights * scores)` for every float tensor of the batch, summed over the feature axis: what
        `(x * x.grad).sum(-1)` gives on the reference's plain-torch forward with the model frozen.
        `batch`: the 14-sequence (fp32 or bf16 features) or an `IndexedBatch`.  `weights [B, N]` float, or `candidate [B]` int64 (a
        one-hot row per mention), not both; with neither, each mention's arg-max over the first N - 1 columns (the reference's
        loss and metric drop the answer slot, common/utils.py:36-37,61-62).
        Token-level entity text is attributed per token `[B, N, T]` WITHOUT its `[B, N, T, D]` gradient: the tokens are pooled
        ahead, the scoring backward returns the pooled rows' gradient `[B, N, D]`, and `drin_token_attribution` contracts it with
        the original block - or with the token table through the candidate index, nothing gathered.  Two identities are used:
        token 0 feeds only the text-text cosine (model.py:73-75) and the object feature rows feed only cosines (model.py:78-92); a
        cosine is homogeneous of degree 0 in each row, so `<x, d cos / dx> = 0` (Euler): token 0 is exactly 0 and the object
        feature rows are NOT returned.
        Works whatever `self.training` and the parameters' `requires_grad` say and changes neither; no parameter and no tensor of
        the caller receives a `.grad`.  Precision "f32" or split-bf16 ("bf16x3_if16" runs as "bf16x3").  A mention with an empty
        span is NaN in its own rows only.
        The token kernel reads the tokens where they are, so their storage matters: a token TABLE must be contiguous float32 or
        bfloat16 (`ValueError` otherwise: widening or copying a table is the caller's decision); a per-pair token BLOCK of another
        dtype is widened to fp32 and a non-contiguous one is copied, once - the one case in which a block-sized tensor is made.
        A `candidate` outside `[0, N - 1]` is clamped without a synchronisation; `validate_indices` raises `IndexError` instead."""
        if candidate is not None and weights is not None:
            raise ValueError("attribute: give `candidate` or `weights`, not both")
        if isinstance(batch, IndexedBatch) and batch.table.text.dim() == 3:
            text = batch.table.text
            if text.dtype not in (torch.float32, torch.bfloat16) or not text.is_contiguous():
                raise ValueError(f"attribute: the token table is read in place and must be contiguous float32 or bfloat16 (got {text.dtype}"
                                 f"{'' if text.is_contiguous() else ', not contiguous'}); convert the EntityTable once")
        if self._index_watch.pending() and not torch.cuda.is_current_stream_capturing():
            self.check_indices(wait=False)
        B = batch.candidates.shape[0] if isinstance(batch, IndexedBatch) else batch[0].shape[0]
        N = self.cfg.num_candidates_model
        for name, t, shape in (("weights", weights, (B, N)), ("candidate", candidate, (B,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"attribute: {name} has shape {tuple(t.shape)}, expected {shape}")
        step = self.MAX_CALL_MENTIONS
        if B <= step:
            return self._attribute(batch, candidate, weights)
        parts = [self._attribute(part, None if candidate is None else candidate[b0:b0 + step],
                                 None if weights is None else weights[b0:b0 + step])
                 for b0, part in zip(range(0, B, step), _split_mentions(batch, step))]
        return Attribution(*(None if parts[0][k] is None else torch.cat([p[k] for p in parts], 0) for k in range(len(parts[0]))))

    def _attribute(self, batch, candidate, weights) -> Attribution:
        """One library call's worth of `attribute` (at most MAX_CALL_MENTIONS mentions)."""
        lib = _lib.load()
        table, index = None, None
        if isinstance(batch, IndexedBatch):
            batch = self._clamped(batch)                               # the torch gathers and the token kernel trust the index
            self._watch_indices(batch.candidates.device)
            table, index = batch.table, batch.candidates.contiguous()
            if table.text.dim() == 3:
                seq, cls = batch.gathered_pooled(self.cfg)             # pooled per ENTITY, once per table version
                tokens, mask = table.text, table.mask
            else:
                seq, cls, tokens, mask = batch.gathered(), None, None, None
        else:
            if len(batch) not in (14, 15):
                raise ValueError(f"batch must be the 14-sequence of drin/data.py:110-126 (got {len(batch)} items)")
            seq, cls, tokens, mask = list(batch[:14]), None, None, None
            etf = seq[7]
            if etf.dim() == 4:                                         # token-level: pooled ahead, the block is read once in place
                if etf.dtype not in (torch.float32, torch.bfloat16):
                    etf = etf.to(torch.float32)
                tokens, mask = etf.detach().contiguous(), seq[8]       # (a copy only of a non-contiguous block, and the only one)
                cls = tokens[:, :, 0, :]
                seq[7], seq[8] = _pool_tokens(tokens, mask), torch.zeros(etf.shape[0], dtype=torch.int64, device=etf.device)
        dev = seq[0].device
        # detached fp32 leaves of the small tensors (a view of the caller's storage where that is fp32 and contiguous already)
        leaves = {}
        for i, field in _ATTRIBUTED.items():
            leaves[field] = seq[i].detach().to(torch.float32).contiguous().requires_grad_(True)
        call_seq = [leaves[_ATTRIBUTED[i]] if i in _ATTRIBUTED else (t.detach() if torch.is_tensor(t) else t)
                    for i, t in enumerate(seq[:14])]
        params = [p.detach() for p in _param_list(self)]              # no parameter is asked for a gradient: drin_backward_ex gets grads = NULL
        with torch.enable_grad():
            call = _Call(self.cfg, call_seq, self._unfused_precision(), entity_text_cls=None if cls is None else cls.detach())
            Bc, N = call.B, call.N
            scores = call.scores() if Bc == 0 else self._score(call, None, True, *params, feats=_feature_inputs(call))
        with torch.no_grad():
            if weights is None:
                if candidate is None:
                    chosen = scores.detach()[:, :max(N - 1, 1)].argmax(1)
                else:
                    raw = candidate.to(device=dev, dtype=torch.int64)
                    chosen = raw.clamp(0, N - 1)                       # never an out-of-range scatter; no synchronisation
                    if self.validate_indices and Bc and not torch.cuda.is_current_stream_capturing() and not bool((chosen == raw).all()):
                        raise IndexError(f"attribute: candidate must be in [0, {N - 1}]")
                G = torch.zeros(Bc, N, dtype=torch.float32, device=dev)
                G.scatter_(1, chosen.view(-1, 1), 1.0)
            else:
                chosen, G = None, weights.to(device=dev, dtype=torch.float32).contiguous()
        fields = list(leaves)
        if Bc == 0:
            grads = [torch.zeros_like(leaves[f]) for f in fields]
        else:
            grads = torch.autograd.grad(scores, [leaves[f] for f in fields], grad_outputs=G)
        g = dict(zip(fields, grads))
        with torch.no_grad():
            x = {field: seq[i] for i, field in _ATTRIBUTED.items()}
            if tokens is not None and Bc == 0:
                entity_text = torch.empty(0, N, tokens.shape[-2], dtype=torch.float32, device=dev)
            elif tokens is not None:
                T, D = tokens.shape[-2], tokens.shape[-1]
                mask = mask.to(device=dev, dtype=torch.int64).contiguous()
                entity_text = torch.empty(Bc, N, T, dtype=torch.float32, device=dev)
                gp = g["entity_text"].contiguous()
                _lib.check(lib.drin_token_attribution(
                    tokens.data_ptr(), _feat_dtype(tokens), mask.data_ptr(), None if index is None else index.data_ptr(),
                    0 if table is None else table.num_entities, None if index is None else self._status_words(dev).data_ptr(),
                    gp.data_ptr(), entity_text.data_ptr(), Bc * N, T, D, call.stream()))
            else:
                entity_text = _rows_dot(x["entity_text"], g["entity_text"], 2)
            out = Attribution(
                scores=scores.detach(), candidate=chosen,
                mention_text=_rows_dot(x["mention_text"], g["mention_text"], 2),
                mention_image=_rows_dot(x["mention_image"], g["mention_image"], 2),
                mention_object_score=leaves["mention_object_score"].detach() * g["mention_object_score"],
                entity_text=entity_text,
                entity_image=_rows_dot(x["entity_image"], g["entity_image"], 2),
                entity_object_score=leaves["entity_object_score"].detach() * g["entity_object_score"],
                miet_similarity=leaves["miet_similarity"].detach() * g["miet_similarity"],
                mtei_similarity=leaves["mtei_similarity"].detach() * g["mtei_similarity"])
        return out

    @torch.no_grad()
    def link(self, mention: Sequence[torch.Tensor], table: EntityTable, k: int, clip_image: torch.Tensor, clip_text: torch.Tensor, *,
             candidates: Optional[torch.Tensor] = None, queries: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
             first_stage: Optional[str] = None, edge_weights: Optional[Sequence[float]] = None):
        """DRIN as the second stage behind a first stage, against a device-resident table: the `k` best of
        `N = cfg.num_candidates_model` candidate rows per mention by the model's own score - `LinkResult(scores [B, k], rows [B, k])`,
        table rows, ordered by the contract of include/drin_hip.h (higher score first, the lower row between equal scores, between
        equal scores on equal rows the earlier candidate slot, NaN last; scores canonical: +0.0 for -0.0, one quiet NaN).
        `mention`: the seven mention-side tensors of the 14-sequence; `clip_image` / `clip_text`: the mentions' projected CLIP
        embeddings `[B, C]` float32; `table` with `set_clip` rows.  The candidates are EITHER `candidates [B, N]` int64 rows of the
        table (for example `ghmfc_model.link(...).rows`) OR come from a cosine first stage: `queries [B, Dq]` against `rows [E, Dq]`
        (float32; `rows` may be bfloat16, read in place - DESIGN.md section 34), the `N` best by `drin_table_topk` in the model's precision (N <= 256; inverse row norms cached per version of
        the `rows` tensor, which the model keeps a reference to until another one is given).  ALL `N` slots are candidates: in linking there is no answer slot (the reference's loss and metric drop the last
        column, common/utils.py:36-37), so none is dropped.  Then `IndexedBatch.from_clip` forms the two CLIP edges, the model's
        own forward scores the batch on whatever route it takes (the per-entity cache when the table has it enabled) and
        `drin_rank_rows` orders each mention's list.  `eval()` only, no gradient, GPU only.

        `first_stage="edges"` (`candidates`, `queries` and `rows` all None): DRIN lists its own candidates,
        the `N` best rows of the table by the sum of three of its four layer-0 edges (`drin_table_topk_sum`, the model's
        precision, N <= 256) - `tt`: `span_mean(mention_text, start, end)` against the rows the table-form forward takes the
        text-text edge from (the token-0 copy of `table.pooled_text` for a token-level table, the text rows of a pooled one);
        `ti`: `clip_text` against `table.clip_image`; `it`: `clip_image` against `table.clip_text`.  The image-image edge `ii` joins as a
        fourth term when `edge_weights` has four entries and the fourth is not zero: `drin_object_rows` of
        `mention[5]` / `mention[6]` against `table.object_rows(cfg)`, the RATIO form `(q . u) / (S T + cfg.miei_eps)` of
        `drin_table_topk_sum_forms` - all four edges the model reads at layer 0; `(0, 0, 0, 1)` ranks by it alone and reads no text
        and no CLIP rows.  `edge_weights`: three floats (default `cfg.gcn_edge_enabled[0:3]`) or four; a zero drops its term, whose
        tensors are then not read; all zero is refused.  Three entries make the three-term call as it was: its launches, its bits.
        The inverse row norms of the three tables are cached per tensor version (the rule of `rows` above; `invalidate()` drops
        them); `u` and `T` per version of the table's object tensors (`EntityTable.object_rows`).  A mention with an EMPTY span has a NaN `tt` row: all its first-stage scores
        are NaN and its candidates are rows `0 .. N-1` by the contract - it is not treated specially.

        bf16-stored tables: `table.text` (with the other five feature tensors: all six bfloat16, or none) and
        the `set_clip` rows may be bfloat16.  Every first stage reads them in place and lists what it would list on their exactly
        widened float32 copies; `tt`'s query is then the span mean of the bfloat16 mention text read in place
        (`drin_mention_rows_fwd`), its table the bfloat16 token-0 copy.  The second stage is the model's forward on the bf16 table
        (route "prepared"; such a table with the cache enabled keeps its `ValueError`)."""
        if self.training:
            raise RuntimeError("Model.link: ranking is eval() only (no gradient flows through a top-k): call .eval()")
        if first_stage is not None:
            if first_stage != "edges":
                raise ValueError(f"Model.link: first_stage = {first_stage!r} is not None or 'edges'")
            if candidates is not None or queries is not None or rows is not None:
                raise ValueError("Model.link: first_stage='edges' conflicts with `candidates` / `queries` / `rows`: it lists its own "
                                 "candidates from the table - pass none of them")
        elif edge_weights is not None:
            raise ValueError("Model.link: `edge_weights` goes with first_stage='edges'")
        edges, cosine_stage = first_stage is not None, queries is not None or rows is not None   # section 33's stage, section 32's
        if not edges and cosine_stage == (candidates is not None):
            raise ValueError("Model.link: give exactly one first stage - `candidates` [B, N], or `queries` [B, Dq] with `rows` [E, Dq]")
        if cosine_stage and (queries is None or rows is None):
            raise ValueError("Model.link: `queries` [B, Dq] and `rows` [E, Dq] go together")
        N, k = self.cfg.num_candidates_model, int(k)
        if candidates is not None and (candidates.dim() != 2 or candidates.shape[1] != N):
            raise ValueError(f"Model.link: candidates has shape {tuple(candidates.shape)}, expected [B, {N}] (cfg.num_candidates_model)")
        if k < 1 or k > N:
            raise ValueError(f"Model.link: k = {k} is not in [1, N = {N}]")
        if table.clip_text is None or table.clip_image is None:
            raise ValueError("Model.link: the table has no CLIP rows: call table.set_clip(clip_text, clip_image)")
        if edges:
            candidates = self._edge_candidates(mention, table, clip_image, clip_text, edge_weights)
        if cosine_stage:
            if N > _lib.TOPK_MAX_K:
                raise ValueError(f"Model.link: a cosine first stage lists at most {_lib.TOPK_MAX_K} rows and N = {N}: pass `candidates`")
            if (queries.dim() != 2 or rows.dim() != 2 or queries.shape[1] != rows.shape[1] or rows.shape[0] != table.num_entities
                    or queries.dtype != torch.float32 or rows.dtype not in (torch.float32, torch.bfloat16)
                    or (rows.dtype == torch.bfloat16 and rows.shape[1] % 8 != 0)):
                raise ValueError(f"Model.link: queries {tuple(queries.shape)} / rows {tuple(rows.shape)} must be float32 [B, Dq] and "
                                 f"[E = {table.num_entities}, Dq] (rows: or bfloat16 with Dq % 8 == 0, read in place)")
            if N > rows.shape[0]:
                raise ValueError(f"Model.link: N = {N} candidates exceed the table's {rows.shape[0]} entities")
            if rows.device.type != "cuda" or queries.device != rows.device:
                raise RuntimeError("Model.link runs on an AMD GPU only (no CPU / eager fallback); move queries and rows to 'cuda'")
            _key, inv, _given, rows = self._norms_entry(self.__dict__, "_link_inv", rows)
            B = queries.shape[0]
            if B == 0:
                candidates = torch.empty(0, N, dtype=torch.int64, device=rows.device)
            else:
                q, precision = queries.detach().contiguous(), "f32" if self.precision == _lib.PREC_F32 else "bf16x3"
                candidates = in_slices(B, self.MAX_CALL_MENTIONS,
                                       lambda sl: table_topk(q[sl], rows, inv, N, self.cfg.cosine_eps, precision).rows)
        if candidates.device.type != "cuda":
            raise RuntimeError("Model.link runs on an AMD GPU only (no CPU / eager fallback); move the batch to 'cuda'")
        candidates = candidates.detach().to(torch.int64).contiguous()
        if candidates.shape[0] == 0:
            return LinkResult(torch.empty(0, k, dtype=torch.float32, device=candidates.device),
                              torch.empty(0, k, dtype=torch.int64, device=candidates.device))
        batch = IndexedBatch.from_clip(mention, table, candidates, clip_image, clip_text, model=self)
        scores = self(batch).contiguous()
        B, dev = candidates.shape[0], candidates.device
        out_scores = torch.empty(B, k, dtype=torch.float32, device=dev)
        out_rows = torch.empty(B, k, dtype=torch.int64, device=dev)
        lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
        for b0 in range(0, B, self.MAX_CALL_MENTIONS):
            sl = slice(b0, min(B, b0 + self.MAX_CALL_MENTIONS))
            _lib.check(lib.drin_rank_rows(_ptr(scores[sl]), _ptr(candidates[sl]), sl.stop - b0, N, k, _ptr(out_scores[sl]),
                                          _ptr(out_rows[sl]), None, stream))
        return LinkResult(out_scores, out_rows)

    def _norms_entry(self, cache: dict, slot, given: torch.Tensor) -> tuple:
        """`(key, inverse row norms, given, dense)` of `cache[slot]`, the norms cache of `link`, rebuilt when the key moved.  The
        norms are per version of the CALLER's tensor: the entry keeps that tensor alive - a key of an address and a version says
        nothing once the memory behind it may have been freed and handed out again - and, for a non-contiguous `given`, the
        contiguous copy the norms were taken of (a copy made per call would start at version 0 in whatever block the allocator
        hands back).  While the entry holds the tensor, an equal address means the same storage, whose version counter every
        in-place torch op bumps (writes through `.data`: Model.invalidate())."""
        key = (given.data_ptr(), given._version, tuple(given.shape), tuple(given.stride()), given.dtype, self.cfg.cosine_eps)
        entry = cache.get(slot)
        if entry is None or entry[0] != key:
            cache[slot] = entry = None                                    # release the stale copy before allocating
            dense = given.detach().contiguous()
            cache[slot] = entry = (key, row_inv_norms(dense, self.cfg.cosine_eps), given, dense)
        return entry

    def _edge_candidates(self, mention, table: EntityTable, clip_image, clip_text, edge_weights) -> torch.Tensor:
        """`candidates [B, N]` of `link(first_stage="edges")`: the N best table rows by the weighted sum of the tt, ti and it
        cosines (`table_topk_sum`) and, with a fourth weight, of the image-image edge as a `RatioTerm`; the checks of that mode."""
        weights = self.cfg.gcn_edge_enabled[0:3] if edge_weights is None else tuple(edge_weights)
        if len(weights) not in (3, 4):
            raise ValueError(f"Model.link: edge_weights has {len(weights)} entries, expected 3 (tt, ti, it) or 4 (tt, ti, it, ii)")
        weights = tuple(float(w) for w in weights)
        if all(w == 0.0 for w in weights):
            raise ValueError(f"Model.link: first_stage='edges' with all {'three' if len(weights) == 3 else 'four'} edge weights zero "
                             "ranks nothing")
        w_ii = weights[3] if len(weights) == 4 else 0.0                   # the image-image edge: a RATIO term behind the three cosines
        weights = weights[:3]
        if len(mention) != 7:
            raise ValueError("Model.link: mention must be the first 7 tensors of the 14-sequence (drin/data.py:110-117)")
        N = self.cfg.num_candidates_model                               # (link() has refused a table without CLIP rows)
        if N > _lib.TOPK_MAX_K:
            raise ValueError(f"Model.link: a cosine first stage lists at most {_lib.TOPK_MAX_K} rows and N = {N}: pass `candidates`")
        if N > table.num_entities:
            raise ValueError(f"Model.link: N = {N} candidates exceed the table's {table.num_entities} entities")
        mtf, start, end = mention[0], mention[2], mention[3]
        B, C = mtf.shape[0], table.clip_text.shape[1]
        for name, t in (("clip_image", clip_image), ("clip_text", clip_text)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, C):
                raise ValueError(f"Model.link: {name} must be float32 [{B}, {C}] (got {getattr(t, 'dtype', None)} "
                                 f"{tuple(getattr(t, 'shape', ()))})")
        stored = (torch.float32, torch.bfloat16)
        if weights[0] != 0.0 and (table.text.dtype not in stored or mtf.dtype != table.text.dtype):   # tt's tensors, when tt is a term
            raise NotImplementedError("Model.link: first_stage='edges' reads mention and table text of ONE storage, float32 or bfloat16 - all "
                                      f"six feature tensors as bfloat16, or none (got mention {mtf.dtype}, table {table.text.dtype}: mixed "
                                      "bf16-stored rows are not built)")
        if weights[0] != 0.0 and mtf.dtype == torch.bfloat16 and mtf.shape[-1] % 8 != 0:
            raise ValueError(f"Model.link: bfloat16 text rows of width {mtf.shape[-1]}: the width must be a multiple of 8")
        mobj, mscore = mention[5], mention[6]
        if w_ii != 0.0:                                                   # ii's tensors, when ii is a term
            if table.object is None or table.object_score is None:
                raise ValueError("Model.link: the image-image edge needs the table's object rows (`object` / `object_score` is None)")
            if mobj.dim() == 4 and mobj.shape[2] == 1:
                mobj = mobj[:, :, 0, :]                                   # the mean over one region row is that row
            if mobj.dim() != 3 or tuple(mscore.shape) != tuple(mobj.shape[:2]) or mobj.dtype != table.object.dtype or mscore.dtype != mobj.dtype:
                raise NotImplementedError(f"Model.link: the image-image edge reads mention objects [B, Km, (1,) R] and scores [B, Km] in the "
                                          f"table's storage (got {tuple(mention[5].shape)} {mention[5].dtype}, {tuple(mscore.shape)} "
                                          f"{mscore.dtype}, table {table.object.dtype}; a region mean over more than one row is not built)")
        dev = table.text.device
        placed = (mtf, start, end, clip_image, clip_text, table.clip_text, table.clip_image)
        placed += (mobj, mscore, table.object, table.object_score) if w_ii != 0.0 else ()
        if dev.type != "cuda" or any(t.device != dev for t in placed):
            raise RuntimeError("Model.link runs on an AMD GPU only (no CPU / eager fallback); move the batch and the table to 'cuda'")
        if B == 0:
            return torch.empty(0, N, dtype=torch.int64, device=dev)
        eps = self.cfg.cosine_eps
        # (query, table rows) per edge, in edge order; a dropped term's tensors are not touched - not even the token-0 copy is made
        sources = ((lambda: row_ops.span_mean(mtf, start, end) if mtf.dtype == torch.float32 else self._span_mean_stored(mtf, start, end),
                    lambda: table.pooled_text(self.cfg)[1] if table.text.dim() == 3 else table.text),
                   (lambda: clip_text, lambda: table.clip_image),
                   (lambda: clip_image, lambda: table.clip_text))
        cache = self.__dict__.setdefault("_link_edges_inv", {})           # the inverse norms, a slot per edge (_norms_entry's rule)
        terms = []
        for s, (w, (query, rows_of)) in enumerate(zip(weights, sources)):
            if w == 0.0:
                terms.append((None, None, None, 0.0))
                continue
            _key, inv, _given, dense = self._norms_entry(cache, s, rows_of())
            terms.append((query().detach().contiguous(), dense, inv, w))
        precision = "f32" if self.precision == _lib.PREC_F32 else "bf16x3"
        if w_ii != 0.0:
            u, T = table.object_rows(self.cfg)
            q, S = object_rows(mobj.detach().contiguous(), mscore.detach().contiguous(), eps)
            return in_slices(B, self.MAX_CALL_MENTIONS, lambda sl: table_topk_sum(
                [(None if x is None else x[sl], r, i, w) for x, r, i, w in terms] + [RatioTerm(q[sl], S[sl], u, T, w_ii, self.cfg.miei_eps)],
                N, eps, precision).rows)
        return in_slices(B, self.MAX_CALL_MENTIONS, lambda sl: table_topk_sum(
            [(None if x is None else x[sl], r, i, w) for x, r, i, w in terms], N, eps, precision).rows)

    @staticmethod
    def _span_mean_stored(text: torch.Tensor, start: torch.Tensor, end: torch.Tensor) -> torch.Tensor:
        """`[B, D]` float32: the span mean of bfloat16 mention text `[B, L, D]`, read in place (`drin_mention_rows_fwd` with
        `DRIN_FEAT_BF16`: the row the fused forward takes its text-text edge from on bf16-stored features)."""
        text = text.detach().contiguous()
        B, L, D = text.shape
        # the positions as the kernel reads them - int64, contiguous, on the text's device - held in locals across the launch
        # (row_ops.span_mean's rule: any integer dtype is taken, a wrong length is refused before the launch)
        start, end = (torch.as_tensor(t).to(text.device, torch.int64).contiguous() for t in (start, end))
        if tuple(start.shape) != (B,) or tuple(end.shape) != (B,):
            raise ValueError(f"Model.link: mention start {tuple(start.shape)} / end {tuple(end.shape)} are not [batch] = {(B,)}")
        out = torch.empty(2, B, D, dtype=torch.float32, device=text.device)   # the edge row and the (equal) vertex row
        _lib.check(_lib.load().drin_mention_rows_fwd(_ptr(text), _lib.FEAT_BF16, None, _ptr(start), _ptr(end), _lib.REPR_AVG_EXTRACT,
                                                     _ptr(out[0]), _ptr(out[1]), None, B, L, D,
                                                     torch.cuda.current_stream(text.device).cuda_stream))
        return out[0]

    def wait_for_parameters(self) -> None:
        """Make the current stream wait for an optimiser update `train.OverlappedStep` left running on its side stream (no-op
        otherwise).  Every path that reads the parameters calls it - or, the layer-by-layer forward, hands the event to
        `drin_forward_staged` so that its parameter-free head runs under the update."""
        ev, self._params_ready = self._params_ready, None
        if ev is not None:
            torch.cuda.current_stream(next(self.parameters()).device).wait_event(ev)

    def _score(self, call: _Call, prepared, training: bool, *params, feats=((), ())):
        call.owner = self
        call.input_roles, inputs = feats
        ev = self._params_ready
        if ev is not None:
            if prepared is None:                             # route "layers", the layer-by-layer entry point: staged
                call.params_ready, self._params_ready = ev, None
            else:
                self.wait_for_parameters()
        try:
            return _DrinScore.apply(call, prepared, training, *params, *inputs)
        except BaseException:
            # a staged call that failed before the library enqueued its wait (validation / workspace error) must not lose the
            # ordering behind the update still running on the side stream: the current stream waits here (harmless if the
            # library already did), so that whatever reads the parameters next reads them after Adam has written them
            if ev is not None:
                torch.cuda.current_stream(call.device).wait_event(ev)
            raise

    def _clamped(self, batch: "IndexedBatch") -> "IndexedBatch":
        """The batch with its candidate rows clamped into the tables and any clamped row reported in the status words like the
        kernels do (four small launches, no synchronisation: word 0 becomes 1, the value words stay 0): the torch gathers of
        the paths off the fused kernels must never see a row >= E (a device-side assert), a negative row wraps silently there,
        and the layer-by-layer kernels trust the index (only the stream kernel of the fused path clamps it) - a bad candidate
        row can never become an out-of-bounds read on the device."""
        cand = batch.candidates
        safe = cand.clamp(0, batch.table.num_entities - 1)
        self._status_words(cand.device)[0:1].bitwise_or_((safe != cand).any().view(1).to(torch.int32))
        return IndexedBatch(batch.mention, batch.table, safe, batch.miet_similarity, batch.mtei_similarity)

    @torch.no_grad()
    def _forward_cached(self, call: _Call, table: EntityTable, params) -> torch.Tensor:
        """Table-form inference from the per-entity cache (`drin_forward_cached`)."""
        lib = _lib.load()
        self.wait_for_parameters()
        _det, pc = call.param_struct(params)                      # `_det` lives to the end of the call: `pc` points into it
        pbuf = self._prepared.get(call, params, pc)
        cache = table._get_cache(call, (id(self._prepared), self._prepared.generation), pc, pbuf)
        ws, scores = call.byte_buffer(lib.drin_cached_workspace_bytes(C.byref(call.cfg))), call.scores()
        _lib.check(lib.drin_forward_cached(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), pbuf.data_ptr(),
                                           cache.data_ptr(), ws.data_ptr(), ws.numel(), scores.data_ptr(), call.stream()))
        return scores

    @torch.no_grad()
    def forward_traced(self, batch: Sequence[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Scores plus every stage's vertices and edges (tests / debugging)."""
        lib = _lib.load()
        self.wait_for_parameters()
        call = _Call(self.cfg, batch, self._unfused_precision())
        _det, pc = call.param_struct(_param_list(self))
        B, N, D, nl, dev = call.B, call.N, call.D, self.cfg.num_gcn_layers, call.device
        edge_shape = (4, B, N, D) if call.cfg.vector_edges else (4, B, N)
        tr = _lib.DrinTraceC()
        out: Dict[str, torch.Tensor] = {}
        for l in range(nl + 1):
            for field, key, shape in (("mention_text_vertex", f"mt{l}", (B, D)), ("mention_image_vertex", f"mi{l}", (B, D)),
                                      ("entity_text_vertex", f"et{l}", (B, N, D)), ("entity_image_vertex", f"ei{l}", (B, N, D)),
                                      ("edges", f"edges{l}", edge_shape)):
                t = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
                out[key] = t
                getattr(tr, field)[l] = t.data_ptr()
        ws, scores = call.workspace(False), call.scores()
        _lib.check(lib.drin_forward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(),
                                    scores.data_ptr(), 0, C.byref(tr), call.stream()))
        out["scores"] = scores
        return out
