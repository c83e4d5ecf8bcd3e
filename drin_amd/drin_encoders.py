"""DRIN with its other mention-text encoders (`common/args.py:28-29`: `mention_final_layer_name` "transformer" | "none",
`mention_final_representation` "avg extract" | "max pool"; `baselines/ghmfc.py:152-199` with `inline_bert=False`,
`drin/model.py:21,58,71-76`) on the HIP library.  `Model(cfg)` returns an `EncoderModel` for such a configuration; the linear
encoder - the default - stays `drin_amd.model.Model`.

The mention-text vertex is `repr(intermediate(mention_text))` with no Linear behind it and the text-text edge takes
`repr(mention_text)` of the RAW block; `repr` is the mean over the mention span or the max over all L positions.  The
intermediate layer of "transformer" is `ghmfc_variants.transformer_stack` (the composition GHMFC's encoder runs); the two `repr`
rows, the GCN and the score run behind `drin_forward_staged_head` / `drin_backward_head`, one autograd edge that has the encoded
block as an input.  What the kernels compute and what is not built: DESIGN.md section 22.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch
from torch import nn

from . import _lib
from .attention import DropoutStream
from .config import DrinConfig
from .ghmfc_train import check_setup
from .ghmfc_variants import transformer_stack
from .model import (_INPUT_FIELDS, IndexedBatch, Model, _batch_requires_grad, _Call, _dead_param_indices, _feature_inputs, _fill_params,
                    _split_mentions)

NOT_BUILT = "is not built for the transformer / none mention encoders (DESIGN.md section 22, 'not done')"
_PRECISION_NAMES = {_lib.PREC_F32: "f32", _lib.PREC_BF16X3: "bf16x3"}


class MultilayerTransformer(nn.Module):
    """Parameter container of ghmfc.py:72-90: torch's own encoder, so the 12 keys per layer under
    `...intermediate_layer.transformer.layers.{i}.` and the initial draw (one layer drawn, then deep-copied) are torch's.  Its
    `forward` is never called: `EncoderModel` runs the layers on the library."""

    def __init__(self, cfg: DrinConfig):
        super().__init__()
        layer = nn.TransformerEncoderLayer(cfg.bert_embed_dim, cfg.transformer_num_heads, cfg.transformer_ffn_hidden_size,
                                           cfg.transformer_dropout, cfg.transformer_ffn_activation, batch_first=True)
        self.transformer = nn.TransformerEncoder(layer, cfg.transformer_num_layers, enable_nested_tensor=False)

    def forward(self, *args, **kwargs):
        raise RuntimeError("drin_amd.drin_encoders: torch's TransformerEncoder holds the parameters only; EncoderModel runs them")


def _gcn_params(model: "EncoderModel") -> List[torch.Tensor]:
    """The 22 (+ 2 per layer with vector edges) tensors of the C structs in `_fill_params` order, without the mention-text
    Linear this model does not have."""
    ve = model.vertex_encoder
    ps = [ve.entity_text_encoder.final_layer.weight, ve.entity_text_encoder.final_layer.bias, ve.mention_image_linear.weight,
          ve.mention_image_linear.bias, ve.entity_image_linear.weight, ve.entity_image_linear.bias]
    for layer in model.gcn_layers:
        ps += [layer.w_h.weight, layer.w_h.bias, layer.w_u.weight, layer.w_u.bias, layer.w_v.weight, layer.w_v.bias,
               layer.layer_norm.weight, layer.layer_norm.bias]
        if hasattr(layer, "w_m"):
            ps += [layer.w_m.weight, layer.w_m.bias]
    return ps


def _head_struct(model: "EncoderModel", call: _Call, enc: Optional[torch.Tensor]):
    """`(drin_mention_head, max positions [2, B, D] int32 or None)` of one call; `enc`: the encoded block as the library reads it."""
    head = _lib.DrinMentionHeadC()
    head.struct_size, head.encoder = C.sizeof(head), _lib.MENTION_ROWS
    head.representation = _lib.MENTION_REPR[model.cfg.mention_final_representation]
    head.encoded = None if enc is None else enc.data_ptr()
    idx = None
    if head.representation == _lib.REPR_MAX_POOL:
        idx = torch.empty(2, call.B, call.D, dtype=torch.int32, device=call.device)
        head.max_index = idx.data_ptr()
    return head, idx


def _param_struct(call: _Call, params: Sequence[torch.Tensor]):
    """`(tensors, drin_params)` with the mention-text Linear's two pointers NULL (never read under DRIN_MENTION_ROWS)."""
    tensors = tuple(p.detach().contiguous() for p in params)
    pc = _lib.DrinParamsC()
    _fill_params(pc, (None, None) + tensors, call.per_layer)
    return tensors, pc


class _HeadScore(torch.autograd.Function):
    """Autograd edge around drin_forward_staged_head / drin_backward_head.  Inputs: the encoded block (or None: the raw block
    itself), the GCN's parameters, then the batch tensors that require grad (`call.input_roles`, drin_input_grads fields)."""

    @staticmethod
    def forward(ctx, call: _Call, model: "EncoderModel", training: bool, encoded: Optional[torch.Tensor], *tensors: torch.Tensor):
        lib = _lib.load()
        ctx.roles = call.input_roles
        params, pc = _param_struct(call, tensors[:len(tensors) - len(ctx.roles)])
        enc = None if encoded is None else encoded.detach().contiguous()
        head, idx = _head_struct(model, call, enc)
        ws, scores = call.workspace(training), call.scores()
        _lib.check(lib.drin_forward_staged_head(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(),
                                                scores.data_ptr(), 1 if training else 0, None, None, C.byref(head), call.stream()))
        model.max_indices = {} if idx is None else {"edge": idx[0], "text": idx[1]}
        ctx.call, ctx.ws, ctx.pc, ctx.params, ctx.enc, ctx.idx, ctx.head = call, ws, pc, params, enc, idx, head
        return scores

    @staticmethod
    def backward(ctx, grad_scores: torch.Tensor):
        lib = _lib.load()
        call, params, roles, head = ctx.call, ctx.params, ctx.roles, ctx.head
        dev = call.device
        need_enc = ctx.enc is not None and ctx.needs_input_grad[3]
        need_params = ctx.needs_input_grad[4:4 + len(params)]
        needs = ctx.needs_input_grad[4 + len(params):]
        need_feats = [r for r, n in zip(roles, needs) if n]
        gc, out = None, [None] * len(params)
        if any(need_params):
            grads = [torch.empty_like(p) for p in params]
            torch._foreach_zero_(grads)
            gc = _lib.DrinParamGradsC()
            _fill_params(gc, [None, None] + grads, call.per_layer)
            out = list(grads)
            # parameters the score does not depend on get no gradient at all in the reference (.grad is None)
            for i in _dead_param_indices(len(params) + 2, call.per_layer, bool(call.cfg.dynamic_edges)):
                out[i - 2] = None
        ig, feat_out = None, {}
        if need_feats:
            ig = _lib.DrinInputGradsC()
            for role in need_feats:
                feat_out[role] = torch.empty(call.keep[_INPUT_FIELDS[role]].shape, dtype=torch.float32, device=dev)
                setattr(ig, role, feat_out[role].data_ptr())
            scratch = call.byte_buffer(lib.drin_input_grad_scratch_bytes(C.byref(call.cfg)))
            ig.scratch, ig.scratch_bytes = scratch.data_ptr(), scratch.numel()
        g_enc = torch.empty_like(ctx.enc) if need_enc else None
        head.grad_encoded = None if g_enc is None else g_enc.data_ptr()
        g = grad_scores.to(torch.float32).contiguous()
        _lib.check(lib.drin_backward_head(C.byref(call.cfg), C.byref(call.batch), C.byref(ctx.pc), ctx.ws.data_ptr(), ctx.ws.numel(),
                                          g.data_ptr(), None if gc is None else C.byref(gc), None if ig is None else C.byref(ig), None,
                                          C.byref(head), call.stream()))
        feats = [feat_out.get(role) if n else None for role, n in zip(roles, needs)]
        return (None, None, None, g_enc, *out, *feats)


class EncoderModel(Model):
    """`drin/model.py`'s `Model` with `mention_final_layer_name` "transformer" or "none": the reference's modules under the
    reference's names, created in the reference's order (the same state-dict keys and the same initial draw under one
    `torch.manual_seed`; a reference checkpoint loads).

    `forward(batch)` takes the reference's 14-tuple; item 1 (`mention_text_mask`) is read by "transformer"
    (`src_key_padding_mask = mask == 0`).  `train()`: gradients reach every parameter and every float batch tensor that
    requires one; with `transformer_dropout > 0` every transformer layer takes four draws from the model's one
    `DropoutStream(seed)` in `transformer_stack`'s order.  `eval()`: the same composition under `no_grad`, no dropout.  After
    a max-pool forward `max_indices == {"edge": idx, "text": idx}` (int32 [B, D]): the lowest position that attains each maximum
    of the raw block (the text-text edge's row) and of the encoded block (the vertex), over ALL L positions - padded ones take
    part, as in the reference.  `core`: the softmax-attention core of the transformer, "fma" or "mfma".

    A call in which nothing requires a gradient takes the folded two-layer path (`drin_forward_prepared_head`) where
    `Model._route` would take it for the linear model - `fused=True` and a geometry `drin_fused_supported` accepts - else the
    layer-by-layer entry points; `last_path` says which ("prepared" | "layers").  Batch features stored as bf16 are widened to
    fp32.  Not built, each refused with `NotImplementedError`: `IndexedBatch` / `EntityTable`, the per-entity cache,
    `grad_bucket` views, `flatten_parameters`, `LibraryAdam`'s flat form, and - in `drin_amd.train` - `OverlappedStep` and
    `GradBucket(overlap=True)`.  `max_indices` covers the whole batch also when it was scored in slices."""

    flat_buckets = False

    def __init__(self, cfg: DrinConfig, precision: str = "bf16x3", fused: bool = True, grad_bucket: bool = False, core: str = "fma",
                 seed: int = 0):
        super().__init__(cfg, precision=precision, fused=fused, grad_bucket=False)
        if self.cfg.linear_mention_encoder:
            raise ValueError("EncoderModel is the transformer / none mention encoder; the linear one is drin_amd.model.Model")
        if self.precision not in _PRECISION_NAMES:
            raise NotImplementedError(f"precision {precision!r}: the inference-only modes belong to the folded path, which {NOT_BUILT}")
        self.dropout = check_setup(_PRECISION_NAMES[self.precision], core, self.cfg.transformer_dropout)
        self.core = core
        self.dropout_stream = DropoutStream(seed)
        self.max_indices = {}
        self.last_path = None

    # ---- what the flat buckets of the linear model would need: refused ----------------------------------------------------
    def bucket_layout(self):
        raise NotImplementedError(f"Model.bucket_layout (the flat parameter / gradient buckets) {NOT_BUILT}")

    def flatten_parameters(self):
        raise NotImplementedError(f"Model.flatten_parameters (LibraryAdam's flat form, bench.py --gpus) {NOT_BUILT}")

    def grad_bucket(self):
        raise NotImplementedError(f"Model.grad_bucket (gradient bucket views, OverlappedStep) {NOT_BUILT}")

    def attribute(self, batch, candidate=None, weights=None):
        raise NotImplementedError("Model.attribute (gradient x input attribution) under a transformer / none mention encoder is out of "
                                  "scope of DESIGN.md section 31: the linear mention encoder only")

    def link(self, *args, **kwargs):
        raise NotImplementedError(f"Model.link (table-form batches: IndexedBatch / EntityTable behind a first stage) {NOT_BUILT}")

    # ---- the forward -----------------------------------------------------------------------------------------------------
    def forward(self, batch) -> torch.Tensor:
        if isinstance(batch, IndexedBatch):
            raise NotImplementedError(f"IndexedBatch / EntityTable / DeviceSplit (table-form batches, the per-entity cache) {NOT_BUILT}")
        if not self.training:
            with torch.no_grad():
                return self._slices(batch)
        return self._slices(batch)

    def _slices(self, batch) -> torch.Tensor:
        if batch[0].shape[0] > self.MAX_CALL_MENTIONS:
            scores, positions = [], []
            for part in _split_mentions(batch, self.MAX_CALL_MENTIONS):
                scores.append(self._compose(part))
                positions.append(self.max_indices)
            self.max_indices = {k: torch.cat([p[k] for p in positions], 0) for k in positions[0]}   # of the whole batch, [B, D]
            return torch.cat(scores, 0)
        return self._compose(batch)

    def _encode(self, mention_text: torch.Tensor, mask: torch.Tensor) -> Optional[torch.Tensor]:
        """The intermediate layer's output [B, L, D], or None where it is the Identity ("none")."""
        cfg = self.cfg
        if cfg.mention_final_layer_name != "transformer":
            return None
        mask = torch.as_tensor(mask).to(mention_text.device)
        if tuple(mask.shape) != tuple(mention_text.shape[:2]):
            raise ValueError(f"mention_text_mask has shape {tuple(mask.shape)}, expected {tuple(mention_text.shape[:2])}")
        return transformer_stack(self.vertex_encoder.mention_text_encoder.intermediate_layer.transformer.layers, mention_text, mask == 0,
                                 num_heads=cfg.transformer_num_heads, ffn_hidden_size=cfg.transformer_ffn_hidden_size,
                                 ffn_activation=cfg.transformer_ffn_activation, precision=_PRECISION_NAMES[self.precision], core=self.core,
                                 dropout=self.dropout if self.training else 0.0, dropout_stream=self.dropout_stream)

    def _compose(self, batch: Sequence[torch.Tensor]) -> torch.Tensor:
        self.wait_for_parameters()
        call = _Call(self.cfg, batch, self.precision)
        self.max_indices = {}
        if call.B == 0:
            return call.scores()
        params = _gcn_params(self)
        grad = torch.is_grad_enabled()
        training = grad and (_batch_requires_grad(batch) or any(p.requires_grad for p in self.parameters()))
        encoded = self._encode(call.keep[0], batch[1])                 # call.keep[0]: mention_text as the library reads it (fp32)
        if not training and self._prepared is not None and _lib.load().drin_fused_supported(C.byref(call.cfg)) == _lib.OK:
            self.last_path = "prepared"
            return self._score_folded(call, params, encoded)
        self.last_path = "layers"
        call.owner = self
        call.input_roles, inputs = _feature_inputs(call) if training else ((), ())
        return _HeadScore.apply(call, self, training, encoded, *params, *inputs)

    @torch.no_grad()
    def _score_folded(self, call: _Call, params: Sequence[torch.Tensor], encoded: Optional[torch.Tensor]) -> torch.Tensor:
        """Inference on the folded two-layer path: weights folded once per weight version (`drin_prepare`, which skips the
        mention-text Linear's plane), the head as `k_mention_rows` and the mention-image product alone."""
        lib = _lib.load()
        _tensors, pc = _param_struct(call, params)                     # `_tensors` lives to the end of the call: `pc` points into it
        pbuf = self._prepared.get(call, params, pc)
        enc = None if encoded is None else encoded.detach().contiguous()
        head, idx = _head_struct(self, call, enc)
        ws, scores = call.byte_buffer(lib.drin_fused_workspace_bytes(C.byref(call.cfg))), call.scores()
        _lib.check(lib.drin_forward_prepared_head(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), pbuf.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), scores.data_ptr(), C.byref(head), call.stream()))
        self.max_indices = {} if idx is None else {"edge": idx[0], "text": idx[1]}
        return scores

    @torch.no_grad()
    def forward_traced(self, batch: Sequence[torch.Tensor]):
        """Scores plus every stage's vertices and edges, as `Model.forward_traced` (no dropout, whatever the mode)."""
        lib = _lib.load()
        self.wait_for_parameters()
        call = _Call(self.cfg, batch, self.precision)
        was_training = self.training
        self.training = False
        try:
            enc = self._encode(call.keep[0], batch[1])
        finally:
            self.training = was_training
        _tensors, pc = _param_struct(call, _gcn_params(self))
        B, N, D, nl, dev = call.B, call.N, call.D, self.cfg.num_gcn_layers, call.device
        enc = None if enc is None else enc.detach().contiguous()
        head, _idx = _head_struct(self, call, enc)
        edge_shape = (4, B, N, D) if call.cfg.vector_edges else (4, B, N)
        tr, out = _lib.DrinTraceC(), {}
        for l in range(nl + 1):
            for field, key, shape in (("mention_text_vertex", f"mt{l}", (B, D)), ("mention_image_vertex", f"mi{l}", (B, D)),
                                      ("entity_text_vertex", f"et{l}", (B, N, D)), ("entity_image_vertex", f"ei{l}", (B, N, D)),
                                      ("edges", f"edges{l}", edge_shape)):
                out[key] = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
                getattr(tr, field)[l] = out[key].data_ptr()
        ws, scores = call.workspace(False), call.scores()
        _lib.check(lib.drin_forward_staged_head(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(),
                                                scores.data_ptr(), 0, C.byref(tr), None, C.byref(head), call.stream()))
        out["scores"] = scores
        return out
