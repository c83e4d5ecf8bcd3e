"""The reference's GHMFC baseline (`baselines/ghmfc.py`) on the HIP library, for scoring: `Model(nn.Module)` with the
reference's 52 state-dict keys and initialisation order, evaluated by `drin_ghmfc_forward`.

This is the default configuration of `common/args.py` for `model_type = "ghmfc"` (bidirectional cross-attention fusion with
a GELU gate for the mention, Linear for the entity, offline BERT features) in `eval()` mode, where the dropout inside the four
attentions is the identity.  This class scores only; `drin_amd.ghmfc_train.TrainableModel` derives from it and trains
(DESIGN.md section 18).  What is computed and how: section 15.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch
from torch import nn

from . import _lib
from ._lib import _ptr, _stream
from .ghmfc_table import GhmfcIndexedBatch, TableForm

PRECISIONS = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
ENTITY_FINAL_LAYERS = ("linear", "none")
ENTITY_POOLINGS = _lib.ENTITY_POOLINGS


@dataclass
class GhmfcConfig:
    """Geometry of `common/args.py` that GHMFC reads (`bert_embed_dim`, `resnet_embed_dim`, `resnet_num_region`,
    `max_mention_sentence_len`, `num_candidates_model`, `transformer_num_heads`, `max_entity_attr_token_len`).
    `entity_tokens` is the token count of the WikiMEL entity features [B, N, T, D] and ignored on WikiDiverse ([B, N, D]).
    `entity_final_layer_name` ("linear" | "none": `final_layer` is `nn.Identity`, the model has no entity keys) and
    `entity_final_pooling` ("avg" | "max" over tokens 1 : ntok - 1; read for token features only, as in the reference) are
    `common/args.py:15-16`; "bert default" is not offered: the reference's own `EntityEncoder.__init__` raises on it."""
    dataset_name: str = "wikidiverse"
    num_candidates: int = 11
    embed_dim: int = 768
    image_dim: int = 2048
    mention_tokens: int = 128
    image_regions: int = 49
    num_heads: int = 8
    entity_tokens: int = 64
    layer_norm_eps: float = 1e-5
    cosine_eps: float = 1e-8
    entity_final_layer_name: str = "linear"
    entity_final_pooling: str = "avg"

    def __post_init__(self):
        if self.dataset_name not in ("wikidiverse", "wikimel"):
            raise ValueError(f"dataset_name {self.dataset_name!r} is neither 'wikidiverse' nor 'wikimel'")
        if self.entity_final_layer_name not in ENTITY_FINAL_LAYERS:
            raise ValueError(f"entity_final_layer_name {self.entity_final_layer_name!r} is none of {ENTITY_FINAL_LAYERS}")
        if self.entity_final_pooling not in ENTITY_POOLINGS:
            raise ValueError(f"entity_final_pooling {self.entity_final_pooling!r} is none of {tuple(ENTITY_POOLINGS)} ('bert default': "
                             "the reference's EntityEncoder cannot be constructed with it)")

    @property
    def entity_default(self) -> bool:
        """Linear over the token mean: the entity side `drin_ghmfc_forward` runs"""
        return self.entity_final_layer_name == "linear" and self.entity_final_pooling == "avg"


def config_from_reference_args(args) -> GhmfcConfig:
    """GhmfcConfig from a `common.args` module (or any object with its names); refuses the variants that are not built."""
    want = dict(mention_final_layer_name="multimodal", mention_multimodal_attention="bi", multimodal_subspace_activation="gelu",
                entity_final_layer_name="linear", entity_final_pooling="avg", online_bert=False)
    for name, value in want.items():
        got = getattr(args, name, value)
        if got != value:
            raise NotImplementedError(f"ghmfc: {name} = {got!r} is not implemented (only {value!r}; DESIGN.md section 11)")
    D = args.bert_embed_dim
    for name in ("mention_final_output_dim", "entity_final_output_dim"):
        if getattr(args, name, D) != D:
            raise NotImplementedError(f"ghmfc: {name} = {getattr(args, name)} != bert_embed_dim = {D} is not implemented")
    return GhmfcConfig(dataset_name=args.dataset_name, num_candidates=args.num_candidates_model, embed_dim=D,
                       image_dim=args.resnet_embed_dim, mention_tokens=args.max_mention_sentence_len,
                       image_regions=args.resnet_num_region, num_heads=getattr(args, "transformer_num_heads", 8),
                       entity_tokens=getattr(args, "max_entity_attr_token_len", 64))


def entity_settings_from_reference_args(args) -> dict:
    """`entity_final_layer_name` and `entity_final_pooling` of a `common.args` module as `GhmfcConfig` fields, validated."""
    layer, pooling = getattr(args, "entity_final_layer_name", "linear"), getattr(args, "entity_final_pooling", "avg")
    if getattr(args, "online_bert", False):
        raise NotImplementedError("ghmfc: online_bert = True is not implemented (only the offline features; DESIGN.md section 11)")
    if pooling == "bert default":
        raise NotImplementedError("ghmfc: entity_final_pooling = 'bert default' is refused: the reference's own EntityEncoder constructor "
                                  "raises ValueError on it (get_entity_final_pooling_fn, baselines/ghmfc.py:253-260), so no model to agree "
                                  "with exists (DESIGN.md section 28)")
    if layer not in ENTITY_FINAL_LAYERS:
        raise NotImplementedError(f"ghmfc: entity_final_layer_name = {layer!r} is none of {ENTITY_FINAL_LAYERS}")
    if pooling not in ENTITY_POOLINGS:
        raise NotImplementedError(f"ghmfc: entity_final_pooling = {pooling!r} is none of {tuple(ENTITY_POOLINGS)}")
    return dict(entity_final_layer_name=layer, entity_final_pooling=pooling)


def model_device(model: nn.Module, *like) -> torch.device:
    """Where a GHMFC model lives: the device of its first parameter; a model without one (mention encoder "none" with entity
    "none") is where the first tensor of `like` is - the batch's mention features, or the table."""
    for p in model.parameters():
        return p.device
    for t in like:
        if isinstance(t, torch.Tensor):
            return t.device
    return torch.device("cpu")


class _CrossAttention(nn.Module):
    """Parameter container of ghmfc.py's CrossAttention(dim_a, dim_b): same modules, same order.  `attention`: the class (or
    a factory with nn.MultiheadAttention's arguments) of the two attentions - a subclass draws the same initial weights."""

    def __init__(self, dim_a: int, dim_b: int, heads: int, dropout: float = 0.1, attention=nn.MultiheadAttention):
        super().__init__()
        self.a2b_attention = attention(dim_a, heads, dropout, kdim=dim_b, vdim=dim_b, batch_first=True)
        self.a2b_ffn = nn.Linear(dim_a, dim_a)
        self.b2a_attention = attention(dim_a, heads, dropout, batch_first=True)
        self.b2a_ffn = nn.Linear(dim_a, dim_a)
        self.layernorms = nn.ModuleList([nn.LayerNorm(dim_a) for _ in range(4)])

    def param_list(self) -> list:
        a, b = self.a2b_attention, self.b2a_attention
        out = [a.q_proj_weight, a.k_proj_weight, a.v_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
               self.a2b_ffn.weight, self.a2b_ffn.bias, b.in_proj_weight, b.in_proj_bias, b.out_proj.weight, b.out_proj.bias,
               self.b2a_ffn.weight, self.b2a_ffn.bias]
        for ln in self.layernorms:
            out += [ln.weight, ln.bias]
        return out


class _MultimodalFusion(nn.Module):
    def __init__(self, cfg: GhmfcConfig, dropout: float = 0.1, attention=nn.MultiheadAttention):
        super().__init__()
        D, R = cfg.embed_dim, cfg.image_dim
        self.t2v_attention = _CrossAttention(D, R, cfg.num_heads, dropout, attention)
        self.v2t_attention = _CrossAttention(R, D, cfg.num_heads, dropout, attention)
        self.text_linear = nn.Linear(D, D)
        self.image_linear = nn.Linear(R, D)
        self.score_linear = nn.Linear(2 * D, 2)


class _MentionEncoder(nn.Module):
    def __init__(self, cfg: GhmfcConfig, dropout: float = 0.1, attention=nn.MultiheadAttention):
        super().__init__()
        self.intermediate_layer = _MultimodalFusion(cfg, dropout, attention)


class _EntityEncoder(nn.Module):
    def __init__(self, cfg: GhmfcConfig):
        super().__init__()
        # ghmfc.py:210-213: "none" constructs no Linear, so the draws that follow under one seed stay the reference's
        self.final_layer = nn.Linear(cfg.embed_dim, cfg.embed_dim) if cfg.entity_final_layer_name == "linear" else nn.Identity()

    def param_list(self) -> list:
        return list(self.final_layer.parameters())


class Model(TableForm, nn.Module):
    """ghmfc.py's `Model` for scoring: the same modules, created in the same order (so `torch.manual_seed(s); Model()` draws the
    reference's weights) and the same 52 state-dict keys (50 with `entity_final_layer_name = "none"`); a trained checkpoint loads with
    `load_state_dict`.  With non-default entity settings (`GhmfcConfig.entity_final_pooling`, `entity_final_layer_name`; DESIGN.md
    section 28) scoring is `drin_ghmfc_mention_forward` followed by `ghmfc_train.entity_scores`.
    `forward(batch)` takes the reference's 8-item offline batch (mention_feature, mention_mask, begin, end, mention_image,
    entity_feature, entity_mask, entity_image) and returns scores [B, N]; `encode_mentions(batch)` the [B, D] mention
    representations.  Eval mode only, no gradients.  `precision`: "bf16x3" (split-bf16 products, the default) or "f32"
    (exact fp32 MFMA); attention, LayerNorm and the gate are fp32 FMA in both.
    The table form (`drin_amd.ghmfc_table.TableForm`): a `GhmfcIndexedBatch`, or - after
    `attach_entity_table(table)` - an 8-item batch whose item 5 is the integer tensor `[B, N]` of candidate rows, is scored by
    `drin_ghmfc_forward_table` with the bits of the gathered batch; `enable_entity_cache()` scores against per-entity rows."""

    def __init__(self, cfg: GhmfcConfig | None = None, precision: str = "bf16x3"):
        super().__init__()
        cfg = cfg or GhmfcConfig()
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r} not in {sorted(PRECISIONS)}")
        self.cfg, self.precision = cfg, precision
        self.mention_encoder = self._make_mention_encoder(cfg)
        self.entity_encoder = _EntityEncoder(cfg)

    def _make_mention_encoder(self, cfg: GhmfcConfig) -> nn.Module:
        return _MentionEncoder(cfg)

    def param_list(self) -> list:
        """The parameters in drin_ghmfc_params (= state-dict) order: 52, or 50 when the entity final layer is "none"."""
        f = self.mention_encoder.intermediate_layer
        return (f.t2v_attention.param_list() + f.v2t_attention.param_list()
                + [f.text_linear.weight, f.text_linear.bias, f.image_linear.weight, f.image_linear.bias, f.score_linear.weight,
                   f.score_linear.bias] + self.entity_encoder.param_list())

    def _params_c(self):
        """(drin_ghmfc_params, the tensors it points into).  Without an entity Linear its two slots hold text_linear's pointers:
        valid addresses that only `drin_ghmfc_mention_forward` is given, which reads neither."""
        params = [p.detach().contiguous() for p in self.param_list()]
        params += params[44:46] if len(params) == 50 else []
        return _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[p.data_ptr() for p in params])), params

    def _batch_tensors(self, batch):
        """(mention_feature, mention_mask, mention_image, entity_feature, entity_mask or None, entity tokens or 0) of the
        reference's batch: detached, float32 / int64, contiguous, on the model's device, checked against the configuration."""
        mf, mmask, _begin, _end, mimage, ef, emask = batch[:7]
        dev = model_device(self, mf)
        if dev.type != "cuda" or (isinstance(mf, torch.Tensor) and mf.device.type != "cuda"):
            raise RuntimeError("drin_amd.ghmfc.Model runs on the GPU only (no CPU fallback): move the model and the batch with .cuda()")
        cfg = self.cfg
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()          # noqa: E731
        mf, mimage, ef = f(mf), f(mimage), f(ef)
        mmask = torch.as_tensor(mmask).to(dev, torch.int64).contiguous()
        B = mf.shape[0]
        tokens = 0
        if ef.dim() == 4:                                                      # WikiMEL: [B, N, T, D] + entity_mask [B, N, T]
            tokens = ef.shape[2]
            emask = torch.as_tensor(emask).to(dev, torch.int64).contiguous()
            if tuple(emask.shape) != tuple(ef.shape[:3]):
                raise ValueError(f"entity_mask {tuple(emask.shape)} does not match entity_feature {tuple(ef.shape)}")
        else:
            emask = None
        want = (B, cfg.mention_tokens, cfg.embed_dim), (B, cfg.mention_tokens), (B, cfg.image_regions, cfg.image_dim)
        got = tuple(mf.shape), tuple(mmask.shape), tuple(mimage.shape)
        if got != want or tuple(ef.shape[:2]) != (B, cfg.num_candidates) or ef.shape[-1] != cfg.embed_dim:
            raise ValueError(f"ghmfc batch shapes {got}, entity_feature {tuple(ef.shape)} do not match the configuration {cfg}")
        return mf, mmask, mimage, ef, emask, tokens

    def _mention_tensors(self, mention):
        """(mention_feature, mention_mask, mention_image) of the five mention-side items of a table-form batch, prepared and
        checked like `_batch_tensors`' (begin and end are not read)."""
        mf, mmask, _begin, _end, mimage = mention
        dev = model_device(self, mf)
        if dev.type != "cuda" or (isinstance(mf, torch.Tensor) and mf.device.type != "cuda"):
            raise RuntimeError("drin_amd.ghmfc.Model runs on the GPU only (no CPU fallback): move the model and the batch with .cuda()")
        cfg = self.cfg
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()          # noqa: E731
        mf, mimage = f(mf), f(mimage)
        mmask = torch.as_tensor(mmask).to(dev, torch.int64).contiguous()
        B = mf.shape[0]
        want = (B, cfg.mention_tokens, cfg.embed_dim), (B, cfg.mention_tokens), (B, cfg.image_regions, cfg.image_dim)
        got = tuple(mf.shape), tuple(mmask.shape), tuple(mimage.shape)
        if got != want:
            raise ValueError(f"ghmfc batch shapes {got} do not match the configuration {cfg}")
        return mf, mmask, mimage

    def _score_table(self, tb: GhmfcIndexedBatch, want_scores: bool):
        """`_score` of a table-form batch: `drin_ghmfc_forward_table`, from the cached per-entity rows when enabled."""
        mf, mmask, mimage = self._mention_tensors(tb.mention)
        cfg, dev, B = self.cfg, mf.device, mf.shape[0]
        if tb.candidates.shape[0] != B:
            raise ValueError(f"ghmfc table form: candidates {tuple(tb.candidates.shape)} for {B} mentions")
        if not cfg.entity_default:              # the mention half's own bits, then the entity side as the variants run it
            with torch.no_grad():
                mention = self._mention_only(tb.mention)
                return self._eval_scores(tb, mention) if want_scores else mention
        lib = _lib.load()
        text = tb.table.text.contiguous()
        tokens = text.shape[1] if text.dim() == 3 else 0
        mask = tb.table.mask.to(torch.int64).contiguous() if tokens else None
        rows = self._entity_rows(tb.table) if (self._tf.cache_on and want_scores) else None
        c = _lib.DrinGhmfcConfigC(batch=B, num_candidates=cfg.num_candidates, embed_dim=cfg.embed_dim, image_dim=cfg.image_dim,
                                  mention_tokens=cfg.mention_tokens, image_regions=cfg.image_regions, num_heads=cfg.num_heads,
                                  entity_tokens=tokens, precision=PRECISIONS[self.precision], layer_norm_eps=cfg.layer_norm_eps,
                                  cosine_eps=cfg.cosine_eps)
        pc, _params = self._params_c()
        bt = _lib.DrinGhmfcBatchC(_ptr(mf), _ptr(mmask), _ptr(mimage), None, None)
        status = self._status_words(dev)
        tc = _lib.DrinGhmfcTableC(size=C.sizeof(_lib.DrinGhmfcTableC), text=_ptr(text), mask=_ptr(mask), num_entities=text.shape[0],
                                  entity_tokens=tokens, candidates=_ptr(tb.candidates), index_status=_ptr(status), rows=_ptr(rows))
        nbytes = lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(tc))
        if nbytes == 0:
            _lib.check(_lib.E_SHAPE)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        scores = torch.empty(B, cfg.num_candidates, dtype=torch.float32, device=dev)
        mention = torch.empty(B, cfg.embed_dim, dtype=torch.float32, device=dev)
        _lib.check(lib.drin_ghmfc_forward_table(C.byref(c), C.byref(bt), C.byref(pc), C.byref(tc), _ptr(ws), nbytes, _ptr(scores),
                                                _ptr(mention), _stream(dev)))
        self._watch_indices(dev)
        return scores if want_scores else mention

    def _mention_only(self, mention) -> torch.Tensor:
        """`[B, D]` mention representations from the five mention-side items alone (`drin_ghmfc_mention_forward`: the mention
        half of `drin_ghmfc_forward`, its bits) - what `link` ranks the table with."""
        mf, mmask, mimage = self._mention_tensors(mention)
        cfg, dev, B = self.cfg, mf.device, mf.shape[0]
        lib = _lib.load()
        c = _lib.DrinGhmfcConfigC(batch=B, num_candidates=cfg.num_candidates, embed_dim=cfg.embed_dim, image_dim=cfg.image_dim,
                                  mention_tokens=cfg.mention_tokens, image_regions=cfg.image_regions, num_heads=cfg.num_heads,
                                  entity_tokens=0, precision=PRECISIONS[self.precision], layer_norm_eps=cfg.layer_norm_eps,
                                  cosine_eps=cfg.cosine_eps)
        pc, _params = self._params_c()
        bt = _lib.DrinGhmfcBatchC(_ptr(mf), _ptr(mmask), _ptr(mimage), None, None)
        nbytes = lib.drin_ghmfc_mention_forward_workspace_bytes(C.byref(c))
        if nbytes == 0:
            _lib.check(_lib.E_SHAPE)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mention_repr = torch.empty(B, cfg.embed_dim, dtype=torch.float32, device=dev)
        _lib.check(lib.drin_ghmfc_mention_forward(C.byref(c), C.byref(bt), C.byref(pc), _ptr(ws), nbytes, _ptr(mention_repr), _stream(dev)))
        return mention_repr

    def _run(self, batch, want_scores: bool):
        if self.training:
            raise RuntimeError("drin_amd.ghmfc.Model is scoring only: call .eval(); GHMFC training is not implemented, DESIGN.md §11")
        return self._score(batch, want_scores)

    def _score(self, batch, want_scores: bool):
        tb = self._table_form(batch)
        if tb is not None:
            return self._score_table(tb, want_scores)
        mf, mmask, mimage, ef, emask, tokens = self._batch_tensors(batch)
        cfg, dev, B = self.cfg, mf.device, mf.shape[0]
        if not cfg.entity_default:              # drin_ghmfc_mention_forward, then the entity side operation by operation
            from .ghmfc_train import entity_scores
            with torch.no_grad():
                mention = self._mention_only([mf, mmask, None, None, mimage])
                return entity_scores(mention, ef, emask, self.entity_encoder.final_layer, cfg, self.precision) if want_scores else mention
        lib = _lib.load()
        c = _lib.DrinGhmfcConfigC(batch=B, num_candidates=cfg.num_candidates, embed_dim=cfg.embed_dim, image_dim=cfg.image_dim,
                                  mention_tokens=cfg.mention_tokens, image_regions=cfg.image_regions, num_heads=cfg.num_heads,
                                  entity_tokens=tokens, precision=PRECISIONS[self.precision], layer_norm_eps=cfg.layer_norm_eps,
                                  cosine_eps=cfg.cosine_eps)
        pc, _params = self._params_c()
        bt = _lib.DrinGhmfcBatchC(_ptr(mf), _ptr(mmask), _ptr(mimage), _ptr(ef), _ptr(emask))
        nbytes = lib.drin_ghmfc_workspace_bytes(C.byref(c))
        if nbytes == 0:
            _lib.check(_lib.E_SHAPE)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        scores = torch.empty(B, cfg.num_candidates, dtype=torch.float32, device=dev)
        mention = torch.empty(B, cfg.embed_dim, dtype=torch.float32, device=dev)
        _lib.check(lib.drin_ghmfc_forward(C.byref(c), C.byref(bt), C.byref(pc), _ptr(ws), nbytes, _ptr(scores), _ptr(mention),
                                          _stream(dev)))
        return scores if want_scores else mention

    def forward(self, batch) -> torch.Tensor:
        return self._run(batch, True)

    def encode_mentions(self, batch) -> torch.Tensor:
        return self._run(batch, False)
