"""GHMFC's other mention encoders (`baselines/ghmfc.py:152-199`, selected by `common/args.py:11-19`) on the HIP library, for
scoring and training: `"transformer"` (eight post-norm `nn.TransformerEncoderLayer`s over the mention sentence), `"multimodal"`
with `mention_multimodal_attention = "text"` (one `CrossAttention(text, image)`), `"linear"` (`AvgLinear`) and `"none"`, each
followed by the max over all positions or the mean over the mention span.  The default (`"multimodal"`, `"bi"`) stays
`drin_amd.ghmfc_train.TrainableModel`.

The forward is composed operation by operation from the library's differentiable functions (`drin_amd.attention`,
`drin_amd.row_ops`): every one a HIP kernel pair, no torch math between the batch and the scores.  What the kernels compute,
the dropout draws and the measured errors: DESIGN.md section 20.
"""
from __future__ import annotations

from dataclasses import dataclass, fields

import torch
from torch import nn

from .attention import PRECISIONS, DropoutStream, _linear, multihead_attention_forward
from .ghmfc import GhmfcConfig, _CrossAttention, _EntityEncoder, model_device
from .ghmfc_table import TableForm
from .ghmfc_train import TrainableModel, attention_factory, check_setup, cross_attention, entity_scores
from .row_ops import act_dropout, layer_norm_res, seq_max, span_mean

FINAL_LAYERS = ("multimodal", "transformer", "linear", "none")
ATTENTIONS = ("bi", "text")
REPRESENTATIONS = ("max pool", "avg extract")
FFN_ACTIVATIONS = ("gelu", "relu")


@dataclass
class VariantConfig(GhmfcConfig):
    """`GhmfcConfig` plus the names of `common/args.py` that select the mention encoder (`mention_final_layer_name`,
    `mention_multimodal_attention`, `mention_final_representation`) and the transformer's geometry (`transformer_num_layers`,
    `transformer_ffn_hidden_size`, `transformer_ffn_activation`).  The forcing rule of `args.py:12` is applied: `"linear"`
    implies "avg extract", `"multimodal"` with `"bi"` implies "max pool"."""
    mention_final_layer_name: str = "multimodal"
    mention_multimodal_attention: str = "bi"
    mention_final_representation: str = "max pool"
    transformer_num_layers: int = 8
    transformer_ffn_hidden_size: int = 512
    transformer_ffn_activation: str = "gelu"

    def __post_init__(self):
        super().__post_init__()
        for name, allowed in (("mention_final_layer_name", FINAL_LAYERS), ("mention_multimodal_attention", ATTENTIONS),
                              ("mention_final_representation", REPRESENTATIONS), ("transformer_ffn_activation", FFN_ACTIVATIONS)):
            if getattr(self, name) not in allowed:
                raise ValueError(f"{name} {getattr(self, name)!r} is none of {allowed}")
        if self.mention_final_layer_name == "linear":
            self.mention_final_representation = "avg extract"
        elif self.is_default:
            self.mention_final_representation = "max pool"
        if self.mention_final_layer_name == "transformer" and (
                self.transformer_num_layers < 1 or self.transformer_ffn_hidden_size < 4 or self.transformer_ffn_hidden_size % 4):
            raise ValueError(f"transformer_num_layers {self.transformer_num_layers} must be >= 1 and transformer_ffn_hidden_size "
                             f"{self.transformer_ffn_hidden_size} a positive multiple of 4")

    @property
    def is_default(self) -> bool:
        """the `model_type == "ghmfc"` default: bidirectional fusion, `TrainableModel`'s"""
        return self.mention_final_layer_name == "multimodal" and self.mention_multimodal_attention == "bi"

    @property
    def reads_mention_image(self) -> bool:
        return self.mention_final_layer_name == "multimodal"

    def base(self) -> GhmfcConfig:
        return GhmfcConfig(**{f.name: getattr(self, f.name) for f in fields(GhmfcConfig)})


def variant_config_from_reference_args(args) -> VariantConfig:
    """VariantConfig from a `common.args` module (or any object with its names); refuses what is not built."""
    want = dict(entity_final_layer_name="linear", entity_final_pooling="avg", online_bert=False)
    for name, value in want.items():
        got = getattr(args, name, value)
        if got != value:
            raise NotImplementedError(f"ghmfc: {name} = {got!r} is not implemented (only {value!r}; DESIGN.md section 11)")
    D = args.bert_embed_dim
    for name in ("mention_final_output_dim", "entity_final_output_dim"):
        if getattr(args, name, D) != D:
            raise NotImplementedError(f"ghmfc: {name} = {getattr(args, name)} != bert_embed_dim = {D} is not implemented")
    cfg = VariantConfig(dataset_name=args.dataset_name, num_candidates=args.num_candidates_model, embed_dim=D,
                        image_dim=args.resnet_embed_dim, mention_tokens=args.max_mention_sentence_len,
                        image_regions=args.resnet_num_region, num_heads=getattr(args, "transformer_num_heads", 8),
                        entity_tokens=getattr(args, "max_entity_attr_token_len", 64),
                        mention_final_layer_name=getattr(args, "mention_final_layer_name", "multimodal"),
                        mention_multimodal_attention=getattr(args, "mention_multimodal_attention", "bi"),
                        mention_final_representation=getattr(args, "mention_final_representation", "max pool"),
                        transformer_num_layers=getattr(args, "transformer_num_layers", 8),
                        transformer_ffn_hidden_size=getattr(args, "transformer_ffn_hidden_size", 512),
                        transformer_ffn_activation=getattr(args, "transformer_ffn_activation", "gelu"))
    if cfg.is_default and getattr(args, "multimodal_subspace_activation", "gelu") != "gelu":
        raise NotImplementedError(f"ghmfc: multimodal_subspace_activation = {args.multimodal_subspace_activation!r} is not implemented "
                                  "(only 'gelu'; DESIGN.md section 11)")
    return cfg


def transformer_stack(layers, x, padding, *, num_heads: int, ffn_hidden_size: int, ffn_activation: str, precision: str, core: str,
                      dropout: float, dropout_stream: DropoutStream):
    """nn.TransformerEncoder(x, src_key_padding_mask=padding) over the `layers` of torch's own encoder (the parameter container):
    post-norm layers, no final norm (ghmfc.py:75-90), composed from the library's differentiable functions.  x [B, L, D] fp32 on
    the GPU, padding [B, L] bool (True = drop the key).  `dropout` > 0 (the caller passes 0 outside training): every layer takes
    four draws from `dropout_stream` in the order attention weights, drop1 (on the attention output), drop (on the activated FFN
    hidden rows), drop2 (on the FFN output), layers ascending.  Shared by `VariantModel` (GHMFC's "transformer" encoder) and
    `drin_amd.drin_encoders.EncoderModel` (DRIN's)."""
    prec = PRECISIONS[precision]
    B, L, D = x.shape
    rows = B * L

    def drop(width: int):
        """(p, seed, call) of the next row draw, or None when nothing is dropped"""
        return (dropout, dropout_stream.seed, dropout_stream.draw_rows(rows, width)) if dropout > 0 else None
    for layer in layers:
        sa = layer.self_attn
        a = multihead_attention_forward(
            x, x, x, padding, embed_dim=D, num_heads=num_heads, kdim=D, vdim=D, in_proj_weight=sa.in_proj_weight,
            q_proj_weight=None, k_proj_weight=None, v_proj_weight=None, in_proj_bias=sa.in_proj_bias,
            out_proj_weight=sa.out_proj.weight, out_proj_bias=sa.out_proj.bias, precision=precision, dropout=dropout,
            dropout_stream=dropout_stream, core=core)
        drop1 = drop(D)
        if drop1 is not None:
            a = act_dropout(a, "none", drop1)
        x = layer_norm_res(a, x, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
        h = _linear(x.view(rows, D), layer.linear1.weight, layer.linear1.bias, prec)
        h = act_dropout(h, ffn_activation, drop(ffn_hidden_size))
        h = _linear(h, layer.linear2.weight, layer.linear2.bias, prec)
        drop2 = drop(D)
        if drop2 is not None:
            h = act_dropout(h, "none", drop2)
        x = layer_norm_res(h.view(B, L, D), x, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)
    return x


class _MultilayerTransformer(nn.Module):
    """Parameter container of ghmfc.py's MultilayerTransformer: torch's own encoder, so the 12 keys per layer and the initial
    draw (one layer drawn, then deep-copied: all layers start equal) are torch's.  Its `forward` is never called."""

    def __init__(self, cfg: VariantConfig, dropout: float):
        super().__init__()
        layer = nn.TransformerEncoderLayer(cfg.embed_dim, cfg.num_heads, cfg.transformer_ffn_hidden_size, dropout,
                                           cfg.transformer_ffn_activation, batch_first=True)
        self.transformer = nn.TransformerEncoder(layer, cfg.transformer_num_layers, enable_nested_tensor=False)

    def forward(self, *args, **kwargs):
        raise RuntimeError("drin_amd.ghmfc_variants: torch's TransformerEncoder holds the parameters only; VariantModel runs them")


class _AvgLinear(nn.Module):
    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.linear = nn.Linear(in_dim, out_dim)


class _VariantMentionEncoder(nn.Module):
    """ghmfc.py's MentionEncoder for the three variants: the same modules under the same names, created in the same order."""

    def __init__(self, cfg: VariantConfig, dropout: float, attention):
        super().__init__()
        D = cfg.embed_dim
        if cfg.mention_final_layer_name == "linear":
            self.final_layer = _AvgLinear(D, D)
        elif cfg.mention_final_layer_name == "transformer":
            self.intermediate_layer = _MultilayerTransformer(cfg, dropout)
        elif cfg.mention_final_layer_name == "multimodal":
            self.intermediate_layer = _CrossAttention(D, cfg.image_dim, cfg.num_heads, dropout, attention)


class VariantModel(TableForm, nn.Module):
    """ghmfc.py's `Model` with one of the other mention encoders: the reference's modules created in its order (the same
    state-dict keys and the same initial draw under one `torch.manual_seed`; a reference checkpoint loads).  With the default
    configuration (`"multimodal"`, `"bi"`) the constructor returns a `TrainableModel`.

    `forward(batch)` takes the reference's 8-item offline batch and returns scores [B, N], `encode_mentions(batch)` the [B, D]
    mention representations.  Item 4 (`mention_image`) is read by `"multimodal"` only; for the other encoders it is the loader's
    0 and never touched.  `train()`: gradients reach every parameter that requires one; with `dropout > 0` every transformer
    layer takes four draws from the model's one `DropoutStream(seed)` in the order attention weights, drop1 (on the attention
    output), drop (on the activated FFN hidden rows), drop2 (on the FFN output), layers ascending; `"text"` takes its two
    attention draws in CrossAttention's order.  `eval()`: the same composition under `no_grad`, no dropout.  After a max-pool
    forward `max_indices == {"text": idx [B, D]}` (int32): the lowest position that attains each maximum, over ALL L positions
    (padded ones take part, as in the reference).  "avg extract" means over `begin : end` with Python's slice clipping; an
    empty span gives a NaN row, as the reference.

    A mention whose mask is all zero: in the transformer its attention rows are zero (the core's rule for a query with no
    kept key), so its scores are finite - the library's definition; torch has two answers there (NaN on its fused inference
    path, finite under autograd).  Batch tensors are detached: their gradients are out of scope.  CPU tensors are refused.
    `core`: the softmax-attention core of every attention of the model, "fma" (the default) or "mfma"
    (`drin_amd.attention.attention_core`), in `train()` and `eval()` alike.
    Table form (`drin_amd.ghmfc_table.TableForm`): the mention representation as above, the entity side through the indexed row
    kernels - the bits of the gathered batch; `enable_entity_cache()` scores `eval()` calls against per-entity rows."""

    def __new__(cls, cfg: VariantConfig | None = None, precision: str = "bf16x3", dropout: float = 0.1, seed: int = 0,
                core: str = "fma"):
        cfg = cfg or VariantConfig()
        if cfg.is_default:
            return TrainableModel(cfg.base(), precision=precision, dropout=dropout, seed=seed, core=core)
        return super().__new__(cls)

    def __init__(self, cfg: VariantConfig | None = None, precision: str = "bf16x3", dropout: float = 0.1, seed: int = 0,
                 core: str = "fma"):
        super().__init__()
        self.cfg, self.precision, self.dropout, self.core = cfg, precision, check_setup(precision, core, dropout), core
        self.dropout_stream = DropoutStream(seed)
        self.max_indices = {}
        self.mention_encoder = _VariantMentionEncoder(cfg, self.dropout, attention_factory(precision, self.dropout_stream, core))
        self.entity_encoder = _EntityEncoder(cfg)

    # ---- the batch ---------------------------------------------------------------------------------------------
    def _batch_tensors(self, batch, table_form: bool = False):
        """table_form: items 5 and 6 are not the entity features (ef comes back as None: the caller reads the table)"""
        mf, mmask, begin, end, mimage = batch[:5]
        ef, emask = (None, None) if table_form else batch[5:7]
        dev = model_device(self, mf)
        if dev.type != "cuda" or (isinstance(mf, torch.Tensor) and mf.device.type != "cuda"):
            raise RuntimeError("drin_amd.ghmfc_variants.VariantModel runs on the GPU only (no CPU fallback): move the model and the "
                               "batch with .cuda()")
        cfg = self.cfg
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()          # noqa: E731
        i = lambda t: torch.as_tensor(t).detach().to(dev, torch.int64).contiguous()   # noqa: E731
        mf, mmask, begin, end = f(mf), i(mmask), i(begin), i(end)
        mimage = f(mimage) if cfg.reads_mention_image else None
        B = mf.shape[0]
        if table_form:
            got = tuple(mf.shape), tuple(mmask.shape), tuple(begin.shape), tuple(end.shape)
            want = (B, cfg.mention_tokens, cfg.embed_dim), (B, cfg.mention_tokens), (B,), (B,)
            if got != want or (mimage is not None and tuple(mimage.shape) != (B, cfg.image_regions, cfg.image_dim)):
                raise ValueError(f"ghmfc batch shapes {got} do not match the configuration {cfg}")
            return mf, mmask, begin, end, mimage, None, None
        ef = f(ef)
        if ef.dim() == 4:                                                      # WikiMEL: [B, N, T, D] + entity_mask [B, N, T]
            emask = i(emask)
            if tuple(emask.shape) != tuple(ef.shape[:3]):
                raise ValueError(f"entity_mask {tuple(emask.shape)} does not match entity_feature {tuple(ef.shape)}")
        else:
            emask = None
        got = tuple(mf.shape), tuple(mmask.shape), tuple(begin.shape), tuple(end.shape)
        want = (B, cfg.mention_tokens, cfg.embed_dim), (B, cfg.mention_tokens), (B,), (B,)
        if got != want or tuple(ef.shape[:2]) != (B, cfg.num_candidates) or ef.shape[-1] != cfg.embed_dim or (
                mimage is not None and tuple(mimage.shape) != (B, cfg.image_regions, cfg.image_dim)):
            raise ValueError(f"ghmfc batch shapes {got}, entity_feature {tuple(ef.shape)} do not match the configuration {cfg}")
        return mf, mmask, begin, end, mimage, ef, emask

    # ---- the encoders ------------------------------------------------------------------------------------------
    def _transformer(self, x, padding):
        """nn.TransformerEncoder(x, src_key_padding_mask=padding): post-norm layers, no final norm (ghmfc.py:75-90)"""
        cfg = self.cfg
        return transformer_stack(self.mention_encoder.intermediate_layer.transformer.layers, x, padding, num_heads=cfg.num_heads,
                                 ffn_hidden_size=cfg.transformer_ffn_hidden_size, ffn_activation=cfg.transformer_ffn_activation,
                                 precision=self.precision, core=self.core, dropout=self.dropout if self.training else 0.0,
                                 dropout_stream=self.dropout_stream)

    def _mention(self, mf, mmask, begin, end, mimage):
        cfg, prec = self.cfg, PRECISIONS[self.precision]
        name = cfg.mention_final_layer_name
        padding = mmask == 0                                                   # nn.MultiheadAttention: True = drop the key
        if name == "transformer":
            x = self._transformer(mf, padding)
        elif name == "multimodal":
            x = cross_attention(self.mention_encoder.intermediate_layer, mf, padding, mimage, None, self.precision,
                                cfg.layer_norm_eps)                            # every key of the image is kept
        else:
            x = mf
        self.max_indices = {}
        if name == "linear":
            final = self.mention_encoder.final_layer.linear
            return _linear(span_mean(x, begin, end), final.weight, final.bias, prec)
        if cfg.mention_final_representation == "max pool":
            out, idx = seq_max(x)
            self.max_indices = {"text": idx}
            return out
        return span_mean(x, begin, end)

    def _mention_only(self, mention) -> torch.Tensor:
        """`[B, D]` mention representations from the five mention-side items alone (the eval composition's mention encoder):
        what `link` ranks the table with."""
        mf, mmask, begin, end, mimage, _ef, _emask = self._batch_tensors(mention, True)
        return self._mention(mf, mmask, begin, end, mimage)

    def _run(self, batch, want_scores: bool):
        if not self.training:
            with torch.no_grad():
                return self._compose(batch, want_scores)
        return self._compose(batch, want_scores)

    def _compose(self, batch, want_scores: bool):
        tb = self._table_form(batch)
        mf, mmask, begin, end, mimage, ef, emask = self._batch_tensors(batch if tb is None else tb.mention, tb is not None)
        mention = self._mention(mf, mmask, begin, end, mimage)
        if not want_scores:
            return mention
        if tb is not None:
            if tb.candidates.shape[0] != mf.shape[0]:
                raise ValueError(f"ghmfc table form: candidates {tuple(tb.candidates.shape)} for {mf.shape[0]} mentions")
            if not self.training:
                return self._eval_scores(tb, mention)
            ef = self._train_candidates(tb)
        return entity_scores(mention, ef, emask, self.entity_encoder.final_layer, self.cfg, self.precision)

    def forward(self, batch) -> torch.Tensor:
        return self._run(batch, True)

    def encode_mentions(self, batch) -> torch.Tensor:
        return self._run(batch, False)
