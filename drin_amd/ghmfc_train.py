"""GHMFC (`baselines/ghmfc.py`) that trains on the HIP library: `TrainableModel`, `drin_amd.ghmfc.Model` with a training-mode
forward composed of `drin_amd.attention.MultiheadAttention`, the library's linear products and the row operations of
`drin_amd.row_ops` - every one a HIP kernel pair, no torch math between the batch and the scores.  Attention dropout is the
library's own counter-based mask (one `DropoutStream` for the four attentions), not torch's random stream.  What the kernels
compute, the tie rule of the max and the mask function: DESIGN.md section 18.
"""
from __future__ import annotations

import torch

from .attention import PRECISIONS, DropoutStream, MultiheadAttention, _check_core, _linear
from .ghmfc import GhmfcConfig, Model, _MentionEncoder
from .row_ops import cosine_rows, entity_token_pool, gate_mix, layer_norm_res, seq_max


# ---- what TrainableModel and drin_amd.ghmfc_variants.VariantModel share ---------------------------------------------
def check_setup(precision: str, core: str, dropout: float) -> float:
    """The constructor arguments of both models, refused before any module is built; returns the rate as a float."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r} not in {sorted(PRECISIONS)}")
    _check_core(core)
    if not 0.0 <= dropout < 1.0:
        raise ValueError(f"dropout {dropout} is not in [0, 1)")
    return float(dropout)


def attention_factory(precision: str, stream: DropoutStream, core: str):
    """nn.MultiheadAttention's arguments -> a `MultiheadAttention` of the model's precision, dropout stream and core."""
    def attention(*args, **kwargs):
        return MultiheadAttention(*args, precision=precision, dropout_stream=stream, core=core, **kwargs)
    return attention


def cross_attention(ca, seq_a, drop_a, seq_b, drop_b, precision: str, eps: float) -> torch.Tensor:
    """CrossAttention(seq_a, mask_a, seq_b, mask_b) of ghmfc.py:114-128: [B, La, E].  drop_a / drop_b: bool key padding masks
    (True = drop the key) or None, which keeps every key."""
    B, La, E = seq_a.shape
    prec, ln = PRECISIONS[precision], ca.layernorms
    ffn = lambda m, t: _linear(t.view(B * La, E), m.weight, m.bias, prec).view(B, La, E)   # noqa: E731
    x, _ = ca.a2b_attention(seq_a, seq_b, seq_b, key_padding_mask=drop_b)
    x = layer_norm_res(x, None, ln[0].weight, ln[0].bias, eps)
    x = layer_norm_res(ffn(ca.a2b_ffn, x), x, ln[1].weight, ln[1].bias, eps)
    y, _ = ca.b2a_attention(x, seq_a, seq_a, key_padding_mask=drop_a)
    y = layer_norm_res(y, None, ln[2].weight, ln[2].bias, eps)
    return layer_norm_res(ffn(ca.b2a_ffn, y), y, ln[3].weight, ln[3].bias, eps)


def entity_scores(mention, ef, emask, final, cfg: GhmfcConfig, precision: str) -> torch.Tensor:
    """EntityEncoder and the cosine (ghmfc.py:237-250, :297-298): scores [B, N] of mention [B, D] against the candidates.
    ef: [B, N, D], or [B, N, T, D] with emask [B, N, T] (WikiMEL: the token pool of `cfg.entity_final_pooling` first); final: the
    encoder's last linear, or its nn.Identity (`entity_final_layer_name = "none"`): then no product, the cosine is of the pooled rows."""
    B, N, D = mention.shape[0], cfg.num_candidates, cfg.embed_dim
    ent = entity_token_pool(ef, emask, cfg.entity_final_pooling) if emask is not None else ef
    if not isinstance(final, torch.nn.Identity):
        ent = _linear(ent.view(B * N, D), final.weight, final.bias, PRECISIONS[precision]).view(B, N, D)
    return cosine_rows(mention, ent, cfg.cosine_eps)


class TrainableModel(Model):
    """`drin_amd.ghmfc.Model` that also trains: the same modules created in the same order (the same 52 state-dict keys and
    the same initial draw under one `torch.manual_seed`; a `ghmfc.Model` checkpoint loads), with the four attentions as
    `drin_amd.attention.MultiheadAttention`s that share one `DropoutStream(seed)`.

    `eval()`: `forward` / `encode_mentions` are the parent's (`drin_ghmfc_forward`, the same bits, no gradient).
    `train()`: the forward runs operation by operation in the order of `drin_ghmfc_forward`, and gradients reach every
    parameter that requires one (a frozen parameter is skipped; the bits of the others do not change).  Attention weights are
    dropped at rate `dropout` by the library's mask; `dropout=0` trains without.  After each training forward
    `max_indices == {"text": idx [B, D], "image": idx [B, R]}` (int32) holds the position each max over the sequence took its
    value from - the lowest one on a tie, which is where the gradient goes.  The batch tensors are detached: their gradients
    are out of scope.  A 2-token WikiMEL entity gives a NaN row, as in the reference.  CPU tensors are refused.
    Table form (`drin_amd.ghmfc_table`): a training step gathers the candidates' rows of the once-pooled table and runs the
    same `entity_scores` on them - the scores and gradients of the gathered-batch step, bit for bit.
    `core`: the softmax-attention core of the training forward and backward, "fma" (the default) or "mfma"
    (`drin_amd.attention.attention_core`); `eval()` scores through `drin_ghmfc_forward`, whose core is the FMA one."""

    def __init__(self, cfg: GhmfcConfig | None = None, precision: str = "bf16x3", dropout: float = 0.1, seed: int = 0,
                 core: str = "fma"):
        dropout = check_setup(precision, core, dropout)
        # read by _make_mention_encoder, which the parent's __init__ calls: set ahead of nn.Module.__init__, past its __setattr__
        object.__setattr__(self, "_attention_setup", (dropout, DropoutStream(seed), precision, core))
        super().__init__(cfg, precision)
        self.dropout, self.dropout_stream = self._attention_setup[:2]
        self.core = core
        self.max_indices = {}

    def _make_mention_encoder(self, cfg: GhmfcConfig):
        dropout, stream, precision, core = self._attention_setup
        return _MentionEncoder(cfg, dropout, attention_factory(precision, stream, core))

    def _run(self, batch, want_scores: bool):
        if not self.training:
            return self._score(batch, want_scores)
        tb = self._table_form(batch)
        if tb is None:
            mf, mmask, mimage, ef, emask, tokens = self._batch_tensors(batch)
        else:                                                                  # table form: pooled candidate rows [B, N, D], gathered
            mf, mmask, mimage = self._mention_tensors(tb.mention)
            ef, emask = (self._train_candidates(tb) if want_scores else None), None
        cfg, prec = self.cfg, PRECISIONS[self.precision]
        f = self.mention_encoder.intermediate_layer
        padding = mmask == 0                                                   # nn.MultiheadAttention: True = drop the key
        # CrossAttention and the max over seq_a's positions (ghmfc.py:143 / :145)
        t, idx_t = seq_max(cross_attention(f.t2v_attention, mf, padding, mimage, None, self.precision, cfg.layer_norm_eps))
        v, idx_v = seq_max(cross_attention(f.v2t_attention, mimage, None, mf, padding, self.precision, cfg.layer_norm_eps))
        self.max_indices = {"text": idx_t, "image": idx_v}
        tl = _linear(t, f.text_linear.weight, f.text_linear.bias, prec)
        vl = _linear(v, f.image_linear.weight, f.image_linear.bias, prec)
        mention = gate_mix(tl, vl, f.score_linear.weight, f.score_linear.bias)
        if not want_scores:
            return mention
        return entity_scores(mention, ef, emask, self.entity_encoder.final_layer, cfg, self.precision)
