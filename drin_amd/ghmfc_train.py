"""GHMFC (`baselines/ghmfc.py`) that trains on the HIP library: `TrainableModel`, `drin_amd.ghmfc.Model` with a training-mode
forward composed of `drin_amd.attention.MultiheadAttention`, the library's linear products and the row operations of
`drin_amd.row_ops` - every one a HIP kernel pair, no torch math between the batch and the scores.  Attention dropout is the
library's own counter-based mask (one `DropoutStream` for the four attentions), not torch's random stream.  What the kernels
compute, the tie rule of the max and the mask function: DESIGN.md section 18.
"""
from __future__ import annotations

import torch

from .attention import CORES, PRECISIONS, DropoutStream, MultiheadAttention, _linear
from .ghmfc import GhmfcConfig, Model, _MentionEncoder
from .row_ops import cosine_rows, entity_token_mean, gate_mix, layer_norm_res, seq_max


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
    `core`: the softmax-attention core of the training forward and backward, "fma" (the default) or "mfma"
    (`drin_amd.attention.attention_core`); `eval()` scores through `drin_ghmfc_forward`, whose core is the FMA one."""

    def __init__(self, cfg: GhmfcConfig | None = None, precision: str = "bf16x3", dropout: float = 0.1, seed: int = 0,
                 core: str = "fma"):
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout {dropout} is not in [0, 1)")
        if core not in CORES:
            raise ValueError(f"core {core!r} not in {list(CORES)}")
        # read by _make_mention_encoder, which the parent's __init__ calls: set ahead of nn.Module.__init__, past its __setattr__
        object.__setattr__(self, "_attention_setup", (float(dropout), DropoutStream(seed), precision, core))
        super().__init__(cfg, precision)
        self.dropout, self.dropout_stream = self._attention_setup[:2]
        self.core = core
        self.max_indices = {}

    def _make_mention_encoder(self, cfg: GhmfcConfig):
        dropout, stream, precision, core = self._attention_setup

        def attention(*args, **kwargs):
            return MultiheadAttention(*args, precision=precision, dropout_stream=stream, core=core, **kwargs)
        return _MentionEncoder(cfg, dropout, attention)

    def _cross_attention_max(self, ca, seq_a, drop_a, seq_b, drop_b):
        """CrossAttention(seq_a, seq_b) and the max over seq_a's positions (ghmfc.py:114-128, :143 / :145)."""
        B, La, E = seq_a.shape
        prec, eps, ln = PRECISIONS[self.precision], self.cfg.layer_norm_eps, ca.layernorms
        ffn = lambda m, t: _linear(t.view(B * La, E), m.weight, m.bias, prec).view(B, La, E)   # noqa: E731
        x, _ = ca.a2b_attention(seq_a, seq_b, seq_b, key_padding_mask=drop_b)
        x = layer_norm_res(x, None, ln[0].weight, ln[0].bias, eps)
        x = layer_norm_res(ffn(ca.a2b_ffn, x), x, ln[1].weight, ln[1].bias, eps)
        y, _ = ca.b2a_attention(x, seq_a, seq_a, key_padding_mask=drop_a)
        y = layer_norm_res(y, None, ln[2].weight, ln[2].bias, eps)
        y = layer_norm_res(ffn(ca.b2a_ffn, y), y, ln[3].weight, ln[3].bias, eps)
        return seq_max(y)

    def _run(self, batch, want_scores: bool):
        if not self.training:
            return self._score(batch, want_scores)
        mf, mmask, mimage, ef, emask, tokens = self._batch_tensors(batch)
        cfg, prec = self.cfg, PRECISIONS[self.precision]
        B, N, D = mf.shape[0], cfg.num_candidates, cfg.embed_dim
        f = self.mention_encoder.intermediate_layer
        padding = mmask == 0                                                   # nn.MultiheadAttention: True = drop the key
        t, idx_t = self._cross_attention_max(f.t2v_attention, mf, padding, mimage, None)
        v, idx_v = self._cross_attention_max(f.v2t_attention, mimage, None, mf, padding)
        self.max_indices = {"text": idx_t, "image": idx_v}
        tl = _linear(t, f.text_linear.weight, f.text_linear.bias, prec)
        vl = _linear(v, f.image_linear.weight, f.image_linear.bias, prec)
        mention = gate_mix(tl, vl, f.score_linear.weight, f.score_linear.bias)
        if not want_scores:
            return mention
        ent = entity_token_mean(ef, emask) if tokens else ef
        final = self.entity_encoder.final_layer
        ent = _linear(ent.view(B * N, D), final.weight, final.bias, prec).view(B, N, D)
        return cosine_rows(mention, ent, cfg.cosine_eps)
