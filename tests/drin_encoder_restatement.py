"""fp64 restatement of DRIN's forward under a mention representation head (drin/model.py:164-209 with
`MentionEncoder(inline_bert=False)` of baselines/ghmfc.py:152-199 for `mention_final_layer_name` "none" / "transformer"):
the mention-text vertex is `repr(encoded)` - `encoded` being the intermediate layer's output, or the raw block itself - with no
Linear behind it, and the text-text edge takes `repr(mention_text)` of the RAW block (model.py:58,71-76).  `repr` is `Avg.avg`
(ghmfc.py:54-60) or `MaxPool` (ghmfc.py:63-70: the max over ALL positions).  Everything else is `oracle.drin_oracle`'s
vertex_encoder / edge_encoder / gcn_layer, composed as its `forward` composes them.  TEST INFRASTRUCTURE."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from oracle import drin_oracle as O

AVG, MAX = "avg extract", "max pool"
_W_MT = "vertex_encoder.mention_text_encoder.final_layer.linear."


def repr_rows(x: torch.Tensor, begin: torch.Tensor, end: torch.Tensor, representation: str, at: Optional[torch.Tensor] = None):
    """[B, D] = repr(x [B, L, D]).  `at` [B, D]: take the max at these positions (the library's own: where a column ties, autograd
    then sends the gradient where the library sends it); None: torch.max's."""
    if representation == AVG:
        return O.span_mean(x, begin, end)
    if at is None:
        return x.max(1)[0]
    return x.gather(1, at[:, None, :].long())[:, 0]


def head_forward(p, batch: Sequence[torch.Tensor], encoded: Optional[torch.Tensor], representation: str, *, at_edge=None,
                 at_vertex=None, num_layers=2, edge_enabled=(1, 1, 1, 1), dynamic=True, vector=False, vertex_activation="gelu",
                 edge_activation="sigmoid", trace: Optional[dict] = None) -> torch.Tensor:
    """Scores [B, N]; `p`, `batch`, `encoded` in the dtype to compute in (the caller converts and sets requires_grad)."""
    mtf, start, end = batch[0], batch[2], batch[3]
    D = mtf.shape[-1]
    q = dict(p)                                                        # the oracle's vertex encoder wants the Linear it replaces
    q.setdefault(_W_MT + "weight", torch.zeros(D, D, dtype=mtf.dtype))
    q.setdefault(_W_MT + "bias", torch.zeros(D, dtype=mtf.dtype))
    vertexes = O.vertex_encoder(q, batch, batch[7].dim() == 4)
    vertexes[0] = repr_rows(mtf if encoded is None else encoded, start, end, representation, at_edge if encoded is None else at_vertex)
    m = repr_rows(mtf, start, end, representation, at_edge)            # model.py:71: the raw block, never the encoder's output
    et_raw = batch[7][:, :, 0] if batch[7].dim() == 4 else batch[7]
    edges = [O.cosine(m[:, None, :], et_raw), batch[13] / 100, batch[12] / 100, O.edge_encoder(batch)[1]]
    if vector:
        edges = [e.unsqueeze(-1).expand(-1, -1, D) for e in edges]
    if trace is not None:
        trace["vertex0"], trace["edge0"] = [v.clone() for v in vertexes], [e.clone() for e in edges]
    for l in range(num_layers):
        vertexes, edges = O.gcn_layer(p, l, vertexes, edges, edge_enabled, dynamic, vector=vector, vertex_activation=vertex_activation,
                                      edge_activation=edge_activation)
    return O.cosine(vertexes[0][:, None, :], vertexes[2])


TRANSFORMER = "vertex_encoder.mention_text_encoder.intermediate_layer.transformer."


def encoder_forward(sd, batch: Sequence[torch.Tensor], cfg, *, at_edge=None, at_vertex=None, keeps=None, p: float = 0.0,
                    trace: Optional[dict] = None) -> torch.Tensor:
    """The whole model of a `DrinConfig` with the "transformer" / "none" encoder: the intermediate layer
    (tests/ghmfc_variant_restatement.transformer_encoder on the state dict `sd`; `keeps`, `p`: its dropout masks in draw order),
    then `head_forward`."""
    from tests.ghmfc_variant_restatement import transformer_encoder
    encoded = None
    if cfg.mention_final_layer_name == "transformer":
        encoded = transformer_encoder(sd, batch[0], batch[1] != 0, cfg.transformer_num_heads, cfg.transformer_num_layers,
                                      cfg.transformer_ffn_activation, keeps, p, prefix=TRANSFORMER)
    if trace is not None:
        trace["encoded"] = encoded
    return head_forward(sd, batch, encoded, cfg.mention_final_representation, at_edge=at_edge, at_vertex=at_vertex, trace=trace,
                        **O.config_kwargs(cfg))
