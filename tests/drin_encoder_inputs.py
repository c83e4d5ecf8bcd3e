"""Cases and seeded inputs of DRIN's other mention encoders, shared by tools/gen_drin_encoder_golden.py
(which runs the unmodified reference) and the tests (which read tests/golden/drin_encoders.npz).  Neither weights nor inputs are
stored: the weights are the initial draw under `torch.manual_seed(case seed)`, the inputs `drin_amd.synth.make_batch` plus the
plants below.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig

GOLDEN_FILE = "drin_encoders.npz"
SMALL = dict(bert_embed_dim=16, gcn_embed_dim=16, resnet_embed_dim=8, max_mention_sentence_len=5, resnet_num_region=2,
             num_candidates_data=2, transformer_num_layers=2, transformer_num_heads=2, transformer_ffn_hidden_size=32)
AVG, MAX = "avg extract", "max pool"

# name: (config, B, data seed, weight seed)
CASES = {
    "none_avg": (DrinConfig(mention_final_layer_name="none", mention_final_representation=AVG, **SMALL), 3, 51, 1),
    "none_max": (DrinConfig(mention_final_layer_name="none", mention_final_representation=MAX, **SMALL), 3, 52, 2),
    "tr_avg": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=AVG, **SMALL), 3, 53, 3),
    "tr_max": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=MAX, **SMALL), 3, 54, 4),
    # WikiMEL form: token-level entity text, N = 4, T = 3
    "tr_max_wm": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=MAX, dataset_name="wikimel",
                             max_entity_attr_token_len=3, **{**SMALL, "num_candidates_data": 3}), 3, 55, 5),
    "tr_max_vector_static": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=MAX,
                                        gcn_edge_feature="vector", gcn_edge_type="static", **SMALL), 3, 56, 6),
    # head dim 5, L past one 32-key tile of the attention cores and no multiple of the row groups
    "tr_head5": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=MAX,
                            **{**SMALL, "bert_embed_dim": 20, "gcn_embed_dim": 20, "transformer_num_heads": 4,
                               "max_mention_sentence_len": 33}), 3, 57, 7),
    # the reference widths: 8 layers of 8 heads, ffn 512, L = 128, N = 11
    "tr_full": (DrinConfig(mention_final_layer_name="transformer", mention_final_representation=MAX), 2, 58, 8),
}
EMPTY_SPAN_CASE, EMPTY_SPAN_ROW = "none_avg", 2      # an empty span: a NaN row, as the reference
PADDED_ROW, TIE_ROW = 0, 1                           # max cases: a padded position attains a maximum; an exact tie


def mask_lengths(name: str) -> np.ndarray:
    """Tokens kept per mention: row 0 is the shortest (its last position is padded), none is all-zero."""
    cfg, B = CASES[name][0], CASES[name][1]
    L = cfg.max_mention_sentence_len
    return np.array([max(3, L - 2), L, L - 1][:B] + [L] * max(0, B - 3), dtype=np.int64)


def encoder_inputs(name: str):
    """The reference's 15-sequence (the 14-tuple + answer) of case `name`, CPU tensors."""
    cfg, B, dseed, _w = CASES[name]
    batch = synth.make_batch(cfg, B, dseed)
    L = cfg.max_mention_sentence_len
    batch[1] = torch.from_numpy((np.arange(L)[None, :] < mask_lengths(name)[:, None]).astype(np.int64))
    text = batch[0]
    if cfg.mention_final_representation == MAX:
        text[PADDED_ROW, L - 1, 0] = 9.0                               # a padded position (row 0 keeps L - 2 tokens) wins column 0
        text[TIE_ROW, :, 2] = -1.0
        text[TIE_ROW, 1, 2] = text[TIE_ROW, 3, 2] = 7.0                # an exact tie: the lowest position takes the gradient
    if name == EMPTY_SPAN_CASE:
        batch[2][EMPTY_SPAN_ROW], batch[3][EMPTY_SPAN_ROW] = 2, 2
    return batch


def rows_without_nan(name: str):
    B = CASES[name][1]
    return [b for b in range(B) if not (name == EMPTY_SPAN_CASE and b == EMPTY_SPAN_ROW)]


def transformer_keys(layers: int):
    pre = "vertex_encoder.mention_text_encoder.intermediate_layer.transformer.layers."
    per = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight",
           "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
    return [f"{pre}{i}.{k}" for i in range(layers) for k in per]
