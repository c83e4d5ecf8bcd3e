"""Generate tests/golden/drin_encoders.npz: scores, layer-0 vertices and layer-0 edges of the UNMODIFIED reference DRIN model with
`mention_final_layer_name` "none" / "transformer" and either `mention_final_representation` (common/args.py:28-29), in eval mode.

TEST INFRASTRUCTURE, run in the build container only (needs the reference checkout, like tools/gen_ghmfc_variant_golden.py).  The
reference's `drin/model.py` `Model` is built after `torch.manual_seed(case seed)` with the module globals of `common.args`,
`baselines.ghmfc` and `drin.model` patched to the case's geometry and encoder names, `use_device = "cpu"`, put in `eval()` mode
and run WITH autograd enabled on the batch of tests/drin_encoder_inputs.py (under `torch.no_grad()` torch's transformer takes a
fused inference path; the generator asserts that both agree to 1e-6 on every transformer case).  Stored per case: `scores`
[B, N], the four layer-0 vertices, the four layer-0 edges [4, B, N], the state-dict key names and the per-tensor weight sums.
Weights and inputs are not stored.

usage:  python tools/gen_drin_encoder_golden.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import common.args as ref_args  # noqa: E402

ref_args.use_device = "cpu"
from baselines import ghmfc as ref_ghmfc  # noqa: E402
from drin import model as ref_model  # noqa: E402

from tests.drin_encoder_inputs import (CASES, EMPTY_SPAN_CASE, EMPTY_SPAN_ROW, GOLDEN_FILE, MAX, PADDED_ROW, TIE_ROW, encoder_inputs,  # noqa: E402
                                       mask_lengths, transformer_keys)


def _patch(cfg) -> None:
    vals = dict(dataset_name=cfg.dataset_name, num_candidates_data=cfg.num_candidates_data, num_candidates_model=cfg.num_candidates_model,
                bert_embed_dim=cfg.bert_embed_dim, resnet_embed_dim=cfg.resnet_embed_dim, gcn_embed_dim=cfg.gcn_embed_dim,
                mention_final_output_dim=cfg.gcn_embed_dim, entity_final_output_dim=cfg.gcn_embed_dim, num_gcn_layers=cfg.num_gcn_layers,
                gcn_edge_type=cfg.gcn_edge_type, gcn_edge_feature=cfg.gcn_edge_feature, gcn_edge_enabled=list(cfg.gcn_edge_enabled),
                gcn_vertex_activation=cfg.gcn_vertex_activation, gcn_edge_activation=cfg.gcn_edge_activation, use_device="cpu",
                online_bert=False, entity_final_layer_name="linear", entity_final_pooling="avg",
                max_mention_sentence_len=cfg.max_mention_sentence_len, mention_final_layer_name=cfg.mention_final_layer_name,
                mention_final_representation=cfg.mention_final_representation, transformer_num_layers=cfg.transformer_num_layers,
                transformer_num_heads=cfg.transformer_num_heads, transformer_ffn_hidden_size=cfg.transformer_ffn_hidden_size,
                transformer_ffn_activation=cfg.transformer_ffn_activation, transformer_dropout=cfg.transformer_dropout)
    for mod in (ref_args, ref_model, ref_ghmfc):
        for k, v in vals.items():
            setattr(mod, k, v)


def run(name: str, seen: dict) -> dict:
    cfg, _B, _dseed, wseed = CASES[name]
    _patch(cfg)
    torch.manual_seed(wseed)
    model = ref_model.Model().eval()
    sd = model.state_dict()
    tr = cfg.mention_final_layer_name == "transformer"
    assert len(sd) == 22 + (2 * cfg.num_gcn_layers if cfg.gcn_edge_feature == "vector" else 0) + (12 * cfg.transformer_num_layers if tr else 0)
    if tr:
        assert list(sd)[:12 * cfg.transformer_num_layers] == transformer_keys(cfg.transformer_num_layers)
    batch = encoder_inputs(name)
    inputs = batch[:-1]
    cap = {}
    model.vertex_encoder.register_forward_hook(lambda m, i, o: cap.__setitem__("vertex0", [t.detach().clone() for t in o]))
    model.edge_encoder.register_forward_hook(lambda m, i, o: cap.__setitem__("edge_enc", [t.detach().clone() for t in o]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scores = model(inputs).detach()
        if tr:
            assert int(mask_lengths(name).min()) >= 1, "a transformer case holds an all-zero mask"
            with torch.no_grad():
                fused = model(inputs)
            gap = (fused - scores).abs().max().item()
            assert gap <= 1e-6, (name, gap)
    mtet, miei = cap["edge_enc"]
    edges0 = torch.stack([mtet, inputs[13] / 100, inputs[12] / 100, miei])      # drin/model.py:201-204: tt, ti, it, ii
    nan = torch.isnan(scores)
    if name == EMPTY_SPAN_CASE:
        want = torch.zeros_like(nan)
        want[EMPTY_SPAN_ROW] = True
        assert torch.equal(nan, want), name
        seen["empty_span"] = True
    else:
        assert not nan.any(), name
    if cfg.mention_final_representation == MAX:
        text, L = inputs[0], cfg.max_mention_sentence_len
        where = text[PADDED_ROW].argmax(0)
        assert (where >= int(mask_lengths(name)[PADDED_ROW])).any(), "no padded position attains a maximum"
        col = text[TIE_ROW, :, 2]
        assert int((col == col.max()).sum()) == 2, "no exact tie"
        seen["padded_max"] = seen["tie"] = True
    out = {f"{name}/scores": scores.numpy().copy(), f"{name}/edges0": edges0.numpy().copy(), f"{name}/keys": np.array(list(sd)),
           f"{name}/w_sums": np.array([v.double().sum().item() for v in sd.values()])}
    for key, v in zip(("mt0", "mi0", "et0", "ei0"), cap["vertex0"]):
        out[f"{name}/{key}"] = v.numpy().copy()
    return out


def main():
    torch.set_num_threads(8)
    data, seen = {}, {}
    for name in CASES:
        data.update(run(name, seen))
        print("case", name, flush=True)
    assert seen.get("empty_span") and seen.get("padded_max") and seen.get("tie"), seen     # the generator's own coverage
    dst = os.path.join(REPO, "tests", "golden", GOLDEN_FILE)
    np.savez_compressed(dst, **data)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
