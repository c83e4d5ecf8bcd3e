"""Generate tests/golden/ghmfc_variants_*.npz: scores and mention representations of the UNMODIFIED reference GHMFC model with
its other mention encoders ("transformer", "multimodal" + "text", "linear", "none"; max pool or avg extract), in eval mode.

TEST INFRASTRUCTURE, run in the build container only (needs the reference checkout, like tools/gen_ghmfc_golden.py).  The
reference's `baselines/ghmfc.py` `Model` is built after `torch.manual_seed(case seed)` with its module globals patched to the
case's geometry and encoder names, put in `eval()` mode and run WITH autograd enabled on the batch of
tests/ghmfc_variant_inputs.py: under `torch.no_grad()` torch's transformer takes a fused inference path whose answer for a
fully masked mention differs (NaN), so no transformer case holds such a mention, and the generator asserts that both paths
agree to 1e-6 on every transformer case.  Stored per case: `scores` [B, N], `mention_repr` [B, D], the state-dict key names and
the per-tensor weight sums.  Weights and inputs are not stored.

  ghmfc_variants_tiny.npz    the tiny-width cases of all seven encoder / representation combinations
  ghmfc_variants_shapes.npz  head dim 5, L = 200, and the 1024-row products of tr_gates
  ghmfc_variants_full.npz    the reference widths with 8 layers, B = 2, and the key names and sums of all seven combinations

usage:  python tools/gen_ghmfc_variant_golden.py
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

from tests.ghmfc_variant_inputs import (CASES, EMPTY_SPAN_ROW, GOLDEN_FILE, PADDED_MAX_ROW, TINY, case_keys, dataset_of, geometry,  # noqa: E402
                                        keys_for, mask_lengths, reference_names, variant_inputs)

COMBINATIONS = [("transformer", "max"), ("transformer", "avg"), ("text", "max"), ("text", "avg"), ("linear", "avg"), ("none", "max"),
                ("none", "avg")]


def _patch(g: dict, dataset: str, names: dict) -> None:
    vals = dict(bert_embed_dim=g["D"], resnet_embed_dim=g["R"], max_mention_sentence_len=g["L"], resnet_num_region=g["P"],
                num_candidates_model=g["N"], transformer_num_heads=g["H"], mention_final_output_dim=g["D"],
                entity_final_output_dim=g["D"], dataset_name=dataset, use_device="cpu", online_bert=False,
                entity_final_layer_name="linear", entity_final_pooling="avg", multimodal_subspace_activation="gelu",
                transformer_num_layers=g["layers"], transformer_ffn_hidden_size=g["ffn"], **names)
    for mod in (ref_args, ref_ghmfc):
        for k, v in vals.items():
            setattr(mod, k, v)


def _tensors(batch):
    """numpy -> torch; the loader's scalar 0 items become the [B] zero tensors its collate function makes of them."""
    B = batch[0].shape[0]
    return [torch.from_numpy(x) if isinstance(x, np.ndarray) else torch.zeros(B, dtype=torch.int64) for x in batch]


def _sums(sd) -> np.ndarray:
    return np.array([v.double().sum().item() for v in sd.values()])


def run(name: str) -> dict:
    case, g = CASES[name], geometry(name)
    _patch(g, dataset_of(name), reference_names(name))
    torch.manual_seed(case["seed"])
    model = ref_ghmfc.Model().eval()
    sd = model.state_dict()
    assert list(sd) == case_keys(name), list(sd)
    batch = _tensors(variant_inputs(name))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scores = model(batch).detach()
        mention = model.mention_encoder(batch[:5]).detach()
        if case["enc"] == "transformer":
            assert int(mask_lengths(name).min()) >= 1, "a transformer case holds an all-zero mask"
            layers = model.mention_encoder.intermediate_layer.transformer.layers
            first = layers[0].state_dict()
            assert all(torch.equal(v, first[k]) for layer in layers for k, v in layer.state_dict().items()), "layers differ at init"
            with torch.no_grad():
                fused = model(batch)
            gap = (fused - scores).abs()[~torch.isnan(scores)].max().item()
            assert gap <= 1e-6 and torch.equal(torch.isnan(fused), torch.isnan(scores)), (name, gap)
        if case["masks"] == "corners":
            seq = model.mention_encoder.intermediate_layer(batch[0], batch[1], batch[4]).detach()
            where = seq[PADDED_MAX_ROW].argmax(0)
            assert (where >= int(mask_lengths(name)[PADDED_MAX_ROW])).any(), "no padded position wins the max"
    nan = torch.isnan(scores)
    if case["spans"] == "forms":   # the empty span: a NaN row
        want = torch.zeros_like(nan)
        want[EMPTY_SPAN_ROW] = True
        assert torch.equal(nan, want) and torch.equal(torch.isnan(mention), want[:, :1].expand_as(mention)), name
    else:
        assert not nan.any() and not torch.isnan(mention).any(), name
    return {f"{name}/scores": scores.numpy().copy(), f"{name}/mention_repr": mention.numpy().copy(), f"{name}/keys": np.array(list(sd)),
            f"{name}/w_sums": _sums(sd)}


def main():
    torch.set_num_threads(8)
    files = {f: {} for f in sorted(set(GOLDEN_FILE.values()))}
    for name in CASES:
        files[GOLDEN_FILE[name]].update(run(name))
        print("case", name, flush=True)
    for enc, rep in COMBINATIONS:   # key names and weight sums of every combination at the tiny widths after torch.manual_seed(0)
        names = dict(mention_final_layer_name="multimodal" if enc == "text" else enc,
                     mention_multimodal_attention="text" if enc == "text" else "bi",
                     mention_final_representation="max pool" if rep == "max" else "avg extract", transformer_ffn_activation="gelu")
        _patch(TINY, "wikidiverse", names)
        torch.manual_seed(0)
        sd = ref_ghmfc.Model().state_dict()
        assert list(sd) == keys_for(enc, TINY["layers"])
        files["ghmfc_variants_full.npz"][f"state_dict_seed0/{enc}_{rep}/keys"] = np.array(list(sd))
        files["ghmfc_variants_full.npz"][f"state_dict_seed0/{enc}_{rep}/sums"] = _sums(sd)
    for fname, data in files.items():
        dst = os.path.join(REPO, "tests", "golden", fname)
        np.savez_compressed(dst, **data)
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
