"""Generate tests/golden/ghmfc_entity.npz: scores, mention representations and entity encoder outputs of the UNMODIFIED
reference GHMFC model with `entity_final_pooling = "max"` and / or `entity_final_layer_name = "none"`, in eval mode.

TEST INFRASTRUCTURE, run in the build container only (needs the reference checkout, like tools/gen_ghmfc_variant_golden.py).
The reference's `baselines/ghmfc.py` `Model` is built after `torch.manual_seed(case seed)` with its module globals patched to the
case's geometry and encoder names, put in `eval()` mode and run on the batch of tests/ghmfc_entity_inputs.py.  Stored per case:
`scores` [B, N], `mention_repr` [B, D], the state-dict key names, the per-tensor weight sums and - the tiny cases - `entity_repr`
[B, N, D], the entity encoder's output.  Weights and inputs are not stored.

The generator asserts what the cases rest on: no pair holds 1 or 2 tokens (the reference raises IndexError on the empty max), no
score is NaN, and the max-pooled rows of an Identity final layer are bit-equal to `entity_feature[b, n, 1:ntok-1].max(0)[0]`.

usage:  python tools/gen_ghmfc_entity_golden.py
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

from tests.ghmfc_entity_inputs import CASES, GOLDEN_FILE, TINY_CASES, case_keys, dataset_of, entity_inputs, geometry, reference_names  # noqa: E402


def _patch(g: dict, dataset: str, names: dict) -> None:
    vals = dict(bert_embed_dim=g["D"], resnet_embed_dim=g["R"], max_mention_sentence_len=g["L"], resnet_num_region=g["P"],
                num_candidates_model=g["N"], transformer_num_heads=g["H"], mention_final_output_dim=g["D"],
                entity_final_output_dim=g["D"], dataset_name=dataset, use_device="cpu", online_bert=False,
                multimodal_subspace_activation="gelu", transformer_num_layers=g["layers"], transformer_ffn_hidden_size=g["ffn"], **names)
    for mod in (ref_args, ref_ghmfc):
        for k, v in vals.items():
            setattr(mod, k, v)


def _tensors(batch):
    """numpy -> torch; the loader's scalar 0 items become the [B] zero tensors its collate function makes of them."""
    B = batch[0].shape[0]
    return [torch.from_numpy(x) if isinstance(x, np.ndarray) else torch.zeros(B, dtype=torch.int64) for x in batch]


def run(name: str) -> dict:
    case, g = CASES[name], geometry(name)
    _patch(g, dataset_of(name), reference_names(name))
    torch.manual_seed(case["seed"])
    model = ref_ghmfc.Model().eval()
    sd = model.state_dict()
    assert list(sd) == case_keys(name), list(sd)
    batch = _tensors(entity_inputs(name))
    if "T" in case:
        ntok = batch[6].sum(-1)
        assert not ((ntok == 1) | (ntok == 2)).any(), f"{name}: a pair with 1 or 2 tokens (the reference raises on the empty slice)"
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        scores = model(batch)
        mention = model.mention_encoder(batch[:5])
        entity = model.entity_encoder(batch[5:])
    assert not torch.isnan(scores).any() and not torch.isnan(mention).any(), name
    if "T" in case and case["pooling"] == "max" and case["layer"] == "none":
        ef = batch[5]
        for b in range(ef.shape[0]):
            for n in range(ef.shape[1]):
                assert torch.equal(entity[b, n], ef[b, n, 1:int(ntok[b, n]) - 1].max(0)[0]), (name, b, n)
    out = {f"{name}/scores": scores.numpy().copy(), f"{name}/mention_repr": mention.numpy().copy(), f"{name}/keys": np.array(list(sd), dtype=str),
           f"{name}/w_sums": np.array([v.double().sum().item() for v in sd.values()])}
    if name in TINY_CASES:
        out[f"{name}/entity_repr"] = entity.numpy().copy()
    return out


def main():
    torch.set_num_threads(8)
    data = {}
    for name in CASES:
        data.update(run(name))
        print("case", name, flush=True)
    dst = os.path.join(REPO, "tests", "golden", GOLDEN_FILE)
    np.savez_compressed(dst, **data)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
