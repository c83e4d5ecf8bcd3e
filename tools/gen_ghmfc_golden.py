"""Generate tests/golden/ghmfc_*.npz: scores and mention representations of the UNMODIFIED reference GHMFC model in eval mode.

TEST INFRASTRUCTURE, run in the build container only (needs the reference checkout that oracle/gen_golden.py imports).  The
reference's `baselines/ghmfc.py` `Model` is built after `torch.manual_seed(case seed)` with its module globals patched to the
case's geometry and to the `model_type == "ghmfc"` defaults of `common/args.py`, put in `eval()` mode and run on the batch of
`tests/ghmfc_inputs.py` (numpy Philox: the tests regenerate it bit for bit).  Stored per case: `scores` [B, N] and
`mention_repr` [B, D] (the output of `model.mention_encoder`) in full, the 52 state-dict key names and the per-tensor weight
sums (the tests regenerate the weights from the seed).  Weights and inputs are not stored.

  ghmfc_tiny.npz    the tiny-width cases (WikiDiverse B = 1, 5, WikiMEL B = 3)
  ghmfc_shapes.npz  the shape cases (head dims 5 and 9, L = P = N = 1, L = 200 and 512, B = 300)
  ghmfc_full.npz    the reference widths, B = 4 and 64, plus the key names and weight sums after torch.manual_seed(0)

usage:  python tools/gen_ghmfc_golden.py
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

from tests.ghmfc_inputs import ALL_ZERO_ROW, CASES, FULL, KEYS, PADDED_MAX_ROW, dataset_of, geometry, ghmfc_inputs, mask_lengths  # noqa: E402


def _patch(g: dict, dataset: str) -> None:
    vals = dict(bert_embed_dim=g["D"], resnet_embed_dim=g["R"], max_mention_sentence_len=g["L"], resnet_num_region=g["P"],
                num_candidates_model=g["N"], transformer_num_heads=g["H"], mention_final_output_dim=g["D"],
                entity_final_output_dim=g["D"], dataset_name=dataset, use_device="cpu", online_bert=False,
                mention_final_layer_name="multimodal", mention_final_representation="max pool", entity_final_layer_name="linear",
                entity_final_pooling="avg", multimodal_subspace_activation="gelu", mention_multimodal_attention="bi")
    for mod in (ref_args, ref_ghmfc):
        for k, v in vals.items():
            setattr(mod, k, v)


def _tensors(batch):
    """numpy -> torch; the loader's scalar 0 items become the [B] zero tensors its collate function makes of them."""
    B = batch[0].shape[0]
    return [torch.from_numpy(x) if isinstance(x, np.ndarray) else torch.zeros(B, dtype=torch.int64) for x in batch]


def run(name: str) -> dict:
    case = CASES[name]
    _patch(geometry(name), dataset_of(name))
    torch.manual_seed(case["seed"])
    model = ref_ghmfc.Model().eval()
    sd = model.state_dict()
    assert list(sd) == KEYS, list(sd)
    batch = _tensors(ghmfc_inputs(name))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scores = model(batch)
        mention = model.mention_encoder(batch[:5])
        if case["masks"] == "corners":
            # the scaled padded token row must win the max over the sequence somewhere
            seq = model.mention_encoder.intermediate_layer.t2v_attention(batch[0], batch[1], batch[4], None)
            where = seq[PADDED_MAX_ROW].argmax(0)
            assert (where >= int(mask_lengths(name)[PADDED_MAX_ROW])).any(), "no padded position wins the max"
            assert torch.isfinite(scores[ALL_ZERO_ROW]).all(), "the all-zero mask row is not finite"
    nan = torch.isnan(scores)
    if "T" in case:   # the 2-token entities: tokens 1 : 1 are an empty slice
        ntok = torch.from_numpy(ghmfc_inputs(name)[6]).sum(-1)
        assert torch.equal(nan, ntok == 2), "NaN scores exactly at the 2-token entities"
    else:
        assert not nan.any(), name
    assert not torch.isnan(mention).any(), name
    return {f"{name}/scores": scores.numpy().copy(), f"{name}/mention_repr": mention.numpy().copy(),
            f"{name}/keys": np.array(list(sd)), f"{name}/w_sums": np.array([v.double().sum().item() for v in sd.values()])}


def main():
    torch.set_num_threads(8)
    files = {"ghmfc_tiny.npz": {}, "ghmfc_shapes.npz": {}, "ghmfc_full.npz": {}}
    for name, case in CASES.items():
        dst = "ghmfc_full.npz" if case.get("geom") is FULL else ("ghmfc_shapes.npz" if "geom" in case or name == "b300" else "ghmfc_tiny.npz")
        files[dst].update(run(name))
        print("case", name, flush=True)
    _patch(FULL, "wikidiverse")
    torch.manual_seed(0)
    sd = ref_ghmfc.Model().state_dict()
    files["ghmfc_full.npz"]["state_dict_seed0/keys"] = np.array(list(sd))
    files["ghmfc_full.npz"]["state_dict_seed0/sums"] = np.array([v.double().sum().item() for v in sd.values()])
    for fname, data in files.items():
        dst = os.path.join(REPO, "tests", "golden", fname)
        np.savez_compressed(dst, **data)
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
