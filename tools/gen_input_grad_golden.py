"""Generate tests/golden/input_grads.npz: gradients of the batch tensors through the UNMODIFIED reference.

TEST INFRASTRUCTURE, run in the build container only (needs the reference checkout that oracle/gen_golden.py imports).  For
each case of `oracle.cases`, the reference `Model` (drin/model.py:156-209) is built with the case's weights, every float
tensor of the 14-item batch is made a leaf that requires grad, and `(scores * G).sum()` is backpropagated, with G a seeded
standard normal [B, N] (stored as `<case>/G`).  Stored per case: the ten batch gradients in full for the tiny cases, their
fp64 sum and L2 norm plus the first 16 elements for the full-width ones.

usage:  python tools/gen_input_grad_golden.py            (writes tests/golden/input_grads.npz)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.gen_golden import _patch, ref_model  # noqa: E402
from oracle.cases import build_case  # noqa: E402

# position in the 14-sequence (drin/data.py:110-126) -> name
FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
FULL = ["tiny_wd", "tiny_wm", "tiny_wd_edges_1010", "tiny_wd_static", "tiny_wd_layers3", "tiny_wd_vector", "tiny_wm_silu_relu"]
SUMMARY = ["wd_b4", "wm_b2"]


def functional_weights(name: str, shape) -> np.ndarray:
    seed = sum(ord(c) for c in name)
    g = np.random.Generator(np.random.Philox(key=[seed, 7]))
    return g.standard_normal(size=tuple(shape), dtype=np.float32)


def run(name: str, full: bool) -> dict:
    cfg, sd, batch = build_case(name)
    _patch(cfg)
    model = ref_model.Model()
    model.load_state_dict(sd)
    inputs = list(batch[:14])
    for i in FLOAT_INPUTS:
        inputs[i] = inputs[i].detach().clone().requires_grad_(True)
    scores = model(inputs)
    G = functional_weights(name, scores.shape)
    (scores * torch.from_numpy(G)).sum().backward()
    out = {f"{name}/G": G}
    for i, field in FLOAT_INPUTS.items():
        gr = inputs[i].grad
        assert gr is not None, f"{name}: the reference gives no gradient for {field}"
        if full:
            out[f"{name}/{field}"] = gr.numpy().copy()
        else:
            out[f"{name}/{field}_sum"] = np.float64(gr.double().sum().item())
            out[f"{name}/{field}_l2"] = np.float64(gr.double().norm().item())
            out[f"{name}/{field}_head"] = gr.flatten()[:16].numpy().copy()
    return out


def main():
    torch.set_num_threads(8)
    out = {}
    for name in FULL:
        out.update(run(name, True))
        print("case", name)
    for name in SUMMARY:
        out.update(run(name, False))
        print("case", name)
    dst = os.path.join(REPO, "tests", "golden", "input_grads.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
