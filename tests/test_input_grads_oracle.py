"""The CPU oracle's autograd gives the reference's gradients w.r.t. the batch tensors (tests/golden/input_grads.npz, written by
tools/gen_input_grad_golden.py from the unmodified reference).  Pins oracle/drin_oracle.py for this use: the GPU tests of the
input gradients compare against its fp64 autograd at sizes the fixtures do not cover.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import drin_oracle as O
from oracle.cases import build_case

FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
FULL = ["tiny_wd", "tiny_wm", "tiny_wd_edges_1010", "tiny_wd_static", "tiny_wd_layers3", "tiny_wd_vector", "tiny_wm_silu_relu"]
SUMMARY = ["wd_b4", "wm_b2"]
BAR = 2e-4          # relative Frobenius error per tensor, the bar of the parameter gradients
ABS_ZERO = 1e-6     # entity_object_score with one entity object: analytically 0 (the reference leaves ~1e-9) - unless a
#                     mention's object scores are all zero (tiny_wd): then its rows are ~1e6 through the +1e-9 of model.py:92,
#                     and the tensor is compared relatively


def rel_err(got: np.ndarray, ref: np.ndarray) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def oracle_input_grads(name, dtype=torch.float32):
    cfg, sd, batch = build_case(name)
    inputs = list(batch[:14])
    for i in FLOAT_INPUTS:
        inputs[i] = inputs[i].detach().to(dtype).requires_grad_(True)
    p = {k: v.to(dtype) for k, v in sd.items()}
    scores = O.forward(p, inputs, dtype=dtype, **O.config_kwargs(cfg))
    return cfg, inputs, scores


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "input_grads.npz"))


@pytest.mark.parametrize("name", FULL + SUMMARY)
def test_oracle_input_grads_match_reference(golden, name):
    cfg, inputs, scores = oracle_input_grads(name)
    G = torch.from_numpy(golden[f"{name}/G"])
    (scores * G).sum().backward()
    for i, field in FLOAT_INPUTS.items():
        gr = inputs[i].grad
        assert gr is not None, field
        if name in FULL:
            ref = golden[f"{name}/{field}"]
            assert gr.shape == ref.shape, field
            if field == "entity_object_score" and inputs[11].shape[-1] == 1 and np.abs(ref).max() <= ABS_ZERO:
                assert np.abs(gr.numpy()).max() <= ABS_ZERO, field          # analytically 0 (no zero object-score row)
                continue
            assert rel_err(gr.numpy(), ref) <= BAR, (field, rel_err(gr.numpy(), ref))
        else:
            l2 = float(golden[f"{name}/{field}_l2"])
            if field == "entity_object_score" and inputs[11].shape[-1] == 1 and l2 <= ABS_ZERO:
                assert gr.double().norm().item() <= ABS_ZERO
                continue
            assert abs(gr.double().norm().item() - l2) <= BAR * l2, field
            head = golden[f"{name}/{field}_head"]
            np.testing.assert_allclose(gr.flatten()[:16].numpy(), head, rtol=1e-3, atol=1e-3 * np.abs(head).max() + 1e-12)
