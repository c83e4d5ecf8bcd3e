"""Cost of the batch-tensor gradients (drin_backward_ex): WikiMEL training step (forward + backward to the parameters, no
optimiser) at B = 64 and 512 with and without feature gradients, and a frozen-model attribution pass (forward + backward to
the inputs only) at B = 4 096 (WikiDiverse geometry).  Prints one JSON line.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python
tools/input_grad_bench.py` (k_token_block_bwd, k_miei_bwd_*, k_span_mean_bwd, k_axis_mean_bwd).

usage:  python tools/input_grad_bench.py [--steps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drin_amd import synth  # noqa: E402
from drin_amd.config import DrinConfig, wikimel_config  # noqa: E402
from drin_amd.model import Model  # noqa: E402

FLOAT = (0, 4, 5, 6, 7, 9, 10, 11, 12, 13)


def time_step(model, batch, feats: bool, steps: int, warmup: int) -> float:
    x = list(batch[:14])
    if feats:
        for i in FLOAT:
            x[i] = x[i].detach().requires_grad_(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize()
            ev[0].record()
        model.zero_grad(set_to_none=True)
        for i in FLOAT:
            x[i].grad = None
        model(x).sum().backward()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    cfg = wikimel_config()
    model = Model(cfg).cuda()
    model.load_state_dict(synth.make_state_dict(cfg, 7))
    out = {"geometry": "wikimel N=101 T=64 D=768 R=2048"}
    for B in (64, 512):
        batch = synth.make_device_batch(cfg, B, 3, "cuda")
        out[f"step_ms_b{B}"] = round(time_step(model, batch, False, a.steps, a.warmup), 3)
        out[f"step_feat_grads_ms_b{B}"] = round(time_step(model, batch, True, a.steps, a.warmup), 3)
        del batch
    # attribution at B = 4 096 on WikiDiverse (pooled entity text: a WikiMEL token block of 4 096 mentions is 81 GB)
    wd = DrinConfig()
    model = Model(wd).cuda().requires_grad_(False)
    model.load_state_dict(synth.make_state_dict(wd, 7))
    B = 4096
    batch = synth.make_device_batch(wd, B, 4, "cuda")
    out[f"attribution_wikidiverse_ms_b{B}"] = round(time_step(model, batch, True, max(a.steps // 4, 2), 2), 3)
    # the token block's write: B N T D fp32
    out["token_block_bytes_b64"] = 64 * 101 * 64 * 768 * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
