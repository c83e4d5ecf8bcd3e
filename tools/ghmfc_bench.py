"""Time GHMFC scoring on one GPU: the forward at the reference widths (D = 768, R = 2048, L = 128, P = 49, H = 8, N = 11) for
B = 64 and 1024 in both precisions, each configuration in `--repeats` FRESH processes (the band over them is reported), with
the library's per-kernel-class split and, for scale, the same forward in plain torch (nn.MultiheadAttention / nn.Linear /
nn.LayerNorm modules in eval mode, the reference's algorithm restated here) on the same GPU in the same process.
Prints one JSON line per configuration.

usage:  python tools/ghmfc_bench.py [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3] [--steps 10] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_batch(B: int, cfg, seed: int = 0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, R, L, P, N = cfg.embed_dim, cfg.image_dim, cfg.mention_tokens, cfg.image_regions, cfg.num_candidates
    mf = torch.randn(B, L, D, device="cuda", generator=g)
    mimage = torch.randn(B, P, R, device="cuda", generator=g).abs()
    ef = torch.randn(B, N, D, device="cuda", generator=g)
    mlen = torch.randint(8, L + 1, (B,), device="cuda", generator=g)
    mmask = (torch.arange(L, device="cuda")[None] < mlen[:, None]).long()
    return [mf, mmask, 0, 0, mimage, ef, 0, 0]


def torch_form(model, batch):
    """The reference's forward on the model's own modules (eval mode: no dropout)."""
    import torch
    import torch.nn.functional as F
    mf, mmask, _, _, mimage, ef = batch[:6]
    fusion = model.mention_encoder.intermediate_layer
    pad = mmask == 0

    def cross(ca, sa, pad_a, sb, pad_b):
        x = ca.a2b_attention(sa, sb, sb, key_padding_mask=pad_b, need_weights=False)[0]
        x = ca.layernorms[0](x)
        x = ca.layernorms[1](ca.a2b_ffn(x) + x)
        y = ca.b2a_attention(x, sa, sa, key_padding_mask=pad_a, need_weights=False)[0]
        y = ca.layernorms[2](y)
        return ca.layernorms[3](ca.b2a_ffn(y) + y)

    t = F.gelu(fusion.text_linear(cross(fusion.t2v_attention, mf, pad, mimage, None).max(1)[0]))
    v = F.gelu(fusion.image_linear(cross(fusion.v2t_attention, mimage, None, mf, pad).max(1)[0]))
    s = torch.softmax(fusion.score_linear(torch.cat([t, v], 1)), 1)
    men = s[:, :1] * t + s[:, 1:] * v
    ent = model.entity_encoder.final_layer(ef)
    return F.cosine_similarity(men.unsqueeze(1).expand_as(ent), ent, dim=-1)


def timeit(fn, steps: int, warmup: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def child(B: int, precision: str, steps: int, warmup: int, torch_steps: int) -> dict:
    import torch

    from drin_amd import _lib
    from drin_amd.ghmfc import GhmfcConfig, Model
    cfg = GhmfcConfig()
    torch.manual_seed(0)
    model = Model(cfg, precision=precision).cuda().eval()
    batch = make_batch(B, cfg)
    with torch.no_grad():
        fwd_ms = timeit(lambda: model(batch), steps, warmup)
        _lib.profile_begin()
        got = model(batch)
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        t_ms = timeit(lambda: torch_form(model, batch), torch_steps, 2)
        diff = (got - torch_form(model, batch)).abs().max().item()
    return {"forward_ms": fwd_ms, "torch_forward_ms": t_ms, "max_abs_diff_vs_torch": diff,
            "kernel_ms": {k: round(v[0], 4) for k, v in prof.items() if v[1]}, "launches": {k: v[1] for k, v in prof.items() if v[1]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        B, precision = a.child.split(":")
        print("RESULT " + json.dumps(child(int(B), precision, a.steps, a.warmup, a.torch_steps)), flush=True)
        return
    for B in [int(x) for x in a.batches.split(",")]:
        for precision in a.precisions.split(","):
            runs = []
            for _ in range(a.repeats):   # a fresh process each: allocator state, clocks and placement start over
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{B}:{precision}", "--steps", str(a.steps),
                                    "--warmup", str(a.warmup), "--torch-steps", str(a.torch_steps)], capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"child {B}:{precision} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            f = sorted(x["forward_ms"] for x in runs)
            t = sorted(x["torch_forward_ms"] for x in runs)
            mid = runs[[x["forward_ms"] for x in runs].index(statistics.median_low(f))]
            new = sum(mid["kernel_ms"].get(k, 0.0) for k in ("attn", "norm"))
            gemm = sum(mid["kernel_ms"].get(k, 0.0) for k in ("gemm", "gemm_x3", "gemm_planes"))
            print(json.dumps({
                "workload": "ghmfc_forward", "batch": B, "precision": precision, "repeats": a.repeats,
                "forward_ms": {"min": round(f[0], 3), "median": round(statistics.median_low(f), 3), "max": round(f[-1], 3)},
                "mentions_per_s": round(B / statistics.median_low(f) * 1e3, 1),
                "torch_forward_ms": {"min": round(t[0], 3), "median": round(statistics.median_low(t), 3), "max": round(t[-1], 3)},
                "torch_over_library": round(statistics.median_low(t) / statistics.median_low(f), 2),
                "max_abs_diff_vs_torch": mid["max_abs_diff_vs_torch"],
                "kernel_ms": mid["kernel_ms"], "launches": mid["launches"],
                "new_non_gemm_ms": round(new, 4), "gemm_ms": round(gemm, 4), "new_non_gemm_below_gemm": new < gemm,
            }), flush=True)


if __name__ == "__main__":
    main()
