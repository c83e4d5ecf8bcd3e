"""Time linking against the whole table on one GPU (`drin_table_topk`): synthetic rows at D = 768,
E in {65 536, 1 000 000}, B in {64, 1024}, k = 100, both precisions, each configuration in `--repeats` FRESH processes (median
and spread over them), with the library's per-kernel-class split of one call (`edge`: padding, selection, re-score and sort;
the GEMM classes: the product), and in the same process, for scale:
  * the chunk's product alone in both orientations through `drin_linear_fwd` - entities as the row side, y[Ec, Bp] = rows x^T
    (what `drin_table_topk` launches), and mentions as the row side, y[B, Ec] = x rows^T;
  * chunked `torch.topk` over the normalised `x @ rows.T`.
Recorded rates: the selection's (edge class's) share of the call, the rows' bytes over the call time at B = 64, the product's
useful TF/s at B = 1024.  A record, not a gate.  Writes `--out` (profiles/ghmfc_link_bench.jsonl): a summary line, then one
line per configuration.

usage:  python tools/ghmfc_link_bench.py [--entities 65536,1000000] [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
D, K = 768, 100
BLOCK_BUDGET = 256 << 20


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


def default_chunk(B: int, E: int) -> int:
    """the library's default (table_topk.hip: TopkLayout): a multiple of 256 rows whose block stays inside 256 MiB"""
    Bp = (B + 3) // 4 * 4
    return min(max(BLOCK_BUDGET // (Bp * 4) // 256 * 256, 256), E)


def child(E: int, B: int, precision: str, steps: int, warmup: int) -> dict:
    import torch

    from drin_amd import _lib
    from drin_amd._lib import _ptr, _stream
    from drin_amd.attention import PRECISIONS
    from drin_amd.ghmfc_table import row_inv_norms
    lib, dev = _lib.load(), torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = torch.randn(E, D, device=dev, generator=g)
    x = torch.randn(B, D, device=dev, generator=g)
    inv = row_inv_norms(rows, 1e-8)
    nbytes = lib.drin_table_topk_workspace_bytes(B, E, D, K, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    scores = torch.empty(B, K, device=dev)
    best = torch.empty(B, K, dtype=torch.int64, device=dev)
    prec = PRECISIONS[precision]

    def link():
        _lib.check(lib.drin_table_topk(_ptr(x), _ptr(rows), _ptr(inv), E, B, D, K, 1e-8, prec, 0, _ptr(ws), nbytes, _ptr(scores), _ptr(best),
                                       _stream(dev)))

    call_ms = timeit(link, steps, warmup)
    _lib.profile_begin()
    link()
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    norms_ms = timeit(lambda: row_inv_norms(rows, 1e-8), steps, 1)
    # the chunk's product alone, both orientations
    chunk, Bp = default_chunk(B, E), (B + 3) // 4 * 4
    chunks = -(-E // chunk)
    xp = torch.zeros(Bp, D, device=dev)
    xp[:B] = x
    y = torch.empty(chunk * Bp, device=dev)
    part = rows[:chunk]
    entity_rows_ms = timeit(lambda: _lib.check(lib.drin_linear_fwd(_ptr(part), _ptr(xp), None, _ptr(y), chunk, Bp, D, prec, _stream(dev))),
                            steps, warmup) * chunks
    mention_rows_ms = timeit(lambda: _lib.check(lib.drin_linear_fwd(_ptr(xp), _ptr(part), None, _ptr(y), Bp, chunk, D, prec, _stream(dev))),
                             steps, warmup) * chunks

    # torch, for scale: normalised x @ rows.T in chunks of 65536 rows, a top-k per chunk, a top-k over the chunks' lists
    xn = torch.nn.functional.normalize(x, dim=1)

    def torch_link():
        vals, idx = [], []
        for e0 in range(0, E, 65536):
            s = (xn @ rows[e0:e0 + 65536].T) * inv[e0:e0 + 65536]
            v, i = torch.topk(s, K, dim=1)
            vals.append(v)
            idx.append(i + e0)
        v, j = torch.topk(torch.cat(vals, 1), K, dim=1)
        return v, torch.gather(torch.cat(idx, 1), 1, j)

    torch_ms = timeit(torch_link, max(steps // 2, 2), 1)
    agree = float((torch.sort(torch_link()[1], 1)[0] == torch.sort(best, 1)[0]).float().mean())
    return {"call_ms": call_ms, "norms_ms": norms_ms, "torch_ms": torch_ms, "rows_agree_with_torch": agree, "chunk": chunk, "chunks": chunks,
            "product_entity_rows_ms": entity_rows_ms, "product_mention_rows_ms": mention_rows_ms,
            "kernel_ms": {k: round(v[0], 4) for k, v in prof.items() if v[1]}, "launches": {k: v[1] for k, v in prof.items() if v[1]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", default="65536,1000000")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ghmfc_link_bench.jsonl"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        E, B, precision = a.child.split(":")
        print("RESULT " + json.dumps(child(int(E), int(B), precision, a.steps, a.warmup)), flush=True)
        return
    records, summary = [], {"workload": "ghmfc_link", "width": D, "k": K, "repeats": a.repeats}
    for E in [int(v) for v in a.entities.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            for precision in a.precisions.split(","):
                runs = []
                for _ in range(a.repeats):   # a fresh process each: allocator state, clocks and placement start over
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{E}:{B}:{precision}", "--steps", str(a.steps),
                                        "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        raise SystemExit(f"child {E}:{B}:{precision} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                    runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
                band = lambda key: {"min": round(min(v[key] for v in runs), 3), "median": round(statistics.median_low(v[key] for v in runs), 3),   # noqa: E731
                                    "max": round(max(v[key] for v in runs), 3)}
                call = band("call_ms")
                mid = runs[[v["call_ms"] for v in runs].index(statistics.median_low(v["call_ms"] for v in runs))]
                edge = mid["kernel_ms"].get("edge", 0.0)
                gemm = sum(mid["kernel_ms"].get(c, 0.0) for c in ("gemm", "gemm_x3", "gemm_planes"))
                rec = {"workload": "ghmfc_link", "entities": E, "batch": B, "width": D, "k": K, "precision": precision, "repeats": a.repeats,
                       "chunk": mid["chunk"], "chunks": mid["chunks"], "call_ms": call, "norms_ms": band("norms_ms"),
                       "mentions_per_s": round(B / call["median"] * 1e3, 1), "kernel_ms": mid["kernel_ms"], "launches": mid["launches"],
                       "selection_ms": round(edge, 4), "product_ms": round(gemm, 4), "selection_share": round(edge / max(edge + gemm, 1e-30), 3),
                       "selection_exceeds_product": edge > gemm,
                       "rows_gb_per_s": round(E * D * 4 / call["median"] / 1e6, 1),
                       "product_tflops": round(2.0 * B * E * D / max(gemm, 1e-30) / 1e9, 2),
                       "product_entity_rows_ms": band("product_entity_rows_ms"), "product_mention_rows_ms": band("product_mention_rows_ms"),
                       "torch_ms": band("torch_ms"), "torch_over_library": round(statistics.median_low(v["torch_ms"] for v in runs) / call["median"], 2),
                       "rows_agree_with_torch": mid["rows_agree_with_torch"]}
                records.append(rec)
                summary[f"E{E}_B{B}_{precision}"] = {key: (rec[key]["median"] if isinstance(rec[key], dict) and "median" in rec[key] else rec[key])
                                                    for key in ("call_ms", "selection_ms", "product_ms", "selection_share", "rows_gb_per_s",
                                                                "product_tflops", "product_entity_rows_ms", "product_mention_rows_ms", "torch_ms",
                                                                "torch_over_library")}
                print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
