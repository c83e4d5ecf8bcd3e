"""Time the summed-cosine first stage on one GPU (`drin_table_topk_sum`, `Model.link(first_stage="edges")`):
synthetic tables at the widths of the three terms (768 text, 512 + 512 CLIP), k = N = 101, E in {65 536, 1 000 000}, B in {64, 1024},
both precisions; each configuration in `--repeats` FRESH child processes (median and spread over them).  Per configuration:
* `sum_ms` / `single_ms`: CALL times (a host clock over back-to-back calls that ends in one synchronise) of `table_topk_sum` with
  the three terms and, for scale, of `table_topk` at width 768 in the same process;
* per call, from `drin_profile_*` (device time per kernel class): `products_ms` (the GEMM classes of the whole call) and
  `edge_class_ms` (everything else of it), split by profiling the pieces alone in the same process - `combine_ms`
  (`drin_topk_combine` on blocks of the call's chunk, times the chunks of a call), `rescore_ms` (the three
  `drin_cosine_rows_indexed_fwd` on kp rows per mention) and `selection_ms` = the rest (partial lists, merges, padding, norms of
  the mentions, the chain, the finish);
* `link_edges_ms` beside `link_queries_ms`: `Model.link(first_stage="edges")` and `Model.link(queries=, rows=)` at the same N
  (pooled-text table, per-entity cache on), unless `--no-link`.
The KERNEL's rate comes from a run of its own under `rocprofv3 --kernel-trace --stats` (the program behind `--`), E = 1 M,
B = 1024: `k_topk_combine`'s bytes - (S + 1) blocks of a chunk per launch - over its average time, next to the 6.29 TB/s the
microarchitecture guide measures for a float4 copy.  A record, not a gate.  Writes `--out` (profiles/drin_link_edges_bench.jsonl):
a summary line, then one line per configuration.

usage:  python tools/drin_link_edges_bench.py [--entities 65536,1000000] [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3]
                                              [--no-link] [--no-trace]
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WIDTHS, K, KP, GUIDE_COPY_TB_S = (768, 512, 512), 101, 128, 6.29
BUDGET = 256 << 20


def default_chunk(E: int, B: int, S: int) -> int:
    Bp = (B + 3) // 4 * 4
    return min(E, max(256, BUDGET // (S * Bp * 4) // 256 * 256))


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


def profiled(fn, steps: int) -> dict:
    """device milliseconds per call and kernel class over `steps` calls of fn (drin_profile_begin / _end)"""
    import torch

    from drin_amd import _lib
    fn()
    torch.cuda.synchronize()
    _lib.profile_begin()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return {name: ms / steps for name, (ms, _n) in _lib.profile_end().items()}


def child(E: int, B: int, precision: str, steps: int, warmup: int, link: bool) -> dict:
    import torch

    from drin_amd import _lib, synth
    from drin_amd._lib import _ptr, _stream
    from drin_amd.config import DrinConfig
    from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk, table_topk_sum
    from drin_amd.model import EntityTable, Model
    lib, dev, eps, S = _lib.load(), torch.device("cuda"), 1e-8, len(WIDTHS)
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    tables = [rn(E, d) for d in WIDTHS]
    xs = [rn(B, d) for d in WIDTHS]
    invs = [row_inv_norms(t, eps) for t in tables]
    terms = [(x, t, i, 1.0) for x, t, i in zip(xs, tables, invs)]
    whole = lambda: table_topk_sum(terms, K, eps, precision)   # noqa: E731
    out = {"sum_ms": timeit(whole, steps, warmup), "single_ms": timeit(lambda: table_topk(xs[0], tables[0], invs[0], K, eps, precision), steps, warmup)}
    by_class = profiled(whole, steps)
    out["products_ms"] = sum(v for k, v in by_class.items() if k.startswith("gemm"))
    out["edge_class_ms"] = by_class["edge"]
    # the pieces alone: the combine on blocks of the call's chunk, the re-score on kp rows per mention
    Bp, chunk = (B + 3) // 4 * 4, default_chunk(E, B, S)
    blocks, scales = [rn(chunk, Bp) for _ in range(S)], [torch.rand(Bp, device=dev, generator=g) + 0.5 for _ in range(S)]
    arrays = [(C.c_void_p * S)(*[t.data_ptr() for t in ts]) for ts in (blocks, [i[:chunk] for i in invs], scales)]
    weights = (C.c_float * S)(*[1.0] * S)
    combine = lambda: _lib.check(lib.drin_topk_combine(*arrays, weights, S, Bp, B, chunk, _ptr(blocks[0]), _stream(dev)))   # noqa: E731
    out["chunk_entities"], out["chunks_per_call"] = chunk, -(-E // chunk)
    out["combine_launch_ms"] = profiled(combine, 4 * steps)["edge"]
    out["combine_ms"] = out["combine_launch_ms"] * E / chunk
    out["combine_bytes_per_call"] = (S + 1) * E * Bp * 4
    listed = torch.randint(0, E, (B, KP), device=dev, generator=g)
    out["rescore_ms"] = profiled(lambda: [cosine_rows_indexed(x, t, listed, eps, None) for x, t in zip(xs, tables)], steps)["edge"]
    out["selection_ms"] = out["edge_class_ms"] - out["combine_ms"] - out["rescore_ms"]
    del blocks
    if link:
        cfg = DrinConfig(num_candidates_data=K - 1)                     # WikiDiverse layout (pooled entity text) with N = 101
        R = cfg.resnet_embed_dim
        table = EntityTable(tables[0], None, rn(E, R), rn(E, 1, R), torch.rand(E, 1, device=dev, generator=g))
        table.set_clip(tables[1], tables[2]).enable_cache()
        model = Model(cfg, precision=precision).to(dev).eval()
        mention = synth.make_device_batch(cfg.with_(num_candidates_data=0), B, 3, dev)[:7]
        clip_image, clip_text = xs[2], xs[1]
        edges = lambda: model.link(mention, table, 10, clip_image, clip_text, first_stage="edges")   # noqa: E731
        queries = lambda: model.link(mention, table, 10, clip_image, clip_text, queries=xs[0], rows=tables[0])   # noqa: E731
        edges(), queries()                                              # builds the folds, the per-entity cache and the norms
        out["link_edges_ms"], out["link_queries_ms"] = timeit(edges, steps, warmup), timeit(queries, steps, warmup)
        model.check_indices()
    return out


TRACE_CALLS = 6


def trace_child(E: int, B: int) -> None:
    import torch

    from drin_amd.ghmfc_table import row_inv_norms, table_topk_sum
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(7)
    tables = [torch.randn(E, d, device=dev, generator=g) for d in WIDTHS]
    terms = [(torch.randn(B, d, device=dev, generator=g), t, row_inv_norms(t, 1e-8), 1.0) for d, t in zip(WIDTHS, tables)]
    for _ in range(TRACE_CALLS):
        table_topk_sum(terms, K, 1e-8, "bf16x3")
    torch.cuda.synchronize()


def kernel_trace(E: int, B: int) -> dict:
    """One run of `trace_child` under rocprofv3's kernel trace: k_topk_combine's average over all its launches of that run"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", f"{E}:{B}"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
    hit = [x for x in rows if "k_topk_combine" in x["Name"]]
    if not hit:
        raise RuntimeError("no k_topk_combine row in the kernel trace")
    row = max(hit, key=lambda x: int(x["Calls"]))
    S, Bp = len(WIDTHS), (B + 3) // 4 * 4
    chunk = default_chunk(E, B, S)
    launches = -(-E // chunk)
    mean_bytes = (S + 1) * E * Bp * 4 / launches                        # the last chunk is shorter: bytes of a call over its launches
    avg_ms = float(row["AverageNs"]) / 1e6
    return {"entities": E, "batch": B, "terms": S, "chunk_entities": chunk, "launches_per_call": launches, "combine_calls": int(row["Calls"]),
            "combine_average_ms": round(avg_ms, 5), "combine_min_ms": round(float(row["MinNs"]) / 1e6, 5),
            "combine_mean_bytes": int(mean_bytes), "combine_tb_per_s": round(mean_bytes / avg_ms / 1e9, 3), "guide_copy_tb_per_s": GUIDE_COPY_TB_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", default="65536,1000000")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "drin_link_edges_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--trace-child", default="")
    ap.add_argument("--no-link", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        E, B = a.trace_child.split(":")
        trace_child(int(E), int(B))
        return
    if a.child:
        E, B, precision = a.child.split(":")
        print("RESULT " + json.dumps(child(int(E), int(B), precision, a.steps, a.warmup, not a.no_link)), flush=True)
        return
    records, summary = [], {"workload": "drin_link_edges", "widths": list(WIDTHS), "k": K, "repeats": a.repeats,
                            "guide_copy_tb_per_s": GUIDE_COPY_TB_S, "predicted_products_over_single": round(sum(WIDTHS) / WIDTHS[0], 3)}
    for E in [int(v) for v in a.entities.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            for precision in a.precisions.split(","):
                runs = []
                for _ in range(a.repeats):   # a fresh process each (started, never replaced): allocator state, clocks and placement start over
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{E}:{B}:{precision}", "--steps", str(a.steps), "--warmup",
                           str(a.warmup)] + (["--no-link"] if a.no_link else [])
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        raise SystemExit(f"child {E}:{B}:{precision} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                    runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
                band = lambda key: {"min": round(min(v[key] for v in runs), 4), "median": round(statistics.median_low(v[key] for v in runs), 4),   # noqa: E731
                                    "max": round(max(v[key] for v in runs), 4)}
                timed = [k for k in runs[0] if k.endswith("_ms")]
                rec = {"workload": "drin_link_edges", "entities": E, "batch": B, "widths": list(WIDTHS), "k": K, "precision": precision,
                       "repeats": a.repeats, "chunk_entities": runs[0]["chunk_entities"], "chunks_per_call": runs[0]["chunks_per_call"],
                       "combine_bytes_per_call": runs[0]["combine_bytes_per_call"], **{k: band(k) for k in timed}}
                rec["sum_over_single"] = round(rec["sum_ms"]["median"] / rec["single_ms"]["median"], 3)
                rec["combine_call_tb_per_s"] = round(rec["combine_bytes_per_call"] / rec["combine_ms"]["median"] / 1e9, 3)
                records.append(rec)
                summary[f"E{E}_B{B}_{precision}"] = {**{k: rec[k]["median"] for k in timed}, "sum_over_single": rec["sum_over_single"],
                                                    "combine_call_tb_per_s": rec["combine_call_tb_per_s"]}
                print(json.dumps(rec), flush=True)
    if not a.no_trace:
        rec = dict(kernel_trace(1000000, 1024), workload="drin_link_edges_kernel_trace")
        records.append(rec)
        summary["trace_E1000000_B1024"] = {k: v for k, v in rec.items() if k not in ("workload", "entities", "batch")}
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
