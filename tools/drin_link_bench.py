"""Time DRIN behind a first stage on one GPU (`Model.link`): synthetic pooled-text tables at the reference
widths (D = 768, R = 2048), CLIP rows of C = 512, N = 101 candidates, E in {65 536, 1 000 000}, B in {64, 1024}, both precisions,
the per-entity cache on; each configuration in `--repeats` FRESH processes (median and spread over them).  Per configuration,
milliseconds of the four stages of `Model.link(queries=, rows=)` alone - the cosine first stage (`drin_table_topk`, the pooled
text rows as its table), the cross-modal edges (`drin_cross_modal_edges`), the scoring (`drin_forward_cached`) and the rank
(`drin_rank_rows`) - and of the whole call.  These are CALL times: a host clock over back-to-back calls that ends in one
synchronise, launch overhead included.  The same two matrices (before their scale) produced by two calls of
`drin_cosine_rows_indexed_fwd` are timed alternating with the cross-modal call in the same process; `edges_call_tb_per_s` is the
call's gathered bytes (two table rows per pair) over its call time.
The KERNEL's time comes from a run of its own under `rocprofv3 --kernel-trace --stats` (the program behind `--`), B = 1024 at both
table sizes: `k_cross_modal_edges` and, for the two-call route, `k_cosine_gather`, each over 40 launches that rotate through four
lists of uniformly random candidate rows (1.7 GB of gathered rows between two uses of a list).  The kernel's gathered bytes over
that time stand next to the 5.7 TB/s the microarchitecture guide measures for 2.3 KB rows gathered into registers.
A record, not a gate.  Writes `--out` (profiles/drin_link_bench.jsonl): a summary line, then one line per configuration.

usage:  python tools/drin_link_bench.py [--entities 65536,1000000] [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3] [--no-trace]
"""
from __future__ import annotations

import argparse
import csv
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
CLIP, K, GUIDE_TB_S = 512, 10, 5.7


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


def child(E: int, B: int, precision: str, steps: int, warmup: int) -> dict:
    import torch

    from drin_amd import _lib, synth
    from drin_amd._lib import _ptr, _stream
    from drin_amd.config import DrinConfig
    from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk
    from drin_amd.model import EntityTable, IndexedBatch, Model
    lib, dev = _lib.load(), torch.device("cuda")
    cfg = DrinConfig(num_candidates_data=100)                          # WikiDiverse layout (pooled entity text) with N = 101
    N, D, R = cfg.num_candidates_model, cfg.bert_embed_dim, cfg.resnet_embed_dim
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    table = EntityTable(rn(E, D), None, rn(E, R), rn(E, 1, R), torch.rand(E, 1, device=dev, generator=g))
    table.set_clip(rn(E, CLIP), rn(E, CLIP)).enable_cache()
    model = Model(cfg, precision=precision).to(dev).eval()
    mention = synth.make_device_batch(cfg.with_(num_candidates_data=0), B, 3, dev)[:7]
    clip_image, clip_text, queries = rn(B, CLIP), rn(B, CLIP), rn(B, D)
    rows, eps, scale = table.text, cfg.cosine_eps, cfg.clip_logit_scale
    inv = row_inv_norms(rows, eps)
    cand = table_topk(queries, rows, inv, N, eps, precision).rows
    first_ms = timeit(lambda: table_topk(queries, rows, inv, N, eps, precision), steps, warmup)
    miet, mtei = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)

    def edges():
        _lib.check(lib.drin_cross_modal_edges(_ptr(clip_image), _ptr(clip_text), _ptr(table.clip_text), _ptr(table.clip_image), _ptr(cand), E, B, N,
                                              CLIP, scale, eps, _ptr(miet), _ptr(mtei), None, _stream(dev)))

    def two_calls():
        for x, t, out in ((clip_image, table.clip_text, miet), (clip_text, table.clip_image, mtei)):
            _lib.check(lib.drin_cosine_rows_indexed_fwd(_ptr(x), _ptr(t), _ptr(cand), E, _ptr(out), B, N, CLIP, eps, None, _stream(dev)))

    one, two = [], []
    for _ in range(5):                                                 # alternating: both meet the same clocks and cache state
        one.append(timeit(edges, 4 * steps, warmup))
        two.append(timeit(two_calls, 4 * steps, warmup))
    edges()                                                            # (the alternation's last writer was the two-call route)
    factor = torch.tensor(scale, device=dev)
    same = bool(torch.equal(miet, factor * cosine_rows_indexed(clip_image, table.clip_text, cand, eps, None))
                and torch.equal(mtei, factor * cosine_rows_indexed(clip_text, table.clip_image, cand, eps, None)))
    batch = IndexedBatch.from_clip(mention, table, cand, clip_image, clip_text, model=model)
    with torch.no_grad():
        scores = model(batch)                                          # builds the folds and the per-entity cache
        score_ms = timeit(lambda: model(batch), steps, warmup)
    out_s, out_r = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int64, device=dev)
    rank_ms = timeit(lambda: _lib.check(lib.drin_rank_rows(_ptr(scores), _ptr(cand), B, N, K, _ptr(out_s), _ptr(out_r), None, _stream(dev))),
                     4 * steps, warmup)
    link_ms = timeit(lambda: model.link(mention, table, K, clip_image, clip_text, queries=queries, rows=rows), steps, warmup)
    model.check_indices()
    return {"first_stage_ms": first_ms, "edges_ms": statistics.median(one), "two_call_ms": statistics.median(two), "score_ms": score_ms,
            "rank_ms": rank_ms, "link_ms": link_ms, "edges_equal_scaled_two_call_bits": same, "cache_format": table.cache_format_used}


TRACE_LISTS, TRACE_LAUNCHES = 4, 40


def trace_child(E: int, B: int) -> None:
    """what the kernel trace runs: the cross-modal kernel, then the two-call route, TRACE_LAUNCHES times each after 3 warm-up
    launches, over TRACE_LISTS lists of uniformly random candidate rows in turn"""
    import torch

    from drin_amd import _lib
    from drin_amd._lib import _ptr, _stream
    lib, dev, N = _lib.load(), torch.device("cuda"), 101
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    t_text, t_image, m_image, m_text = rn(E, CLIP), rn(E, CLIP), rn(B, CLIP), rn(B, CLIP)
    lists = [torch.randint(0, E, (B, N), device=dev, generator=g) for _ in range(TRACE_LISTS)]
    miet, mtei = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    for i in range(3 + TRACE_LAUNCHES):
        _lib.check(lib.drin_cross_modal_edges(_ptr(m_image), _ptr(m_text), _ptr(t_text), _ptr(t_image), _ptr(lists[i % TRACE_LISTS]), E, B, N,
                                              CLIP, 100.0, 1e-8, _ptr(miet), _ptr(mtei), None, _stream(dev)))
    for i in range(3 + TRACE_LAUNCHES):
        for x, t, out in ((m_image, t_text, miet), (m_text, t_image, mtei)):
            _lib.check(lib.drin_cosine_rows_indexed_fwd(_ptr(x), _ptr(t), _ptr(lists[i % TRACE_LISTS]), E, _ptr(out), B, N, CLIP, 1e-8, None,
                                                        _stream(dev)))
    torch.cuda.synchronize()


def kernel_trace(E: int, B: int) -> dict:
    """One run of `trace_child` under rocprofv3's kernel trace: per kernel the average over ALL its launches of that run (warm-up
    included; `calls` says how many) and the fastest one.  The two-call route's time is two launches of k_cosine_gather."""
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
    out = {"entities": E, "batch": B, "lists": TRACE_LISTS, "gathered_bytes": int(2.0 * B * 101 * CLIP * 4)}
    for name, key in (("k_cross_modal_edges", "edges"), ("k_cosine_gather", "gather")):
        hit = [x for x in rows if name in x["Name"]]
        if not hit:
            raise RuntimeError(f"no {name} row in the kernel trace")
        row = max(hit, key=lambda x: int(x["Calls"]))
        out[f"{key}_calls"] = int(row["Calls"])
        out[f"{key}_average_ms"] = round(float(row["AverageNs"]) / 1e6, 5)
        out[f"{key}_min_ms"] = round(float(row["MinNs"]) / 1e6, 5)
    out["two_call_kernels_ms"] = round(2 * out["gather_average_ms"], 5)
    out["edges_kernel_tb_per_s"] = round(out["gathered_bytes"] / out["edges_average_ms"] / 1e9, 3)
    out["two_call_kernels_tb_per_s"] = round(out["gathered_bytes"] / out["two_call_kernels_ms"] / 1e9, 3)
    out["two_call_over_edges_kernel"] = round(out["two_call_kernels_ms"] / out["edges_average_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", default="65536,1000000")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "drin_link_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--trace-child", default="")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        E, B = a.trace_child.split(":")
        trace_child(int(E), int(B))
        return
    if a.child:
        E, B, precision = a.child.split(":")
        print("RESULT " + json.dumps(child(int(E), int(B), precision, a.steps, a.warmup)), flush=True)
        return
    records, summary = [], {"workload": "drin_link", "clip_width": CLIP, "candidates": 101, "k": K, "repeats": a.repeats,
                            "guide_gather_tb_per_s": GUIDE_TB_S}
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
                band = lambda key: {"min": round(min(v[key] for v in runs), 4), "median": round(statistics.median_low(v[key] for v in runs), 4),   # noqa: E731
                                    "max": round(max(v[key] for v in runs), 4)}
                edges, two = band("edges_ms"), band("two_call_ms")
                gathered = 2.0 * B * 101 * CLIP * 4                   # two table rows per pair
                spread = max(edges["max"] - edges["min"], two["max"] - two["min"])
                rec = {"workload": "drin_link", "entities": E, "batch": B, "candidates": 101, "clip_width": CLIP, "k": K, "precision": precision,
                       "repeats": a.repeats, "cache_format": runs[0]["cache_format"], "first_stage_ms": band("first_stage_ms"), "edges_ms": edges,
                       "score_ms": band("score_ms"), "rank_ms": band("rank_ms"), "link_ms": band("link_ms"), "two_call_ms": two,
                       "edges_gathered_bytes": int(gathered), "edges_call_tb_per_s": round(gathered / edges["median"] / 1e9, 3),
                       "guide_gather_tb_per_s": GUIDE_TB_S, "two_call_over_edges": round(two["median"] / edges["median"], 3),
                       "process_spread_ms": round(spread, 4), "edges_gain_exceeds_spread": two["median"] - edges["median"] > spread,
                       "edges_equal_scaled_two_call_bits": all(v["edges_equal_scaled_two_call_bits"] for v in runs),
                       "mentions_per_s": round(B / band("link_ms")["median"] * 1e3, 1)}
                records.append(rec)
                summary[f"E{E}_B{B}_{precision}"] = {key: (rec[key]["median"] if isinstance(rec[key], dict) else rec[key])
                                                    for key in ("first_stage_ms", "edges_ms", "two_call_ms", "score_ms", "rank_ms", "link_ms",
                                                                "edges_call_tb_per_s", "two_call_over_edges", "edges_gain_exceeds_spread")}
                print(json.dumps(rec), flush=True)
    if not a.no_trace:
        for E in [int(v) for v in a.entities.split(",")]:
            rec = dict(kernel_trace(E, 1024), workload="drin_link_kernel_trace", guide_gather_tb_per_s=GUIDE_TB_S)
            records.append(rec)
            summary[f"trace_E{E}_B1024"] = {k: v for k, v in rec.items() if k not in ("workload", "entities", "batch")}
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
