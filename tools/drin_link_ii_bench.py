"""Time the image-image edge as the fourth term of DRIN's first stage on one GPU (`drin_table_topk_sum_forms`, `drin_object_rows`;
DESIGN.md section 36): synthetic tables at the widths of the four edges (768 text, 512 + 512 CLIP, 2048 object rows), k = N = 101,
E in {65 536, 1 000 000}, B in {64, 1024}, both precisions; each configuration in `--repeats` FRESH child processes, each under its
own time limit, and a failed one ends the run.  Per configuration:
* `three_ms` / `four_ms`: CALL times (a host clock over back-to-back calls that ends in one synchronise) of `table_topk_sum` with the
  three cosines and with the RATIO term behind them, alternating in one process;
* per call, from `drin_profile_*` (device time per kernel class): `fourth_product_ms` (the GEMM classes of the four-term call minus
  the three-term call's), `combine_ms` (`drin_topk_combine_forms` on blocks of the call's chunk, times the chunks of a call) and
  `rescore_ms` (`drin_ratio_rows_indexed_fwd` on kp rows per mention);
* `mention_rows_ms`: `drin_object_rows` of the batch's `Km = 3` objects, a per-call cost of `Model.link`.
`k_object_rows` over the TABLE comes from a run of its own under `rocprofv3 --kernel-trace --stats` (the program behind `--`):
`E * Ke * R * 4` bytes over its time, next to the 8 TB/s of the data sheet.
`--guard-lib PATH`: the one guard.  The THREE-term call (`forms = NULL`: no new code on its path) is timed on this tree's library
and on another build of the library (the parent commit's), alternating, each in `--repeats` fresh processes, at E = 1 M / B = 1024
and E = 65 536 / B = 64; medians and the spread the other build shows against itself are recorded.  A record, not a gate.  Writes
`--out` (profiles/drin_link_ii_bench.jsonl): a summary line, then one line per configuration.

usage:  python tools/drin_link_ii_bench.py [--entities 65536,1000000] [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3]
                                           [--no-trace] [--guard-lib /path/to/the/other/libdrin_hip.so]
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
WIDTHS, R, KM, KE, K, KP, SHEET_TB_S = (768, 512, 512), 2048, 3, 1, 101, 128, 8.0
BUDGET = 256 << 20
CHILD_LIMIT = 600                                                        # seconds: the time limit of every child process


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


def cosine_terms(E: int, B: int, dev, g):
    import torch

    from drin_amd.table_ops import row_inv_norms
    tables = [torch.randn(E, d, device=dev, generator=g) for d in WIDTHS]
    return [(torch.randn(B, d, device=dev, generator=g), t, row_inv_norms(t, 1e-8), 1.0) for d, t in zip(WIDTHS, tables)]


def child(E: int, B: int, precision: str, steps: int, warmup: int) -> dict:
    import torch

    from drin_amd import _lib
    from drin_amd._lib import _ptr, _stream
    from drin_amd.table_ops import RatioTerm, object_rows, ratio_rows_indexed, table_topk_sum
    lib, dev, eps, miei_eps, S = _lib.load(), torch.device("cuda"), 1e-8, 1e-9, len(WIDTHS) + 1
    g = torch.Generator(device=dev).manual_seed(7)
    terms = cosine_terms(E, B, dev, g)
    eobj, es = torch.randn(E, KE, R, device=dev, generator=g), torch.rand(E, KE, device=dev, generator=g) + 0.05
    u, T = object_rows(eobj, es, eps)
    del eobj
    mobj, ms = torch.randn(B, KM, R, device=dev, generator=g), torch.rand(B, KM, device=dev, generator=g) + 0.05
    q, Sm = object_rows(mobj, ms, eps)
    ratio = RatioTerm(q, Sm, u, T, 1.0, miei_eps)
    three = lambda: table_topk_sum(terms, K, eps, precision)   # noqa: E731
    four = lambda: table_topk_sum(terms + [ratio], K, eps, precision)   # noqa: E731
    out = {"three_ms": [], "four_ms": []}
    for _ in range(2):                                                  # alternating in one process
        out["three_ms"].append(timeit(three, steps, warmup))
        out["four_ms"].append(timeit(four, steps, warmup))
    out = {k: min(v) for k, v in out.items()}
    gemm = lambda by_class: sum(v for k, v in by_class.items() if k.startswith("gemm"))   # noqa: E731
    out["fourth_product_ms"] = gemm(profiled(four, steps)) - gemm(profiled(three, steps))
    Bp, chunk = (B + 3) // 4 * 4, default_chunk(E, B, S)
    blocks, scales = [torch.randn(chunk, Bp, device=dev, generator=g) for _ in range(S)], [torch.rand(Bp, device=dev, generator=g) + 0.5 for _ in range(S)]
    forms = (_lib.DrinTopkFormC * S)()
    forms[S - 1].form, forms[S - 1].x_mass, forms[S - 1].row_mass, forms[S - 1].eps = _lib.TOPK_RATIO, scales[S - 1].data_ptr(), T.data_ptr(), miei_eps
    arrays = [(C.c_void_p * S)(*[t.data_ptr() for t in ts]) for ts in (blocks, [t[2][:chunk] for t in terms] + [T], scales)]
    weights = (C.c_float * S)(*[1.0] * S)
    combine = lambda: _lib.check(lib.drin_topk_combine_forms(*arrays, weights, forms, S, Bp, B, chunk, _ptr(blocks[0]), _stream(dev)))   # noqa: E731
    out["chunk_entities"], out["chunks_per_call"] = chunk, -(-E // chunk)
    out["combine_ms"] = profiled(combine, 4 * steps)["edge"] * E / chunk
    listed = torch.randint(0, E, (B, KP), device=dev, generator=g)
    out["rescore_ms"] = profiled(lambda: ratio_rows_indexed(q, Sm, u, T, listed, miei_eps, None), steps)["edge"]
    out["mention_rows_ms"] = profiled(lambda: object_rows(mobj, ms, eps), steps)["pool"]
    return out


def guard_child(E: int, B: int, precision: str, steps: int, warmup: int) -> dict:
    """the three-term call alone, on whichever library DRIN_LIB_PATH names"""
    import torch

    from drin_amd import _lib
    from drin_amd.table_ops import table_topk_sum
    if os.environ.get("DRIN_LIB_PATH"):                                 # a build from before the newest entry points: bind what it exports
        other = C.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.EXPORTS if not hasattr(other, n)]:
            del _lib.EXPORTS[name]
    dev = torch.device("cuda")
    terms = cosine_terms(E, B, dev, torch.Generator(device=dev).manual_seed(7))
    return {"three_ms": timeit(lambda: table_topk_sum(terms, K, 1e-8, precision), steps, warmup)}


TRACE_CALLS = 6


def trace_child(E: int) -> None:
    import torch

    from drin_amd.table_ops import object_rows
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(7)
    eobj, es = torch.randn(E, KE, R, device=dev, generator=g), torch.rand(E, KE, device=dev, generator=g) + 0.05
    for _ in range(TRACE_CALLS):
        object_rows(eobj, es, 1e-8)
    torch.cuda.synchronize()


def kernel_trace(E: int) -> dict:
    """One run of `trace_child` under rocprofv3's kernel trace: k_object_rows' average over its launches of that run"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", str(E)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=CHILD_LIMIT)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
    hit = [x for x in rows if "k_object_rows" in x["Name"]]
    if not hit:
        raise RuntimeError("no k_object_rows row in the kernel trace")
    row = max(hit, key=lambda x: int(x["Calls"]))
    avg_ms, nbytes = float(row["AverageNs"]) / 1e6, E * KE * R * 4
    return {"entities": E, "objects_per_entity": KE, "width": R, "calls": int(row["Calls"]), "object_rows_average_ms": round(avg_ms, 5),
            "object_rows_min_ms": round(float(row["MinNs"]) / 1e6, 5), "object_rows_bytes": nbytes,
            "object_rows_tb_per_s": round(nbytes / avg_ms / 1e9, 3), "share_of_sheet": round(nbytes / avg_ms / 1e9 / SHEET_TB_S, 3),
            "sheet_tb_per_s": SHEET_TB_S}


def run_child(flag: str, spec: str, a, env=None) -> dict:
    """a fresh process (started, never replaced) under its own time limit; a failed one ends the run"""
    cmd = [sys.executable, os.path.abspath(__file__), flag, spec, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT, env=env)
    if r.returncode != 0:
        raise SystemExit(f"child {flag} {spec} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", default="65536,1000000")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "drin_link_ii_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--guard-child", default="")
    ap.add_argument("--trace-child", default="")
    ap.add_argument("--guard-lib", default="")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child(int(a.trace_child))
        return
    for spec, fn in ((a.child, child), (a.guard_child, guard_child)):
        if spec:
            E, B, precision = spec.split(":")
            print("RESULT " + json.dumps(fn(int(E), int(B), precision, a.steps, a.warmup)), flush=True)
            return
    records, summary = [], {"workload": "drin_link_ii", "widths": list(WIDTHS) + [R], "k": K, "repeats": a.repeats, "sheet_tb_per_s": SHEET_TB_S,
                            "predicted_four_over_three": round((sum(WIDTHS) + R) / sum(WIDTHS), 3)}
    for E in [int(v) for v in a.entities.split(",") if v]:
        for B in [int(v) for v in a.batches.split(",") if v]:
            for precision in a.precisions.split(","):
                runs = [run_child("--child", f"{E}:{B}:{precision}", a) for _ in range(a.repeats)]
                band = lambda key: {"min": round(min(v[key] for v in runs), 4), "median": round(statistics.median_low(v[key] for v in runs), 4),   # noqa: E731
                                    "max": round(max(v[key] for v in runs), 4)}
                timed = [k for k in runs[0] if k.endswith("_ms")]
                rec = {"workload": "drin_link_ii", "entities": E, "batch": B, "widths": list(WIDTHS) + [R], "k": K, "precision": precision,
                       "repeats": a.repeats, "chunk_entities": runs[0]["chunk_entities"], "chunks_per_call": runs[0]["chunks_per_call"],
                       **{k: band(k) for k in timed}}
                rec["four_over_three"] = round(rec["four_ms"]["median"] / rec["three_ms"]["median"], 3)
                records.append(rec)
                summary[f"E{E}_B{B}_{precision}"] = {**{k: rec[k]["median"] for k in timed}, "four_over_three": rec["four_over_three"]}
                print(json.dumps(rec), flush=True)
    if a.guard_lib:
        for E, B in ((1000000, 1024), (65536, 64)):
            for precision in a.precisions.split(","):
                runs = {"tree": [], "other": []}
                for _ in range(a.repeats):                              # alternating: the other build, then this tree's
                    for which in ("other", "tree"):
                        env = dict(os.environ, DRIN_LIB_PATH=os.path.abspath(a.guard_lib)) if which == "other" else None
                        runs[which].append(run_child("--guard-child", f"{E}:{B}:{precision}", a, env)["three_ms"])
                rec = {"workload": "drin_link_ii_guard", "entities": E, "batch": B, "precision": precision, "repeats": a.repeats,
                       "tree_three_ms": [round(v, 4) for v in runs["tree"]], "other_three_ms": [round(v, 4) for v in runs["other"]],
                       "tree_median_ms": round(statistics.median_low(runs["tree"]), 4), "other_median_ms": round(statistics.median_low(runs["other"]), 4),
                       "other_spread_ms": round(max(runs["other"]) - min(runs["other"]), 4)}
                rec["difference_ms"] = round(rec["tree_median_ms"] - rec["other_median_ms"], 4)
                rec["inside_the_spread"] = rec["difference_ms"] <= rec["other_spread_ms"]
                records.append(rec)
                summary[f"guard_E{E}_B{B}_{precision}"] = {k: rec[k] for k in ("tree_median_ms", "other_median_ms", "other_spread_ms",
                                                                               "difference_ms", "inside_the_spread")}
                print(json.dumps(rec), flush=True)
    if not a.no_trace:
        rec = dict(kernel_trace(1000000), workload="drin_link_ii_kernel_trace")
        records.append(rec)
        summary["trace_E1000000"] = {k: v for k, v in rec.items() if k not in ("workload", "entities")}
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
