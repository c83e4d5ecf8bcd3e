"""Time linking against bf16-STORED tables beside the same tables as fp32: synthetic tables at the widths of
the three edge terms (768 text, 512 + 512 CLIP), k = N = 101, E in {65 536, 1 000 000}, B in {64, 1024}, both precisions.  The fp32
tables are the exactly-widened copies of the bf16 ones and the two ALTERNATE inside one process, call by call; each configuration
runs in `--repeats` FRESH child processes, each under its own time limit (`--limit` seconds), and the tool stops at the first one
that fails.  The figures are medians over the processes.  Per configuration and storage (`f32` | `bf16`):
* `topk_*_ms`, `sum_*_ms`: CALL times (a host clock over back-to-back calls that ends in one synchronise) of `table_topk` at width
  768 (`drin_table_topk` | `drin_table_topk_ex`) and of `table_topk_sum` with the three terms;
* from `drin_profile_*` (device time per kernel class) over `table_topk` calls: `product_*_ms` - the GEMM classes: on bf16 rows the
  plane route in bf16x3 precision, the widen route's product in f32 precision - `split_ms` (the `gcn` class of the bf16 call: the
  once-per-call split of the padded mentions into planes; 0 on the widen route) and `widen_ms` (the `edge` class of the bf16 call
  minus the fp32 call's: `k_widen_rows` over every chunk; reported as 0 on the plane route, where no such launch exists and the
  difference is noise);
* the widen route in bf16x3 precision, measured directly at a width the plane kernel misses (776 = 768 + 8; bf16x3 runs only):
  `w776_topk_*_ms` call times and `w776_product_*_ms`, `w776_widen_ms` as above - beside `product_bf16_ms` at 768 (the plane
  route) this is what the choice between the two routes rests on; `w776_route_ms` = product + widening of the bf16 call;
* `rescore_*_ms`: `cosine_rows_indexed` on kp = 128 listed rows per mention, width 768, and `rescore_*_tb_s`: the listed rows' bytes
  (2 or 4 per element) over that time;
* `edges_*_ms`: `drin_cross_modal_edges(_ex)` for N = 101 candidates per mention at C = 512, and `edges_*_tb_s` likewise.
A record, not a gate.  Writes `--out` (profiles/link_bf16_bench.jsonl): a summary line, then one line per configuration.

usage:  python tools/link_bf16_bench.py [--entities 65536,1000000] [--batches 64,1024] [--precisions bf16x3,f32] [--repeats 3] [--limit 240]
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
WIDTHS, K, KP, CLIP = (768, 512, 512), 101, 128, 512
WIDE = 776                                                     # % 8 == 0, % 32 != 0: bf16 rows of this width take the widen route


def child(E: int, B: int, precision: str, steps: int, warmup: int) -> dict:
    import torch

    from drin_amd import _lib
    from drin_amd._lib import _ptr, _stream
    from drin_amd.ghmfc_table import cosine_rows_indexed, row_inv_norms, table_topk, table_topk_sum
    lib, dev, eps = _lib.load(), torch.device("cuda"), 1e-8
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    stored = [rn(E, d).to(torch.bfloat16) for d in WIDTHS]
    tables = {"bf16": stored, "f32": [t.float() for t in stored]}       # the fp32 tables: the exactly-widened copies
    xs = [rn(B, d) for d in WIDTHS]
    invs = [row_inv_norms(t, eps) for t in stored]
    listed = torch.randint(0, E, (B, KP), device=dev, generator=g)
    cand = torch.randint(0, E, (B, K), device=dev, generator=g)
    miet, mtei = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)

    def edges(kind):
        t_text, t_image = tables[kind][1], tables[kind][2]
        _lib.check(lib.drin_cross_modal_edges_ex(_ptr(xs[2]), _ptr(xs[1]), _ptr(t_text), _ptr(t_image), _lib.FEAT_BF16 if kind == "bf16" else _lib.FEAT_F32,
                                                 _ptr(cand), E, B, K, CLIP, 100.0, eps, _ptr(miet), _ptr(mtei), None, _stream(dev)))

    calls = {
        "topk": lambda kind: table_topk(xs[0], tables[kind][0], invs[0], K, eps, precision),
        "sum": lambda kind: table_topk_sum([(x, t, i, 1.0) for x, t, i in zip(xs, tables[kind], invs)], K, eps, precision),
        "rescore": lambda kind: cosine_rows_indexed(xs[0], tables[kind][0], listed, eps, None),
        "edges": edges,
    }
    kinds = ("f32", "bf16")
    out = {}
    for name in ("topk", "sum"):                                        # call times: the two storages alternate, call by call
        spent = {kind: 0.0 for kind in kinds}
        for step in range(warmup + steps):
            for kind in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls[name](kind)
                torch.cuda.synchronize()
                if step >= warmup:
                    spent[kind] += time.perf_counter() - t0
        for kind in kinds:
            out[f"{name}_{kind}_ms"] = spent[kind] * 1e3 / steps
    by_class = {}
    for name in ("topk", "rescore", "edges"):                           # device time per kernel class, alternating as well
        acc = {kind: {} for kind in kinds}
        for kind in kinds:                                              # a kernel's first launch in a process is not its rate
            calls[name](kind)
        for _ in range(steps):
            for kind in kinds:
                torch.cuda.synchronize()
                _lib.profile_begin()
                calls[name](kind)
                torch.cuda.synchronize()
                for cls, (ms, _n) in _lib.profile_end().items():
                    acc[kind][cls] = acc[kind].get(cls, 0.0) + ms / steps
        by_class[name] = acc
    for kind in kinds:
        out[f"product_{kind}_ms"] = sum(v for c, v in by_class["topk"][kind].items() if c.startswith("gemm"))
        out[f"rescore_{kind}_ms"] = by_class["rescore"][kind]["edge"]
        out[f"edges_{kind}_ms"] = by_class["edges"][kind]["edge"]
        width = 2 if kind == "bf16" else 4
        out[f"rescore_{kind}_tb_s"] = B * KP * WIDTHS[0] * width / out[f"rescore_{kind}_ms"] / 1e9
        out[f"edges_{kind}_tb_s"] = 2 * B * K * CLIP * width / out[f"edges_{kind}_ms"] / 1e9
    out["split_ms"] = by_class["topk"]["bf16"].get("gcn", 0.0)
    out["plane_route"] = int(by_class["topk"]["bf16"].get("gemm_planes", 0.0) > 0)
    out["widen_ms"] = 0.0 if out["plane_route"] else by_class["topk"]["bf16"]["edge"] - by_class["topk"]["f32"]["edge"]
    out["table_row_bytes_bf16"] = E * WIDTHS[0] * 2
    if precision == "bf16x3":                                           # the widen route in this precision: a width the plane kernel misses
        del tables, stored
        odd = rn(E, WIDE).to(torch.bfloat16)
        both = {"bf16": odd, "f32": odd.float()}
        x_odd, inv_odd = rn(B, WIDE), row_inv_norms(odd, eps)
        call = lambda kind: table_topk(x_odd, both[kind], inv_odd, K, eps, precision)   # noqa: E731
        spent, acc = {kind: 0.0 for kind in kinds}, {kind: {} for kind in kinds}
        for step in range(warmup + steps):
            for kind in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(kind)
                torch.cuda.synchronize()
                if step >= warmup:
                    spent[kind] += time.perf_counter() - t0
        for _ in range(steps):
            for kind in kinds:
                torch.cuda.synchronize()
                _lib.profile_begin()
                call(kind)
                torch.cuda.synchronize()
                for cls, (ms, _n) in _lib.profile_end().items():
                    acc[kind][cls] = acc[kind].get(cls, 0.0) + ms / steps
        if acc["bf16"].get("gemm_planes", 0.0) > 0:
            raise RuntimeError(f"width {WIDE} was meant to take the widen route")
        for kind in kinds:
            out[f"w776_topk_{kind}_ms"] = spent[kind] * 1e3 / steps
            out[f"w776_product_{kind}_ms"] = sum(v for c, v in acc[kind].items() if c.startswith("gemm"))
        out["w776_widen_ms"] = acc["bf16"]["edge"] - acc["f32"]["edge"]
        out["w776_route_ms"] = out["w776_product_bf16_ms"] + out["w776_widen_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", default="65536,1000000")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--precisions", default="bf16x3,f32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one GPU process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "link_bf16_bench.jsonl"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        E, B, precision = a.child.split(":")
        print("RESULT " + json.dumps(child(int(E), int(B), precision, a.steps, a.warmup)), flush=True)
        return
    records, summary = [], {"workload": "link_bf16", "widths": list(WIDTHS), "k": K, "repeats": a.repeats}
    for E in [int(v) for v in a.entities.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            for precision in a.precisions.split(","):
                runs = []
                for _ in range(a.repeats):   # a fresh process each (started, never replaced), under its own time limit; the first failure ends the tool
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{E}:{B}:{precision}", "--steps", str(a.steps), "--warmup", str(a.warmup)]
                    try:
                        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                    except subprocess.TimeoutExpired:
                        raise SystemExit(f"child {E}:{B}:{precision} ran past its {a.limit} s: stopping")
                    if r.returncode != 0:
                        raise SystemExit(f"child {E}:{B}:{precision} failed ({r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                    runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
                rec = {"workload": "link_bf16", "entities": E, "batch": B, "widths": list(WIDTHS), "k": K, "precision": precision, "repeats": a.repeats,
                       "plane_route": runs[0]["plane_route"]}
                for key in runs[0]:
                    if key.endswith("_ms") or key.endswith("_tb_s"):
                        rec[key] = round(statistics.median_low(v[key] for v in runs), 4)
                rec["topk_bf16_over_f32"] = round(rec["topk_bf16_ms"] / rec["topk_f32_ms"], 3)
                rec["sum_bf16_over_f32"] = round(rec["sum_bf16_ms"] / rec["sum_f32_ms"], 3)
                rec["product_bf16_over_f32"] = round(rec["product_bf16_ms"] / rec["product_f32_ms"], 3)
                rec["product_bf16_table_tb_s"] = round(runs[0]["table_row_bytes_bf16"] / rec["product_bf16_ms"] / 1e9, 3)
                records.append(rec)
                summary[f"E{E}_B{B}_{precision}"] = {k: v for k, v in rec.items() if k not in ("workload", "entities", "batch", "widths", "k", "precision", "repeats")}
                print(json.dumps(rec), flush=True)
            x3 = summary.get(f"E{E}_B{B}_bf16x3")
            if x3:   # the two routes side by side in bf16x3: the plane route at 768 over the widen route at 776 (1 % more columns)
                x3["plane_over_widen_route"] = round((x3["product_bf16_ms"] + x3["split_ms"]) / x3["w776_route_ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
