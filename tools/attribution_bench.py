"""Cost of `Model.attribute` against the route a caller has without it - detached leaves, `backward()`,
`(x * x.grad).sum(-1)`; in table form through `batch.gathered()` - at WikiMEL N = 101, T = 64, B = 64 and 512, as a 14-sequence
and as an `IndexedBatch` over a 65 536-entity table.  The two routes alternate in one process; device-synchronised milliseconds
per call after warm-up and `torch.cuda.max_memory_allocated` above the resident batch, over three fresh processes per case.  One
run of its own under `rocprofv3 --kernel-trace --stats` (the program behind `--`) times `k_token_attribution`; its algorithmic
bytes - kept token rows + mask + gradient row + output, from the masks - over that time are quoted as a share of 8 TB/s.

    python tools/attribution_bench.py [--out profiles/attribution_bench.jsonl] [--processes 3] [--no-trace]
    python tools/attribution_bench.py --child --form seq|table --batch B [--steps 10] [--warmup 3] [--route both|attribute]

The first line of the output file is the summary (medians over the processes, the kernel figures); one line per process follows.
Yardstick from before the method existed: `k_token_block_bwd` writes the 1.27 GB fp32 gradient block of B = 64 in 0.219 ms
 - the block `attribute()` never forms.
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FLOAT = (0, 4, 5, 6, 7, 9, 10, 11, 12, 13)            # float tensors of the 14-sequence
ENTITIES = 65536
HBM_BYTES_PER_S = 8e12
CHILD_TIMEOUT_S = 600


def make_case(form: str, B: int):
    import torch
    from drin_amd import synth
    from drin_amd.config import wikimel_config
    from drin_amd.model import EntityTable, IndexedBatch
    cfg = wikimel_config()
    if form == "seq":
        return cfg, synth.make_device_batch(cfg, B, 3, "cuda")
    tab = synth.make_device_batch(cfg.with_(num_candidates_data=ENTITIES - 1), 1, 5, "cuda")
    men = synth.make_device_batch(cfg.with_(max_entity_attr_token_len=3), B, 3, "cuda")
    cand = torch.randint(0, ENTITIES, (B, cfg.num_candidates_model), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    table = EntityTable(*(tab[i][0].contiguous() for i in (7, 8, 9, 10, 11)))
    return cfg, IndexedBatch(men[:7], table, cand, men[12], men[13])


def todays_route(model, batch, G):
    """What a caller writes without `Model.attribute`: every float tensor a leaf, one backward, gradient x input by torch."""
    from drin_amd.model import IndexedBatch
    seq = batch.gathered() if isinstance(batch, IndexedBatch) else list(batch[:14])
    x = list(seq)
    for i in FLOAT:
        x[i] = x[i].detach().requires_grad_(True)
    (model(x) * G).sum().backward()
    return [(x[i] * x[i].grad).sum(-1) if x[i].dim() > 2 else x[i] * x[i].grad for i in FLOAT]


def kept_bytes(batch, D: int) -> int:
    """Algorithmic bytes of k_token_attribution on this batch: the kept token rows (fp32), the mask rows, one gradient row and one
    output row per pair."""
    from drin_amd.model import IndexedBatch
    mask = batch.table.mask[batch.candidates] if isinstance(batch, IndexedBatch) else batch[8]
    T = mask.shape[-1]
    ntok = mask.sum(-1)
    stop = ntok - 1
    stop = (stop + (stop < 0) * T).clamp(0, T)
    kept = int((stop - 1).clamp(min=0).sum())
    pairs = ntok.numel()
    return kept * D * 4 + pairs * (T * 8 + D * 4 + T * 4)


def child(a) -> dict:
    import torch
    from drin_amd import synth
    from drin_amd.model import Model
    cfg, batch = make_case(a.form, a.batch)
    model = Model(cfg).cuda().requires_grad_(False)
    model.load_state_dict(synth.make_state_dict(cfg, 7))
    B, N = a.batch, cfg.num_candidates_model
    G = torch.randn(B, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    routes = {"attribute": lambda: model.attribute(batch, weights=G)}
    if a.route == "both":
        routes["today"] = lambda: todays_route(model, batch, G)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    ms = {k: [] for k in routes}
    peak = {k: 0 for k in routes}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for k in range(a.warmup + a.steps):                    # the routes alternate: neither gets the warmer half of the process
        for name, fn in routes.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ev[0].record()
            out = fn()
            ev[1].record()
            torch.cuda.synchronize()
            del out
            if k >= a.warmup:
                ms[name].append(ev[0].elapsed_time(ev[1]))
                peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - resident)
    rec = {"form": a.form, "batch": B, "steps": a.steps, "resident_bytes": resident,
           "block_bytes": B * N * cfg.max_entity_attr_token_len * cfg.bert_embed_dim * 4,
           "token_kernel_bytes": kept_bytes(batch, cfg.bert_embed_dim)}
    for name in routes:
        rec[f"{name}_ms"] = round(statistics.median(ms[name]), 4)
        rec[f"{name}_peak_bytes"] = int(peak[name])
    return rec


def run_child(form: str, B: int, extra=(), prefix=()) -> dict:
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", "--form", form, "--batch", str(B)] + list(extra)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:                 # a hung child ends the tool, it does not hang it
        raise RuntimeError(f"{' '.join(cmd)} did not finish in {CHILD_TIMEOUT_S} s") from e
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_trace(form: str, B: int) -> dict:
    """One run of the attribute() route alone under rocprofv3's kernel trace: the average of k_token_attribution over ALL its
    launches of that run - `calls` says how many: the 3 warm-up calls and the 10 timed ones - and the fastest one (`min_ms`)."""
    with tempfile.TemporaryDirectory() as tmp:
        rec = run_child(form, B, ["--route", "attribute", "--steps", "10", "--warmup", "3"],
                        prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"])
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [r for r in csv.DictReader(f) if "k_token_attribution" in r["Name"]]
    if not rows:
        raise RuntimeError("no k_token_attribution row in the kernel trace")
    row = max(rows, key=lambda r: int(r["Calls"]))
    avg_ms = float(row["AverageNs"]) / 1e6
    rate = rec["token_kernel_bytes"] / (avg_ms * 1e-3)
    return {"form": form, "batch": B, "kernel": "k_token_attribution", "calls": int(row["Calls"]), "average_ms": round(avg_ms, 5),
            "min_ms": round(float(row["MinNs"]) / 1e6, 5), "algorithmic_bytes": rec["token_kernel_bytes"],
            "bytes_per_s": round(rate, -9), "share_of_8_tb_s": round(rate / HBM_BYTES_PER_S, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--form", choices=("seq", "table"), default="seq")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", choices=("both", "attribute"), default="both")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attribution_bench.jsonl"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a)))
        return
    records, summary = [], {"geometry": "wikimel N=101 T=64 D=768 R=2048", "table_entities": ENTITIES, "processes": a.processes,
                            "yardstick": {"kernel": "k_token_block_bwd", "ms": 0.219, "bytes": 64 * 101 * 64 * 768 * 4, "batch": 64}}
    for form in ("seq", "table"):
        for B in (64, 512):
            runs = [run_child(form, B, ["--steps", str(a.steps), "--warmup", str(a.warmup)]) for _ in range(a.processes)]
            records += runs
            med = lambda key: statistics.median(r[key] for r in runs)  # noqa: E731
            summary[f"{form}_b{B}"] = {
                "attribute_ms": med("attribute_ms"), "today_ms": med("today_ms"),
                "attribute_peak_mb": round(med("attribute_peak_bytes") / 1e6, 1), "today_peak_mb": round(med("today_peak_bytes") / 1e6, 1),
                "block_mb": round(runs[0]["block_bytes"] / 1e6, 1), "speedup": round(med("today_ms") / med("attribute_ms"), 2)}
            print(form, B, json.dumps(summary[f"{form}_b{B}"]), flush=True)
    if not a.no_trace:
        for form in ("seq", "table"):
            summary[f"trace_{form}_b64"] = kernel_trace(form, 64)
            print("trace", form, json.dumps(summary[f"trace_{form}_b64"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
        for r in records:
            f.write(json.dumps(r) + "\n")
    print(a.out)


if __name__ == "__main__":
    main()
