"""Time the two forms of the WikiMEL entity token pool on one GPU: `drin_entity_token_mean` and the max
form of `drin_entity_token_pool` on the same seeded inputs in the same process, alternating, and the per-entity cache builder
with either pooling (`drin_ghmfc_entity_rows`, `drin_ghmfc_entity_rows_ex`) over a table.

  pool   pairs = 64 * 101, T = 64, D = 768, ntok ~ U{4..64}: the candidates of a batch of 64 WikiMEL mentions
  rows   a table of E = 65 536 entities, the same T, D and token counts, split-bf16 product

Each case runs in `--repeats` FRESH processes; inside a process `--rounds` rounds alternate the two forms, each timed with device
events around `--reps` back-to-back launches (a window well above a fraction of a second per form and process), and the process's
figure is the median round.  Reported: median and spread (min, max) over the processes, and bytes/s over the COMPULSORY bytes -
the rows inside the slices 1 : ntok - 1, computed from the token counts here, plus the written rows.

The acceptance comparison: the max form's median must lie inside the mean's process-to-process spread widened by 10 % of the
mean's median (the extra NaN compare and select per element).  Recorded as `max_inside_band`, not tuned.  Writes `--out`
(profiles/entity_pool_bench.jsonl): a summary line keyed by case, then one line per case.

usage:  python tools/entity_pool_bench.py [--repeats 3] [--out profiles/entity_pool_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
T, D = 64, 768
CASES = {"pool": dict(pairs=64 * 101, reps=3000, rounds=5), "rows": dict(pairs=65536, reps=200, rounds=5)}


def compulsory_bytes(ntok, width: int) -> int:
    """the token rows inside 1 : ntok - 1 (ntok >= 3 here), the mask and the written rows"""
    return int(sum(int(n) - 2 for n in ntok)) * width * 4 + len(ntok) * (T * 8 + width * 4)


def child(case: str, reps: int, rounds: int) -> dict:
    import torch

    from drin_amd import _lib
    from drin_amd._lib import _ptr, _stream
    lib, dev = _lib.load(), torch.device("cuda")
    pairs = CASES[case]["pairs"]
    g = torch.Generator(device="cuda").manual_seed(0)
    feat = torch.randn(pairs, T, D, device=dev, generator=g)
    ntok = torch.randint(4, T + 1, (pairs,), device=dev, generator=g)
    mask = (torch.arange(T, device=dev)[None, :] < ntok[:, None]).to(torch.int64)
    out = {name: torch.empty(pairs, D, device=dev) for name in ("mean", "max")}
    st = _stream(dev)
    if case == "pool":
        forms = {"mean": lambda: lib.drin_entity_token_mean(_ptr(feat), _ptr(mask), _ptr(out["mean"]), pairs, T, D, st),
                 "max": lambda: lib.drin_entity_token_pool(_ptr(feat), _ptr(mask), _ptr(out["max"]), pairs, T, D, _lib.POOL_MAX, st)}
    else:
        w, b = torch.randn(D, D, device=dev, generator=g) / D ** 0.5, torch.randn(D, device=dev, generator=g)
        nbytes = lib.drin_ghmfc_entity_rows_workspace_bytes(pairs, T, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        prec = _lib.PREC_BF16X3
        forms = {"mean": lambda: lib.drin_ghmfc_entity_rows(_ptr(feat), _ptr(mask), pairs, T, D, _ptr(w), _ptr(b), prec, _ptr(out["mean"]),
                                                            _ptr(ws), nbytes, st),
                 "max": lambda: lib.drin_ghmfc_entity_rows_ex(_ptr(feat), _ptr(mask), pairs, T, D, _lib.POOL_MAX, _ptr(w), _ptr(b), prec,
                                                              _ptr(out["max"]), _ptr(ws), nbytes, st)}
    for fn in forms.values():                                          # warm-ups: code objects, clocks
        for _ in range(max(reps // 10, 3)):
            _lib.check(fn())
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():                                  # alternating: both forms see the same machine
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                _lib.check(fn())
            z.record()
            z.synchronize()
            ms[name].append(a.elapsed_time(z) / reps)
    return {"mean_ms": statistics.median(ms["mean"]), "max_ms": statistics.median(ms["max"]), "rounds_ms": ms,
            "window_s": {name: sum(v) * reps / 1e3 for name, v in ms.items()}, "compulsory_bytes": compulsory_bytes(ntok.tolist(), D),
            "outputs_finite": bool(torch.isfinite(out["mean"]).all() and torch.isfinite(out["max"]).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pool,rows")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "entity_pool_bench.jsonl"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        c = CASES[a.child]
        print("RESULT " + json.dumps(child(a.child, c["reps"], c["rounds"])), flush=True)
        return
    records = []
    for case in a.cases.split(","):
        runs = []
        for _ in range(a.repeats):   # a fresh process each: allocator state, clocks and placement start over
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"child {case} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        band = lambda key: {"min": round(min(v[key] for v in runs), 5), "median": round(statistics.median(v[key] for v in runs), 5),   # noqa: E731
                            "max": round(max(v[key] for v in runs), 5)}
        mean, mx = band("mean_ms"), band("max_ms")
        nbytes = runs[0]["compulsory_bytes"]
        lo, hi = mean["min"] - 0.1 * mean["median"], mean["max"] + 0.1 * mean["median"]
        rec = {"workload": "entity_pool", "case": case, "pairs": CASES[case]["pairs"], "tokens": T, "width": D, "repeats": a.repeats,
               "reps": CASES[case]["reps"], "rounds": CASES[case]["rounds"], "mean_ms": mean, "max_ms": mx,
               "window_s": {k: round(min(v["window_s"][k] for v in runs), 3) for k in ("mean", "max")},
               "max_over_mean": round(mx["median"] / mean["median"], 4), "band_ms": [round(lo, 5), round(hi, 5)],
               "max_inside_band": lo <= mx["median"] <= hi, "outputs_finite": all(v["outputs_finite"] for v in runs)}
        if case == "pool":
            rec.update(compulsory_bytes=nbytes, mean_gb_per_s=round(nbytes / mean["median"] / 1e6, 1),
                       max_gb_per_s=round(nbytes / mx["median"] / 1e6, 1))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps({"workload": "entity_pool", **{rec["case"]: rec for rec in records}}) + "\n")   # the summary line
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
