"""Times the two softmax-attention cores - "fma" (drin_attention_train_fwd / drin_attention_bwd) and "mfma"
(drin_attention_mfma_fwd / drin_attention_mfma_bwd) - at GHMFC's four attention shapes, batch 64, 8 heads, core only: the
entry points on projected operands, forward and backward (delta + dq + dkv) apart.  GPU only.

    python tools/attention_core_bench.py [--out profiles/attention_core_bench.jsonl] [--processes 3] [--window-ms 300]

Both cores run in the same process from the same build, alternating window by window after every shape and path has been
warmed.  A window is a loop of calls between two device events, sized per path so that it lasts about --window-ms; a
process reports the median of its three windows per (shape, core, direction), and beside it profiled_*_ms: the kernel
time of profiler class attn per call over one more window (drin_profile_*: events around every launch), which is how
tools/attention_train_bench.py measured core_fwd_ms and core_bwd_ms - the figure to hold against that file.  Every process
is a fresh child (its own HIP context and code-object loads).  The first line of the output holds, per shape and core, the median and the min - max spread
over the processes, the algorithmic FLOPs (4 B H Lq Lk dh forward, 10 B H Lq Lk dh backward) and bytes (every operand and
result once) and the TF/s they give, and the verdict of DESIGN.md section 21: the mfma median below the fma median by more
than the larger of the two spreads.  The lines behind it are the processes' own records.
Text keys (128 of them) carry a mask of random lengths in [64, 128], image keys (49) none, as in GHMFC.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, HEADS = 64, 8
SHAPES = [(128, 49, 96), (128, 128, 96), (49, 128, 256), (49, 49, 256)]   # (Lq, Lk, dh)
CORES = ("fma", "mfma")
WARMUP, WINDOWS = 10, 3


def case_name(Lq, Lk, dh):
    return f"q{Lq}_k{Lk}_dh{dh}"


def work(Lq, Lk, dh):
    """algorithmic FLOPs and bytes of one forward / one backward"""
    B, H, E = BATCH, HEADS, HEADS * dh
    pairs = B * H * Lq * Lk * dh
    rows_q, rows_k, stats = B * Lq * E, B * Lk * E, B * H * Lq
    return {"fwd_flops": 4 * pairs, "bwd_flops": 10 * pairs, "fwd_bytes": 4 * (2 * rows_q + 2 * rows_k + stats),
            "bwd_bytes": 4 * (4 * rows_q + 4 * rows_k + 3 * stats)}


def child(window_ms: float) -> dict:
    import torch

    from drin_amd import _lib

    dev, lib = "cuda", _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    paths = {}
    for Lq, Lk, dh in SHAPES:
        B, H, E = BATCH, HEADS, HEADS * dh
        gen = torch.Generator(device=dev).manual_seed(Lq + Lk + dh)
        q, k, v, dout = (torch.randn(B * n, E, device=dev, generator=gen) for n in (Lq, Lk, Lk, Lq))
        mask = None
        if Lk == 128:
            lengths = torch.randint(64, 129, (B, 1), device=dev, generator=gen)
            mask = (torch.arange(Lk, device=dev)[None, :] < lengths).to(torch.int64)
        out, dq = torch.empty(B * Lq, E, device=dev), torch.empty(B * Lq, E, device=dev)
        dk, dv = torch.empty(B * Lk, E, device=dev), torch.empty(B * Lk, E, device=dev)
        lse, delta = torch.empty(B, H, Lq, device=dev), torch.empty(B, H, Lq, device=dev)
        fwd_args = (ptr(q), E, ptr(k), E, ptr(v), E, ptr(mask), ptr(out), E, ptr(lse), B, H, Lq, Lk, dh)
        bwd_args = (ptr(q), E, ptr(k), E, ptr(v), E, ptr(mask), ptr(out), E, ptr(lse), ptr(dout), E, ptr(dq), E, ptr(dk), E, ptr(dv), E,
                    ptr(delta), B, H, Lq, Lk, dh)
        keepalive = (q, k, v, dout, mask, out, dq, dk, dv, lse, delta)
        calls = {"fma": (lambda a=fwd_args: _lib.check(lib.drin_attention_train_fwd(*a, stream)),
                         lambda a=bwd_args: _lib.check(lib.drin_attention_bwd(*a, stream))),
                 "mfma": (lambda a=fwd_args: _lib.check(lib.drin_attention_mfma_fwd(*a, 0.0, 0, 0, stream)),
                          lambda a=bwd_args: _lib.check(lib.drin_attention_mfma_bwd(*a, 0.0, 0, 0, stream)))}
        for core in CORES:                                             # each core's backward reads its own forward's out, lse
            for direction, fn in zip(("fwd", "bwd"), calls[core]):
                paths[(case_name(Lq, Lk, dh), core, direction)] = (fn, calls[core][0], keepalive)
    counts = {}
    for key, (fn, fwd, _keep) in paths.items():                        # warm every shape and path, and size its window
        fwd()
        per_call = window(fn, WARMUP)
        counts[key] = max(20, int(window_ms / max(per_call, 1e-3)))
    record = {"batch": BATCH, "heads": HEADS, "window_ms": window_ms, "windows": WINDOWS, "device": torch.cuda.get_device_name(0),
              "cases": {}}
    for Lq, Lk, dh in SHAPES:
        name = case_name(Lq, Lk, dh)
        times = {(core, d): [] for core in CORES for d in ("fwd", "bwd")}
        for _ in range(WINDOWS):
            for direction in ("fwd", "bwd"):
                for core in CORES:                                     # alternating: fma window, mfma window
                    fn, fwd, _keep = paths[(name, core, direction)]
                    fwd()                                              # this core's own out and lse under its backward
                    times[(core, direction)].append(window(fn, counts[(name, core, direction)]))
        record["cases"][name] = {core: {f"core_{d}_ms": statistics.median(times[(core, d)]) for d in ("fwd", "bwd")} |
                                 {f"calls_{d}": counts[(name, core, d)] for d in ("fwd", "bwd")} for core in CORES}
        for core in CORES:
            for direction in ("fwd", "bwd"):
                fn, fwd, _keep = paths[(name, core, direction)]
                fwd()
                torch.cuda.synchronize()
                _lib.profile_begin()
                for _ in range(100):
                    fn()
                torch.cuda.synchronize()
                record["cases"][name][core][f"profiled_{direction}_ms"] = _lib.profile_end()["attn"][0] / 100
    return record


def summarise(records):
    cases = {}
    for Lq, Lk, dh in SHAPES:
        name, w = case_name(Lq, Lk, dh), work(Lq, Lk, dh)
        c = dict(w)
        for core in CORES:
            c[core] = {}
            for d in ("fwd", "bwd"):
                xs = [r["cases"][name][core][f"core_{d}_ms"] for r in records]
                med = statistics.median(xs)
                c[core][f"profiled_{d}_ms"] = statistics.median(r["cases"][name][core][f"profiled_{d}_ms"] for r in records)
                c[core].update({f"core_{d}_ms": med, f"core_{d}_ms_min": min(xs), f"core_{d}_ms_max": max(xs),
                                f"core_{d}_tflops": w[f"{d}_flops"] / (med * 1e-3) / 1e12,
                                f"core_{d}_gbytes_per_s": w[f"{d}_bytes"] / (med * 1e-3) / 1e9})
        for d in ("fwd", "bwd"):
            spread = max(c[core][f"core_{d}_ms_max"] - c[core][f"core_{d}_ms_min"] for core in CORES)
            gap = c["fma"][f"core_{d}_ms"] - c["mfma"][f"core_{d}_ms"]
            c[f"{d}_fma_over_mfma"] = c["fma"][f"core_{d}_ms"] / c["mfma"][f"core_{d}_ms"]
            c[f"{d}_mfma_faster_beyond_spread"] = bool(gap > spread)
        cases[name] = c
    return cases


def main(argv):
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default   # noqa: E731
    window_ms = float(opt("--window-ms", 300))
    if "--child" in argv:
        print("RECORD " + json.dumps(child(window_ms)), flush=True)
        return 0
    out, processes = opt("--out", os.path.join(REPO, "profiles", "attention_core_bench.jsonl")), int(opt("--processes", 3))
    records = []
    for i in range(processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--window-ms", str(window_ms)], capture_output=True,
                           text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1                                                   # nothing more is started after a failed process
        rec = json.loads(lines[-1][7:])
        rec["process"] = i
        records.append(rec)
        print(f"process {i}: done", flush=True)
    head = {k: records[0][k] for k in ("batch", "heads", "window_ms", "windows", "device")}
    head.update(summary=f"median and min - max over {processes} fresh processes", cases=summarise(records))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in [head] + records:
            f.write(json.dumps(rec) + "\n")
    for name, c in head["cases"].items():
        for d in ("fwd", "bwd"):
            f_, m_ = c["fma"], c["mfma"]
            print(f"{name:18s} {d}  fma {f_[f'core_{d}_ms']:7.4f} ms [{f_[f'core_{d}_ms_min']:.4f}, {f_[f'core_{d}_ms_max']:.4f}] "
                  f"{f_[f'core_{d}_tflops']:6.1f} TF/s   mfma {m_[f'core_{d}_ms']:7.4f} ms [{m_[f'core_{d}_ms_min']:.4f}, "
                  f"{m_[f'core_{d}_ms_max']:.4f}] {m_[f'core_{d}_tflops']:6.1f} TF/s   x {c[f'{d}_fma_over_mfma']:.2f}  "
                  f"beyond spread: {c[f'{d}_mfma_faster_beyond_spread']}   profiled fma {f_[f'profiled_{d}_ms']:.4f} mfma "
                  f"{m_[f'profiled_{d}_ms']:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
