"""Times drin_amd.attention.MultiheadAttention - forward, and forward + backward - at GHMFC's four attention shapes, batch 64,
in both precisions, with the per-class kernel split of drin_profile_* and plain nn.MultiheadAttention (forward + backward,
same weights, same process) for scale.  GPU only.

    python tools/attention_train_bench.py [--out profiles/attention_train_bench.jsonl] [--processes 3] [--iters 20]

Every process is a fresh child (its own HIP context and code-object loads).  The first line of the output is the median over
the processes, the lines behind it are the processes' own records.  Times are device-event milliseconds per call after a
warm-up of every timed path; the class split comes from a separate profiled loop (the profile's events slow the host).
Text keys (128 of them) carry a padding mask of random lengths in [64, 128], image keys (49) none, as in GHMFC.
"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, HEADS = 64, 8
SHAPES = [(128, 49, 768, 2048), (128, 128, 768, 768), (49, 128, 2048, 768), (49, 49, 2048, 2048)]   # (Lq, Lk, E, kdim)
WARMUP = 5


def case_name(Lq, Lk, E, kdim):
    return f"q{Lq}_k{Lk}_e{E}_kd{kdim}"


def child(iters: int) -> dict:
    import torch
    from torch import nn

    from drin_amd import _lib
    from drin_amd.attention import MultiheadAttention

    dev = "cuda"

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def classes(fn):
        _lib.profile_begin()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return {k: ms / iters for k, (ms, n) in _lib.profile_end().items() if n}

    record = {"batch": BATCH, "heads": HEADS, "iters": iters, "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "cases": {}}
    for precision in ("bf16x3", "f32"):
        record["cases"][precision] = {}
        for Lq, Lk, E, kdim in SHAPES:
            gen = torch.Generator(device=dev).manual_seed(Lq + Lk + E)
            kd = None if kdim == E else kdim
            torch.manual_seed(0)
            mha = MultiheadAttention(E, HEADS, kdim=kd, vdim=kd, batch_first=True, precision=precision).to(dev)
            ref = nn.MultiheadAttention(E, HEADS, kdim=kd, vdim=kd, batch_first=True).to(dev)
            ref.load_state_dict(mha.state_dict())
            query = torch.randn(BATCH, Lq, E, device=dev, generator=gen, requires_grad=True)
            key = torch.randn(BATCH, Lk, kdim, device=dev, generator=gen, requires_grad=True)
            proj = torch.randn(BATCH, Lq, E, device=dev, generator=gen)
            mask = None
            if Lk == 128:
                lengths = torch.randint(64, 129, (BATCH, 1), device=dev, generator=gen)
                mask = torch.arange(Lk, device=dev)[None, :] >= lengths
            leaves = [query, key] + list(mha.parameters())
            ref_leaves = [query, key] + list(ref.parameters())

            def forward(m=mha):
                return m(query, key, key, key_padding_mask=mask, need_weights=False)[0]

            def forward_backward(m=mha, wrt=leaves):
                torch.autograd.grad(forward(m), wrt, proj)

            c = {"fwd_ms": timed(forward), "fwd_bwd_ms": timed(forward_backward),
                 "torch_fwd_bwd_ms": timed(lambda: forward_backward(ref, ref_leaves))}
            c["classes_fwd_ms"] = classes(forward)
            c["classes_fwd_bwd_ms"] = classes(forward_backward)
            core_fwd = c["classes_fwd_ms"]["attn"]
            c["core_fwd_ms"], c["core_bwd_ms"] = core_fwd, c["classes_fwd_bwd_ms"]["attn"] - core_fwd
            c["core_bwd_over_fwd"] = c["core_bwd_ms"] / core_fwd
            c["torch_over_ours_fwd_bwd"] = c["torch_fwd_bwd_ms"] / c["fwd_bwd_ms"]
            record["cases"][precision][case_name(Lq, Lk, E, kdim)] = c
    return record


def median_of(records):
    def walk(nodes):
        if isinstance(nodes[0], dict):
            return {k: walk([n[k] for n in nodes if k in n]) for k in nodes[0]}
        return statistics.median(nodes)
    return walk([r["cases"] for r in records])


def main(argv):
    if "--child" in argv:
        print("RECORD " + json.dumps(child(int(argv[argv.index("--iters") + 1]))), flush=True)
        return 0
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default   # noqa: E731
    out, processes, iters = opt("--out", os.path.join(REPO, "profiles", "attention_train_bench.jsonl")), int(opt("--processes", 3)), opt("--iters", "20")
    records = []
    for i in range(processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", iters], capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1                                                   # nothing more is started after a failed process
        rec = json.loads(lines[-1][7:])
        rec["process"] = i
        records.append(rec)
        print(f"process {i}: done", flush=True)
    head = {k: records[0][k] for k in ("batch", "heads", "iters", "warmup", "device")}
    head.update(summary=f"median of {processes} fresh processes", cases=median_of(records))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in [head] + records:
            f.write(json.dumps(rec) + "\n")
    for precision, cases in head["cases"].items():
        for name, c in cases.items():
            print(f"{precision:7s} {name:24s} fwd {c['fwd_ms']:7.3f} ms  fwd+bwd {c['fwd_bwd_ms']:7.3f} ms  torch fwd+bwd {c['torch_fwd_bwd_ms']:7.3f} ms  "
                  f"core fwd {c['core_fwd_ms']:6.3f} bwd {c['core_bwd_ms']:6.3f} ms (x {c['core_bwd_over_fwd']:.2f})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
