"""Times DRIN with its other mention encoders (drin_amd.drin_encoders.EncoderModel) - scoring (eval: the folded path) and one
training step (forward + backward, transformer_dropout 0.1: four draws per layer) - at the reference widths, WikiDiverse shape
(D = 768, R = 2048, L = 128, N = 11), batch 64, for the four new combinations ("none" | "transformer") x ("avg extract" |
"max pool"), both precisions and, for the transformer, both attention cores; with the per-class kernel split of drin_profile_*,
the launches per step, the host enqueue time, and the two head kernels' own share (class "pool" of a training step holds
k_mention_rows, k_mention_rows_bwd and the region mean).  Record only: nothing exists to compare against.  GPU only.

    python tools/drin_encoder_bench.py [--out profiles/drin_encoder_bench.jsonl] [--processes 3] [--iters 10]

Every process is a fresh child (its own HIP context and code-object loads) under its own time limit.  The first line of the
output is the median over the processes, the lines behind it are the processes' own records.  *_ms: device-event time per call
after a warm-up; *_enqueue_ms: host wall-clock until the last launch call has returned.
"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, WARMUP = 64, 3
COMBINATIONS = [("none", "avg extract", "fma"), ("none", "max pool", "fma"), ("transformer", "avg extract", "fma"),
                ("transformer", "max pool", "fma"), ("transformer", "max pool", "mfma")]


def child(iters: int) -> dict:
    import torch

    from drin_amd import _lib, synth
    from drin_amd.config import DrinConfig
    from drin_amd.model import Model

    dev = "cuda"
    record = {"batch": BATCH, "iters": iters, "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "cases": {}}

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        enqueued = time.perf_counter()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, (enqueued - t0) * 1e3 / iters

    def classes(fn):
        _lib.profile_begin()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        return {k: ms / iters for k, (ms, n) in prof.items() if n}, sum(n for _ms, n in prof.values()) / iters

    for layer, representation, core in COMBINATIONS:
        cfg = DrinConfig(mention_final_layer_name=layer, mention_final_representation=representation)
        batch = [t.to(dev) for t in synth.make_batch(cfg, BATCH, 11)[:14]]
        G = torch.randn(BATCH, cfg.num_candidates_model, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        for precision in ("bf16x3", "f32"):
            torch.manual_seed(0)
            model = Model(cfg, precision=precision, core=core, seed=0).to(dev)
            params = [p for p in model.parameters()]

            def forward():
                return model(batch)

            def step():
                torch.autograd.grad(model(batch), params, G, allow_unused=True)

            c = {}
            model.eval()
            c["eval_ms"], c["eval_enqueue_ms"] = timed(forward)
            c["eval_path"] = model.last_path
            c["classes_eval_ms"], c["launches_eval"] = classes(forward)
            model.train()
            c["step_ms"], c["step_enqueue_ms"] = timed(step)
            c["classes_step_ms"], c["launches_step"] = classes(step)
            c["kernel_ms"] = sum(c["classes_step_ms"].values())
            record["cases"][f"{layer}/{representation}/{core}/{precision}"] = c
    return record


def median_of(records):
    def walk(nodes):
        if isinstance(nodes[0], dict):
            return {k: walk([n[k] for n in nodes if k in n]) for k in nodes[0]}
        if isinstance(nodes[0], str):
            return nodes[0]
        return statistics.median(nodes)
    return walk([r["cases"] for r in records])


def main(argv):
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default   # noqa: E731
    if "--child" in argv:
        print("RECORD " + json.dumps(child(int(argv[argv.index("--iters") + 1]))), flush=True)
        return 0
    out = opt("--out", os.path.join(REPO, "profiles", "drin_encoder_bench.jsonl"))
    processes, iters = int(opt("--processes", 3)), opt("--iters", "10")
    records = []
    for i in range(processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", iters], capture_output=True, text=True,
                           timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1                                                   # nothing more is started after a failed process
        rec = json.loads(lines[-1][7:])
        rec["process"] = i
        records.append(rec)
        print(f"process {i}: done", flush=True)
    head = {k: records[0][k] for k in ("batch", "iters", "warmup", "device")}
    head.update(summary=f"median of {processes} fresh processes", cases=median_of(records))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in [head] + records:
            f.write(json.dumps(rec) + "\n")
    for name, c in head["cases"].items():
        split = " ".join(f"{k} {ms:.3f}" for k, ms in sorted(c["classes_step_ms"].items()))
        print(f"{name:38s} eval {c['eval_ms']:7.3f} ms ({c['eval_path']}, {c['launches_eval']:.0f} launches)  step {c['step_ms']:7.3f} ms  "
              f"kernels {c['kernel_ms']:7.3f} ms: {split}  launches {c['launches_step']:.0f}  host enqueue {c['step_enqueue_ms']:.3f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
