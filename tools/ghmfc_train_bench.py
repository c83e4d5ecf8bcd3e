"""Times one GHMFC training step of drin_amd.ghmfc_train.TrainableModel - forward + backward with attention dropout 0.1 -
at the reference widths (D = 768, R = 2048, L = 128, P = 49, H = 8), N = 11 candidates, batch 64, in both precisions, with
the per-class kernel split of drin_profile_*, the host time between launches, and the same model on plain torch
(nn.MultiheadAttention, F.layer_norm, ..., forward + backward, same weights, same process) for scale - not a gate.  GPU only.

    python tools/ghmfc_train_bench.py [--out profiles/ghmfc_train_bench.jsonl] [--processes 3] [--iters 10]

Every process is a fresh child (its own HIP context and code-object loads).  The first line of the output is the median over
the processes, the lines behind it are the processes' own records.  step_ms is device-event time per step after a warm-up,
step_wall_ms host wall-clock per step of the same loop with one synchronisation at its end, and step_enqueue_ms the host
wall-clock per step until the last launch call has returned (before that synchronisation): what the Python composition costs
the host.  While step_enqueue_ms < step_ms the host runs ahead of the device and the device is never idle between launches
(idle_ms = step_ms - kernel_ms, the step's device time not covered by kernels, says so directly); these two numbers argue for or
against a C-ABI launch sequence.  The class split comes from a separate profiled loop (the profile's events slow the host).
"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, CANDIDATES, DROPOUT, WARMUP = 64, 11, 0.1, 3


def child(iters: int) -> dict:
    import torch
    import torch.nn.functional as F
    from torch import nn

    from drin_amd import _lib
    from drin_amd.ghmfc import GhmfcConfig
    from drin_amd.ghmfc_train import TrainableModel

    dev = "cuda"
    cfg = GhmfcConfig(num_candidates=CANDIDATES)
    D, R, L, P, H = cfg.embed_dim, cfg.image_dim, cfg.mention_tokens, cfg.image_regions, cfg.num_heads
    gen = torch.Generator(device=dev).manual_seed(1)
    text = torch.randn(BATCH, L, D, device=dev, generator=gen)
    image = torch.randn(BATCH, P, R, device=dev, generator=gen).abs()
    lengths = torch.randint(L // 2, L + 1, (BATCH, 1), device=dev, generator=gen)
    mask = (torch.arange(L, device=dev)[None, :] < lengths).long()
    entity = torch.randn(BATCH, CANDIDATES, D, device=dev, generator=gen)
    batch = [text, mask, None, None, image, entity, 0, 0]
    G = torch.randn(BATCH, CANDIDATES, device=dev, generator=gen)

    def torch_forward(m):
        """the same model on plain torch: the parameters of `m` through nn.MultiheadAttention's own forward"""
        f = m.mention_encoder.intermediate_layer
        drop = mask == 0

        def cross(ca, a, drop_a, b, drop_b):
            x = nn.MultiheadAttention.forward(ca.a2b_attention, a, b, b, key_padding_mask=drop_b, need_weights=False)[0]
            ln = ca.layernorms
            x = ln[0](x)
            x = ln[1](ca.a2b_ffn(x) + x)
            y = nn.MultiheadAttention.forward(ca.b2a_attention, x, a, a, key_padding_mask=drop_a, need_weights=False)[0]
            y = ln[2](y)
            return ln[3](ca.b2a_ffn(y) + y).max(1).values

        t = F.gelu(f.text_linear(cross(f.t2v_attention, text, drop, image, None)))
        v = F.gelu(f.image_linear(cross(f.v2t_attention, image, None, text, drop)))
        s = torch.softmax(f.score_linear(torch.cat([t, v], 1)), 1)
        men = s[:, :1] * t + s[:, 1:] * v
        return F.cosine_similarity(men[:, None, :], m.entity_encoder.final_layer(entity), dim=-1)

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
        return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters, (enqueued - t0) * 1e3 / iters

    def classes(fn):
        _lib.profile_begin()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        return {k: ms / iters for k, (ms, n) in prof.items() if n}, sum(n for _ms, n in prof.values()) / iters

    record = {"batch": BATCH, "candidates": CANDIDATES, "dropout": DROPOUT, "iters": iters, "warmup": WARMUP,
              "device": torch.cuda.get_device_name(0), "cases": {}}
    for precision in ("bf16x3", "f32"):
        torch.manual_seed(0)
        model = TrainableModel(cfg, precision=precision, dropout=DROPOUT, seed=0).to(dev).train()
        params = list(model.parameters())

        def forward():
            return model(batch)

        def step():
            torch.autograd.grad(model(batch), params, G)

        def torch_step():
            torch.autograd.grad(torch_forward(model), params, G)

        c = {}
        c["fwd_ms"], c["fwd_wall_ms"], c["fwd_enqueue_ms"] = timed(forward)
        c["step_ms"], c["step_wall_ms"], c["step_enqueue_ms"] = timed(step)
        c["torch_step_ms"], c["torch_step_wall_ms"], c["torch_step_enqueue_ms"] = timed(torch_step)
        c["classes_fwd_ms"], c["launches_fwd"] = classes(forward)
        c["classes_step_ms"], c["launches_step"] = classes(step)
        kernels = sum(c["classes_step_ms"].values())
        group = lambda names: sum(ms for k, ms in c["classes_step_ms"].items() if k in names)   # noqa: E731
        c["kernel_ms"] = kernels
        c["gemm_ms"], c["attn_ms"], c["norm_ms"] = group(("gemm", "gemm_x3", "gemm_planes")), group(("attn",)), group(("norm",))
        c["other_ms"] = kernels - c["gemm_ms"] - c["attn_ms"] - c["norm_ms"]
        c["norm_share"] = c["norm_ms"] / kernels
        c["idle_ms"] = c["step_ms"] - kernels
        c["enqueue_over_step"] = c["step_enqueue_ms"] / c["step_ms"]
        c["torch_over_ours"] = c["torch_step_ms"] / c["step_ms"]
        record["cases"][precision] = c
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
    out, processes, iters = opt("--out", os.path.join(REPO, "profiles", "ghmfc_train_bench.jsonl")), int(opt("--processes", 3)), opt("--iters", "10")
    records = []
    for i in range(processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", iters], capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1                                                   # nothing more is started after a failed process
        rec = json.loads(lines[-1][7:])
        rec["process"] = i
        records.append(rec)
        print(f"process {i}: done", flush=True)
    head = {k: records[0][k] for k in ("batch", "candidates", "dropout", "iters", "warmup", "device")}
    head.update(summary=f"median of {processes} fresh processes", cases=median_of(records))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in [head] + records:
            f.write(json.dumps(rec) + "\n")
    for precision, c in head["cases"].items():
        print(f"{precision:7s} step {c['step_ms']:7.3f} ms (wall {c['step_wall_ms']:7.3f})  torch {c['torch_step_ms']:7.3f} ms  kernels {c['kernel_ms']:7.3f} ms: "
              f"gemm {c['gemm_ms']:.3f} attn {c['attn_ms']:.3f} norm {c['norm_ms']:.3f} other {c['other_ms']:.3f}  "
              f"norm share {c['norm_share']:.3f}  host enqueue {c['step_enqueue_ms']:.3f} ms  idle {c['idle_ms']:.3f} ms  launches {c['launches_step']:.0f}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
