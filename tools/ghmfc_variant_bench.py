"""Times GHMFC's transformer mention encoder on drin_amd.ghmfc_variants.VariantModel - the eval forward and one training step
(forward + backward, dropout 0.1: four draws per layer) - at the reference widths (D = 768, L = 128, H = 8, 8 layers, FFN 512),
N = 11 candidates, batch 64, max pool, in both precisions, with the per-class kernel split of drin_profile_*, the launches per
step, the host time between launches, and the same parameters through torch's own nn.TransformerEncoder (same process) for
scale - not a gate.  GPU only.

    python tools/ghmfc_variant_bench.py [--out profiles/ghmfc_variant_bench.jsonl] [--processes 3] [--iters 10] [--core fma]

--core mfma builds the model on the matrix-core attention core (drin_amd.attention.attention_core); its default output is
profiles/ghmfc_variant_bench_mfma.jsonl, and the record carries the core's name.

Every process is a fresh child (its own HIP context and code-object loads) under its own time limit.  The first line of the
output is the median over the processes, the lines behind it are the processes' own records.  The columns are those of
tools/ghmfc_train_bench.py: *_ms device-event time per call after a warm-up, *_wall_ms host wall-clock of the same loop with
one synchronisation at its end, *_enqueue_ms host wall-clock until the last launch call has returned.  attn_share is the share
of the step's kernel time spent in the softmax-attention core (eight self-attentions at Lq = Lk = 128): the figure a change of
that core is judged against.
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


def child(iters: int, core: str = "fma") -> dict:
    import torch
    import torch.nn.functional as F

    from drin_amd import _lib
    from drin_amd.ghmfc_variants import VariantConfig, VariantModel

    dev = "cuda"
    cfg = VariantConfig(num_candidates=CANDIDATES, mention_final_layer_name="transformer")
    D, L = cfg.embed_dim, cfg.mention_tokens
    gen = torch.Generator(device=dev).manual_seed(1)
    text = torch.randn(BATCH, L, D, device=dev, generator=gen)
    lengths = torch.randint(L // 2, L + 1, (BATCH, 1), device=dev, generator=gen)
    mask = (torch.arange(L, device=dev)[None, :] < lengths).long()
    begin = torch.ones(BATCH, dtype=torch.int64, device=dev)
    entity = torch.randn(BATCH, CANDIDATES, D, device=dev, generator=gen)
    batch = [text, mask, begin, begin + 2, 0, entity, 0, 0]
    G = torch.randn(BATCH, CANDIDATES, device=dev, generator=gen)

    def torch_forward(m):
        """the same parameters through torch's own encoder (its dropout in train(), its fused path under no_grad in eval())"""
        seq = m.mention_encoder.intermediate_layer.transformer(text, src_key_padding_mask=mask == 0)
        return F.cosine_similarity(seq.max(1).values[:, None, :], m.entity_encoder.final_layer(entity), dim=-1)

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

    record = {"batch": BATCH, "candidates": CANDIDATES, "dropout": DROPOUT, "layers": cfg.transformer_num_layers, "iters": iters,
              "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "core": core, "cases": {}}
    for precision in ("bf16x3", "f32"):
        torch.manual_seed(0)
        model = VariantModel(cfg, precision=precision, dropout=DROPOUT, seed=0, core=core).to(dev)
        params = list(model.parameters())

        def forward():
            return model(batch)

        def step():
            torch.autograd.grad(model(batch), params, G)

        def torch_eval():
            with torch.no_grad():
                return torch_forward(model)

        def torch_step():
            torch.autograd.grad(torch_forward(model), params, G)

        c = {}
        model.eval()
        c["eval_ms"], c["eval_wall_ms"], c["eval_enqueue_ms"] = timed(forward)
        c["torch_eval_ms"], c["torch_eval_wall_ms"], c["torch_eval_enqueue_ms"] = timed(torch_eval)
        c["classes_eval_ms"], c["launches_eval"] = classes(forward)
        model.train()
        c["step_ms"], c["step_wall_ms"], c["step_enqueue_ms"] = timed(step)
        c["torch_step_ms"], c["torch_step_wall_ms"], c["torch_step_enqueue_ms"] = timed(torch_step)
        c["classes_step_ms"], c["launches_step"] = classes(step)
        kernels = sum(c["classes_step_ms"].values())
        group = lambda names: sum(ms for k, ms in c["classes_step_ms"].items() if k in names)   # noqa: E731
        c["kernel_ms"] = kernels
        c["gemm_ms"], c["attn_ms"], c["norm_ms"] = group(("gemm", "gemm_x3", "gemm_planes")), group(("attn",)), group(("norm",))
        c["other_ms"] = kernels - c["gemm_ms"] - c["attn_ms"] - c["norm_ms"]
        c["attn_share"] = c["attn_ms"] / kernels
        eval_kernels = sum(c["classes_eval_ms"].values())
        c["eval_attn_share"] = c["classes_eval_ms"].get("attn", 0.0) / eval_kernels
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
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default   # noqa: E731
    core = opt("--core", "fma")
    if "--child" in argv:
        print("RECORD " + json.dumps(child(int(argv[argv.index("--iters") + 1]), core)), flush=True)
        return 0
    default_out = "ghmfc_variant_bench.jsonl" if core == "fma" else f"ghmfc_variant_bench_{core}.jsonl"
    out, processes, iters = opt("--out", os.path.join(REPO, "profiles", default_out)), int(opt("--processes", 3)), opt("--iters", "10")
    records = []
    for i in range(processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", iters, "--core", core], capture_output=True,
                           text=True, timeout=150)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1                                                   # nothing more is started after a failed process
        rec = json.loads(lines[-1][7:])
        rec["process"] = i
        records.append(rec)
        print(f"process {i}: done", flush=True)
    head = {k: records[0][k] for k in ("batch", "candidates", "dropout", "layers", "iters", "warmup", "device", "core")}
    head.update(summary=f"median of {processes} fresh processes", cases=median_of(records))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for rec in [head] + records:
            f.write(json.dumps(rec) + "\n")
    for precision, c in head["cases"].items():
        print(f"{precision:7s} eval {c['eval_ms']:7.3f} ms (torch {c['torch_eval_ms']:7.3f})  step {c['step_ms']:7.3f} ms (wall {c['step_wall_ms']:7.3f}, "
              f"torch {c['torch_step_ms']:7.3f})  kernels {c['kernel_ms']:7.3f} ms: gemm {c['gemm_ms']:.3f} attn {c['attn_ms']:.3f} norm {c['norm_ms']:.3f} "
              f"other {c['other_ms']:.3f}  attn share {c['attn_share']:.3f}  host enqueue {c['step_enqueue_ms']:.3f} ms  idle {c['idle_ms']:.3f} ms  "
              f"launches {c['launches_step']:.0f}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
