"""IN-PROCESS grid over the side schedule of x_i C_i^T (fused_forward.hip: folded_plan) on ONE resident batch: G persistent
workgroups take the first f of the row tiles on the library's side stream, under the entity stream pass.  Needs a PROBE build of
the library, whose plan is set between calls (the shipped library has constants and no setter):

    DRIN_EXTRA_FLAGS=-DDRIN_SIDE_PROBE python -m drin_amd.build --variant probe
    DRIN_LIB_PATH=drin_amd/libdrin_hip_probe.so python tools/probes/image_overlap_ab.py [--features bf16] [--batch B] [--sweep]

Per cell: the library's per-class kernel times (each kernel's events on the stream it runs on: `stream` is k_entity_stream on
256 - G CUs, `gemm_x3` / `gemm_planes` holds side part + rest of the contraction), the wall step time by events on the caller's
stream, and whether the scores are the serial call's bits.  --sweep: serial against one cell (--cell G,f) over call sizes."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from drin_amd import _lib, synth  # noqa: E402
from drin_amd.config import wikimel_config  # noqa: E402
from drin_amd.model import Model  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


bf16 = arg("--features", "f32") == "bf16"
dev = torch.device("cuda", 0)
cfg = wikimel_config()
sd = synth.make_state_dict(cfg, 7)
lib = _lib.load()
set_plan = lib.drin_probe_side_plan        # AttributeError: not a probe build
set_plan.restype, set_plan.argtypes = None, [_lib.C.c_int, _lib.C.c_int]
model = Model(cfg, precision="bf16x3").to(dev).eval()
model.load_state_dict(sd)


def measure(batch, G, permille, steps=10):
    set_plan(G, permille)
    with torch.no_grad():
        for _ in range(3):
            out = model(batch)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            out = model(batch)
        t1.record()
        torch.cuda.synchronize()
        wall = t0.elapsed_time(t1) / steps
        _lib.profile_begin(1 << 12)
        for _ in range(8):
            out = model(batch)
        prof = _lib.profile_end()
        torch.cuda.synchronize()
    return wall, {k: v[0] / 8 for k, v in prof.items() if v[0]}, out.clone()


def line(tag, wall, prof, same):
    print(f"{tag:22s} step {wall:7.3f} ms  same bits {same}  " + "  ".join(f"{k} {v:.3f}" for k, v in prof.items()), flush=True)


def make(B):
    return synth.make_device_batch(cfg, B, 100, dev, dtype=torch.bfloat16 if bf16 else torch.float32)[:14]


if "--sweep" in sys.argv:
    G, f = (int(x) for x in arg("--cell", "64,450").split(","))
    for B in (128, 256, 512, 1024, 2048, 4096):
        batch = make(B)
        for rep in range(2):
            w0, p0, ref = measure(batch, 0, 0)
            w1, p1, out = measure(batch, G, f)
            line(f"B {B} serial", w0, p0, True)
            line(f"B {B} G {G} f {f / 1000:.2f}", w1, p1, bool(torch.equal(out, ref)))
        del batch
    sys.exit(0)

batch = make(int(arg("--batch", "4096")))
w, p, ref = measure(batch, 0, 0)
line("serial", w, p, True)
for G in (32, 48, 64, 96):
    for f in range(100, 901, 100):
        w, p, out = measure(batch, G, f)
        line(f"G {G} f {f / 1000:.2f}", w, p, bool(torch.equal(out, ref)))
    w, p, out = measure(batch, 0, 0)
    line("serial", w, p, bool(torch.equal(out, ref)))
