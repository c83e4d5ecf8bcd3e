"""-m gpu: a plain `bench.py` run times its steps and nothing else, `--full` adds the instrumented pass, and `--dump-outputs`
writes what the timed path returned in its last step - the same in every run with the same arguments, and the path's own
result on the seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = {"roofline", "parity", "cpu_baseline", "legs", "kernel_ms_per_step", "scaling_model", "allreduce_ms", "step_floor_ms"}


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True, env=env,
                       timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_dumps_the_scores_of_its_last_timed_step(tmp_path):
    args = ("--workload", "wikidiverse", "--batch", "64", "--steps", "4", "--warmup", "1")
    a = _bench(*args, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*args, "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["dtype"] == "bf16x3" and line["higher_is_better"] is True
        assert line["unit"] == "pairs/s" and not MOVED & set(line)
    sa, sb = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert sa.dtype == np.float32 and sa.shape == (64, 11) and np.isfinite(sa).all()
    np.testing.assert_allclose(sa, sb, rtol=0, atol=1e-6)
    from drin_amd import synth
    from drin_amd.config import DrinConfig
    from drin_amd.model import Model
    cfg = DrinConfig()
    model = Model(cfg, precision="bf16x3").to("cuda").eval()
    model.load_state_dict(synth.make_state_dict(cfg, 7))
    with torch.no_grad():
        want = model(synth.make_device_batch(cfg, 64, 100, torch.device("cuda"))[:14]).cpu().numpy()
    np.testing.assert_allclose(sa, want, rtol=0, atol=1e-6)
    full = _bench(*args, "--full", "--no-cpu-baseline", "--legs-file", str(tmp_path / "full.json"))
    assert full["steps"] == 4 and {"roofline", "kernel_ms_per_step"} <= set(full) and (tmp_path / "full.json").exists()


def test_plain_training_run_dumps_the_loss_and_parameters_after_its_last_step(tmp_path):
    line = _bench("--mode", "train", "--batch", "16", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and not MOVED & set(line)
    loss, params = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "parameters.npy")
    assert loss.dtype == params.dtype == np.float32 and loss.shape == (1,) and params.size > 10 ** 6
    assert abs(float(loss[0]) - line["final_loss"]) <= 1e-6 and np.isfinite(params).all()
