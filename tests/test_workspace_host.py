"""Every workspace region is declared once, by a take() from one arena (`drin_amd/csrc/arena.h`): a stand-alone host program builds
the layer-by-layer layout (`Layout`) and the backward pass's temporaries (`BackwardScratch`) for 0..8 layers, batches around the
scratch gates (1 .. 4 096 mentions, 1 / 11 / 101 candidates), both width pairs, scalar and vector edges, static and dynamic, the
three precisions, training and inference, and checks alignment, disjointness of what is live together, the total, and that each
backward region holds what the pass indexes."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_regions_are_aligned_disjoint_and_hold_what_the_pass_indexes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "workspace"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{REPO}/drin_amd/csrc", f"{REPO}/tests/host/workspace_main.cpp", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "workspace: 11664 cases hold" in r.stdout
