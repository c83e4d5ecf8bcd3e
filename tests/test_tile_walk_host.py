"""The persistent grid of the four-phase GEMMs (`k_gemm_bf16x3_p4<true>`, `k_gemm_x3_planes_p4<false, false, true>`) walks a range
of 256 x 256 tiles by host-checkable index arithmetic (`drin_amd/csrc/tile_walk.h`): a stand-alone host program walks it for
tiles in {1, 7, 8, 9, 153, 4848}, three column tiles, grids of 1, 8 and 64 workgroups, from row tile 0 and from row tile 5."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_persistent_walk_visits_every_tile_of_its_range_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tile_walk"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{REPO}/drin_amd/csrc", f"{REPO}/tests/host/tile_walk_main.cpp", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "36 cases hold" in r.stdout
