"""The cosine top-k has ONE workspace description for its two forms (`drin_amd/csrc/topk_layout.h`): a
stand-alone host program builds it in the single-table form (`drin_table_topk`) and the summed form (`drin_table_topk_sum`, 1 to 4
terms of mixed widths and storages) for 1 .. 65 535 mentions, tables of 300 .. 1 M rows, widths 16 / 32 / 768 / 776 (776: the
widen route), fp32 and bf16-stored rows, both precisions, k around the kp steps and default and explicit chunks, and checks
alignment, disjointness, the total, that each region holds what its launches index, and that the single form is the summed form at
S = 1 less exactly the rounded `scale` and `cos` regions."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topk_layout_regions_hold_in_both_forms(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "topk_layout"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{REPO}/drin_amd/csrc", f"{REPO}/tests/host/topk_layout_main.cpp", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "topk layout: 49152 cases hold" in r.stdout
