"""The argument checks of `drin_wgrad_probe` are plain host code (`drin_amd/csrc/wgrad_probe_check.h`): a stand-alone program
(`tests/host/wgrad_probe_check_main.cpp`) runs every refusal and every accepted form of each op under ASan and UBSan - a product
count past the struct's array among them - with message buffers shorter than the messages."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_probe_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "wgrad_probe_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{REPO}/drin_amd/csrc", f"{REPO}/tests/host/wgrad_probe_check_main.cpp", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "41 cases hold" in r.stdout
