"""The fragment-major layouts of the fp32 dgrad weight copies w2t / w3t (impala_amd/csrc/net.h
w2t_index / w3t_index) on the CPU: tests/wfrag_check.cpp, compiled with ROCm's clang++ and run;
no GPU involved."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_wfrag_index_maps(tmp_path):
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++")
    exe = tmp_path / "wfrag_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", str(exe),
                    os.path.join(HERE, "wfrag_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wfrag ok" in r.stdout, r.stdout + r.stderr
