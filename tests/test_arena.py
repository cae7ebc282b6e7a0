"""The workspace arena on the CPU (impala_amd/csrc/arena.h): the two-pass carve's sizing pass and
real pass agree, pieces are 256-byte aligned and disjoint; compiled with ROCm's clang++ and run;
no GPU involved."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_arena_two_pass_carve(tmp_path):
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++")
    exe = tmp_path / "arena_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", str(exe),
                    os.path.join(HERE, "arena_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "arena ok" in r.stdout, r.stderr
