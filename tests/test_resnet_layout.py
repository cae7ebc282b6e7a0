"""The IMPALA ResNet unit's layout header on the CPU (impala_amd/csrc/resnet_layout.h): the C side's
flat-buffer offsets equal the running offsets of ``param_specs``, and the handle's two-pass carve is
sound (tests/resnet_layout_check.cpp); compiled with ROCm's clang++ and run; no GPU involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from impala_amd import resnet

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++")
    exe = tmp_path_factory.mktemp("resnet_layout") / "resnet_layout_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", str(exe),
                    os.path.join(HERE, "resnet_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("A", [1, 6, 15])
def test_flat_offsets_match_param_specs(check_output, A):
    line, = [l.split() for l in check_output.splitlines() if l.startswith(f"offsets {A} ")]
    got, total = [int(x) for x in line[2:-2]], int(line[-1])
    specs = resnet.param_specs(A)
    assert len(specs) == 38 and len(got) == 38
    off = 0
    for (key, shape), g in zip(specs, got):  # the C side prints in state_dict order
        assert g == off, key
        off += int(np.prod(shape))
    assert total == off == resnet.param_count(A)


def test_two_pass_carve(check_output):
    assert "carve ok" in check_output
