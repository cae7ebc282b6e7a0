"""Build the HIP extension in-tree: ``python -m impala_amd.build``.

Compiles ``impala_amd/csrc/{impala,sac,dqn_replay,ppo_replay,dqn_inplace,iqn,iqn_replay}.hip`` for gfx950 into ``impala_amd/libimpala_hip.so`` with
hipcc (cross-compiles without a GPU).  The .so is git-ignored and travels with the tree.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libimpala_hip.so")
ARCH = os.environ.get("IMPALA_OFFLOAD_ARCH", "gfx950")


def sources():
    return sorted(os.path.join(SRC_DIR, f) for f in os.listdir(SRC_DIR)
                  if f.endswith((".hip", ".h")))


def hip_units():
    """The translation units linked into the one library (impala.hip: IMPALA / PPO learner and,
    through csrc/dqn.h on the same launchers, the Ape-X DQN learner; sac.hip: SAC learner;
    dqn_replay.hip: the kernels of the DQN learner's device-side replay, kept out of impala.hip's
    code object; ppo_replay.hip: the PPO actor's lambda-return ingest kernel, kept out likewise;
    dqn_inplace.hip: the DQN step's three batch-reading kernels instantiated for a replay ring read in
    place, kept out likewise; iqn.hip: the kernels of the distributional (IQN) actor path and
    training step, kept out likewise; iqn_replay.hip: the two ingest kernels of the IQN learner's
    device-side replay, kept out likewise)."""
    return [os.path.join(SRC_DIR, f)
            for f in ("impala.hip", "sac.hip", "dqn_replay.hip", "ppo_replay.hip", "dqn_inplace.hip",
                      "iqn.hip", "iqn_replay.hip")]


# Per-unit flags.  impala.hip's kernels start on 1 KB boundaries of the code object (the
# compiler's default is 256 B): the bf16 step, eight launches in 0.093 ms, moves by up to 0.9 %
# with where its kernels sit, and with the default alignment that changes whenever a kernel
# before them is added or removed.  The kernels' own machine code is unchanged
# (profiles/onepath: ab.txt, isa_cmp.txt).
_ALIGN_1K = ["-Xarch_device", "-falign-functions=1024"]
# (ppo_replay.hip and dqn_inplace.hip hold learner-step kernels too: the PPO head and the DQN
# step's kernels that read a ring in place)
UNIT_FLAGS = {"impala.hip": _ALIGN_1K, "ppo_replay.hip": _ALIGN_1K, "dqn_inplace.hip": _ALIGN_1K}


def needs_build(out: str = OUT) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    inc = os.path.join(os.path.dirname(HERE), "include")
    deps = sources() + [os.path.join(inc, f) for f in os.listdir(inc)]
    return any(os.path.getmtime(s) > t for s in deps if os.path.exists(s))


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile the library in-tree."""
    out = OUT
    if not force and not needs_build(out):
        return out
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = out + ".tmp"
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall",
             "-Wno-unused-function"]
    # the units compile in parallel (sac.hip dominates), then one link
    objs, procs = [], []
    for src in hip_units():
        obj = os.path.join(HERE, os.path.basename(src) + ".o")
        objs.append(obj)
        cmd = [hipcc] + flags + UNIT_FLAGS.get(os.path.basename(src), []) + ["-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
    failed = [cmd for cmd, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    if os.path.exists(tmp):
        os.remove(tmp)
    subprocess.run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs,
                   check=True)
    os.replace(tmp, out)
    for obj in objs:
        os.remove(obj)
    return out


if __name__ == "__main__":
    print("built", build(force="--force" in sys.argv))
