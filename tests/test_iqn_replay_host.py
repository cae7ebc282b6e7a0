"""iqn_replay on the CPU: the C boundary (declared, bound, exported, ABI 3, every argument refused
before any HIP call: scalars, then named null pointers, then the handle), the Python surface's
refusals that need no device, and the new host bookkeeping (impala_amd/csrc/iqn_replay_host.h)
under sanitizers in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from impala_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(REPO, "include", "iqn_hip.h")
NEW = ("iqn_replay_create", "iqn_replay_destroy", "iqn_replay_bind", "iqn_replay_state",
       "iqn_replay_extend", "iqn_replay_extend_rollout", "iqn_replay_sample", "iqn_replay_update",
       "iqn_replay_weights", "iqn_train_step_replay")
INVALID = 1001
FAKE = 0x1000  # a non-null pointer no entry may look through before it has refused the call


def _err():
    return _lib.lib().iqn_last_error().decode()


# ---------------------------------------------------------------- boundary
def test_new_names_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(iqn_\w+)\s*\(", src))
    lib = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\b(iqn_\w+)\b", out))
    for name in NEW:
        assert name in declared and name in _lib.IQN_EXPORTS and name in exported, name
        assert getattr(lib, name).argtypes is not None, name
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.iqn_abi_version() == 3 == _lib.IQN_ABI_VERSION
    assert "#define IQN_ABI_VERSION 3" in src
    assert "typedef struct iqn_replay iqn_replay;" in src
    # dqn_hip.h is as it was
    assert lib.dqn_abi_version() == 2 == _lib.DQN_ABI_VERSION


def test_null_handles_are_refused_before_any_hip_call():
    lib = _lib.lib()
    n64 = C.c_int64()
    assert lib.iqn_replay_destroy(None) == 0
    assert lib.iqn_replay_bind(None, FAKE, FAKE, FAKE, FAKE, None) == INVALID and "handle" in _err()
    assert lib.iqn_replay_state(None, C.byref(n64), C.byref(n64)) == INVALID and "handle" in _err()
    assert lib.iqn_replay_extend(None, FAKE, FAKE, FAKE, None, 4, None, None) == INVALID
    assert "handle" in _err()
    assert lib.iqn_replay_extend_rollout(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 5, 3, 0.99, None,
                                         None) == INVALID and "handle" in _err()
    assert lib.iqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, None, None, None, None) == INVALID
    assert "handle" in _err()
    assert lib.iqn_replay_update(None, FAKE, FAKE, 4, None) == INVALID and "handle" in _err()
    assert lib.iqn_replay_weights(None, FAKE, None, None) == INVALID and "handle" in _err()
    assert lib.iqn_train_step_replay(None, None, 1, 2, None, 3, 4, None, None, None, None) == INVALID
    assert "handle" in _err()


def _entries(lib):
    """entry -> (call taking its pointer arguments by name, the names in order).  The handle is
    null and every scalar valid, so only the pointer checks can refuse the call before it."""
    return {
        "iqn_replay_bind": (lambda obs, actions, targets, priorities:
                            lib.iqn_replay_bind(None, obs, actions, targets, priorities, None),
                            ("obs", "actions", "targets", "priorities")),
        "iqn_replay_state": (lambda size, cursor: lib.iqn_replay_state(
            None, C.cast(size, C.POINTER(C.c_int64)), C.cast(cursor, C.POINTER(C.c_int64))),
            ("size", "cursor")),
        "iqn_replay_extend": (lambda obs, actions, targets:
                              lib.iqn_replay_extend(None, obs, actions, targets, None, 4, None, None),
                              ("obs", "actions", "targets")),
        "iqn_replay_extend_rollout": (lambda obs, actions, rewards, done, q_pi, q_star:
                                      lib.iqn_replay_extend_rollout(None, obs, actions, rewards, done, q_pi,
                                                                    q_star, 5, 3, 0.99, None, None),
                                      ("obs", "actions", "rewards", "done", "q_pi", "q_star")),
        "iqn_replay_sample": (lambda keys, probabilities:
                              lib.iqn_replay_sample(None, 1, 2, 4, keys, probabilities, None, None, None, None),
                              ("keys", "probabilities")),
        "iqn_replay_update": (lambda keys, priorities: lib.iqn_replay_update(None, keys, priorities, 4, None),
                              ("keys", "priorities")),
        "iqn_replay_weights": (lambda weights_out: lib.iqn_replay_weights(None, weights_out, None, None),
                               ("weights_out",)),
    }


def test_each_null_pointer_is_refused_and_named_before_the_handle_is_looked_at():
    lib = _lib.lib()
    for entry, (call, names) in _entries(lib).items():
        for bad in names:
            args = [None if name == bad else FAKE for name in names]
            assert call(*args) == INVALID, (entry, bad)
            msg = _err()
            assert entry in msg and msg.endswith("null pointer: " + bad), (entry, bad, msg)
        assert call(*([FAKE] * len(names))) == INVALID and "handle" in _err(), entry
    assert lib.iqn_replay_create(16, 8, 0.6, 0, None) == INVALID
    assert _err().endswith("null pointer: out")


def test_out_array_rules_are_refused_before_the_handle_is_looked_at():
    lib = _lib.lib()
    assert lib.iqn_replay_bind(None, FAKE + 8, FAKE, FAKE, FAKE, None) == INVALID
    assert "obs must be 16-byte aligned" in _err()
    for outs in ((FAKE, None, None), (None, FAKE, None), (None, None, FAKE), (FAKE, FAKE, None),
                 (FAKE, None, FAKE), (None, FAKE, FAKE)):
        assert lib.iqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, *outs, None) == INVALID
        assert "all or none" in _err(), outs
    assert lib.iqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, FAKE + 4, FAKE, FAKE, None) == INVALID
    assert "obs_out must be 16-byte aligned" in _err()
    assert lib.iqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert "handle" in _err()


@pytest.mark.parametrize("capacity,n_tau,alpha,word", [
    (16, 0, 0.6, "n_tau"), (16, 33, 0.6, "n_tau"), (16, -1, 0.6, "n_tau"),
    (0, 8, 0.6, "capacity"), (-5, 8, 0.6, "capacity"), (2097153, 8, 0.6, "capacity"),
    (16, 8, -0.1, "priority_exponent"), (16, 8, float("nan"), "priority_exponent"),
    (16, 8, float("inf"), "priority_exponent")])
def test_create_refuses_bad_arguments(capacity, n_tau, alpha, word):
    lib = _lib.lib()
    h = _lib._P()
    assert lib.iqn_replay_create(capacity, n_tau, alpha, 0, C.byref(h)) == INVALID and not h.value
    assert word in _err() and "iqn_replay_create" in _err()
    # the scalars come first: the same refusal with a null out pointer
    assert lib.iqn_replay_create(capacity, n_tau, alpha, 0, None) == INVALID and word in _err()


def test_scalar_arguments_are_refused_and_named():
    """The checks that need no ring run before the pointers and the handle are looked at;
    n > capacity and L - 1 > capacity need a ring: the GPU test covers them."""
    lib = _lib.lib()
    for n in (0, -3):
        assert lib.iqn_replay_extend(None, None, None, None, None, n, None, None) == INVALID
        assert "n must be >= 1" in _err()
        assert lib.iqn_replay_sample(None, 0, 0, n, None, None, None, None, None, None) == INVALID
        assert "n must be >= 1" in _err()
        assert lib.iqn_replay_update(None, None, None, n, None) == INVALID
        assert "n must be >= 1" in _err()
    assert lib.iqn_replay_update(None, FAKE, FAKE, 4097, None) == INVALID and "DQN_MAX_BATCH" in _err()

    def rollout(L=5, n_step=3, gamma=0.99, p=None):
        return lib.iqn_replay_extend_rollout(None, p, p, p, p, p, p, L, n_step, gamma, None, None)
    for L in (1, 0, -2):
        assert rollout(L=L) == INVALID and "L must be >= 2" in _err()
    for k in (0, 17, -1):
        assert rollout(n_step=k) == INVALID and "n_step" in _err()
    for g in (-0.01, 1.01, float("nan")):
        assert rollout(gamma=g) == INVALID and "gamma" in _err()
    assert rollout() == INVALID and "null pointer: obs" in _err()  # valid scalars: the pointers are next
    assert rollout(p=FAKE) == INVALID and "handle" in _err()       # then the handle


def test_host_bookkeeping_under_sanitizers(tmp_path):
    """impala_amd/csrc/iqn_replay_host.h in a stand-alone program built with
    -fsanitize=address,undefined on the CPU (no GPU, nothing loaded into python)."""
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or \
        shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "iqn_replay_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "iqn_replay_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "iqn_replay ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- Python surface
def test_python_refusals_need_no_device():
    import impala_amd
    from impala_amd import iqn
    from impala_amd.dqn import DqnEngine, NativePrioritizedReplay
    assert impala_amd.NativeQuantileReplay is iqn.NativeQuantileReplay
    assert "NativeQuantileReplay" in impala_amd.__all__
    assert issubclass(iqn.NativeQuantileReplay, NativePrioritizedReplay)
    assert iqn.REPLAY_STEP_CALLS == 0
    with pytest.raises(RuntimeError, match="cuda"):
        iqn.NativeQuantileReplay(8, 8, device="cpu")
    for W in (0, 33):
        with pytest.raises(ValueError, match="target_width"):
            iqn.NativeQuantileReplay(8, W, device="cpu")
    with pytest.raises(ValueError, match="observations"):
        iqn.NativeQuantileReplay(8, 8, device="cuda", obs_shape=(3, 32, 32))
    with pytest.raises(NotImplementedError, match="target_width"):
        NativePrioritizedReplay(8, device="cuda", target_width=8)
    # the scalar step refuses a handle that is not a dqn_replay
    stub = iqn.NativeQuantileReplay.__new__(iqn.NativeQuantileReplay)
    with pytest.raises(TypeError):
        DqnEngine._own_replay(stub)
    DqnEngine._own_replay(NativePrioritizedReplay.__new__(NativePrioritizedReplay))


def test_builder_make_replay_native_needs_a_cuda_device():
    from impala_amd.config import load_config
    from impala_amd.dqn import PrioritizedReplay
    from impala_amd.iqn import ApexDistributionalBuilder
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = "cpu"
    cfg.agent.replay_buffer_size = 32
    b = ApexDistributionalBuilder(cfg)
    with pytest.raises(NotImplementedError, match="cuda"):
        b.make_replay(native=True)
    with pytest.raises(NotImplementedError, match="in-place"):
        b.make_replay(native=True, in_place=True)
    with pytest.raises(NotImplementedError, match="in-place"):
        b.make_replay(in_place=True)
    rb = b.make_replay()
    assert type(rb) is PrioritizedReplay and rb.target.shape == (32, 8)


def test_extend_rollout_shape_checks():
    from impala_amd.iqn import NativeQuantileReplay
    rb = NativeQuantileReplay.__new__(NativeQuantileReplay)  # no handle, no device: shapes only
    rb.target_width = W = 8
    L = 5
    good = dict(s=torch.zeros(L, 3, 64, 64, dtype=torch.uint8), a=torch.zeros(L, dtype=torch.int64),
                r=torch.zeros(L), done=torch.zeros(L, dtype=torch.bool), q_pi=torch.zeros(L),
                q_star=torch.zeros(L, W))
    assert NativeQuantileReplay._rollout_shapes(W, **good) == L
    bad = [dict(q_star=torch.zeros(L, W - 1)), dict(q_star=torch.zeros(L)), dict(q_star=torch.zeros(L - 1, W)),
           dict(a=torch.zeros(L - 1, dtype=torch.int64)), dict(r=torch.zeros(L + 1)),
           dict(done=torch.zeros(2, dtype=torch.bool)), dict(q_pi=torch.zeros(L, 2)),
           dict(s=torch.zeros(L, 3, 32, 32, dtype=torch.uint8)),
           {k: v[:1] for k, v in good.items()}]
    for change in bad:
        with pytest.raises(ValueError, match="extend_rollout"):
            rb.extend_rollout(**{**good, **change})
