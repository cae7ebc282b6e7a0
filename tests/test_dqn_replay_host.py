"""dqn_replay on the CPU: the C boundary (declared, bound, exported, ABI 2, arguments refused before
any HIP call), the numpy restatement of the sampling contract and of the n-step recurrence
(tests/dqn_replay_oracle.py) against a transcription of rlax's loop, and the ring's host
bookkeeping (impala_amd/csrc/dqn_replay_host.h) under sanitizers in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dqn_replay_oracle as rorc
from impala_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(REPO, "include", "dqn_hip.h")
NEW = ("dqn_replay_block", "dqn_replay_create", "dqn_replay_destroy", "dqn_replay_bind",
       "dqn_replay_state", "dqn_replay_extend", "dqn_replay_extend_rollout", "dqn_replay_sample",
       "dqn_replay_update", "dqn_train_step_replay", "dqn_replay_weights")
INVALID = 1001
FAKE = 0x1000  # a non-null pointer no entry may look through before it has refused the call


def _err():
    return _lib.lib().dqn_last_error().decode()


# ---------------------------------------------------------------- boundary
def test_new_names_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dqn_\w+)\s*\(", src))
    lib = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\b(dqn_\w+)\b", out))
    for name in NEW:
        assert name in declared and name in _lib.DQN_EXPORTS and name in exported, name
        assert getattr(lib, name).argtypes is not None or name == "dqn_replay_block", name
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dqn_abi_version() == 2 == _lib.DQN_ABI_VERSION
    assert "#define DQN_ABI_VERSION 2" in src
    assert lib.dqn_replay_block() == _lib.DQN_REPLAY_BLOCK
    assert f"#define DQN_REPLAY_BLOCK {_lib.DQN_REPLAY_BLOCK}" in src
    b = _lib.DQN_REPLAY_BLOCK
    assert b >= 64 and b & (b - 1) == 0  # a fixed power of two


def test_null_handles_and_pointers_are_refused_before_any_hip_call():
    lib = _lib.lib()
    h = _lib._P()
    assert lib.dqn_replay_create(16, 0.6, 0, None) == INVALID and "out" in _err()
    assert lib.dqn_replay_destroy(None) == 0
    assert lib.dqn_replay_bind(None, FAKE, FAKE, FAKE, FAKE, None) == INVALID and "handle" in _err()
    n64 = C.c_int64()
    assert lib.dqn_replay_state(None, C.byref(n64), C.byref(n64)) == INVALID and "handle" in _err()
    assert lib.dqn_replay_extend(None, FAKE, FAKE, FAKE, None, 4, None, None) == INVALID
    assert "handle" in _err()
    assert lib.dqn_replay_extend_rollout(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 5, 3, 0.99, None,
                                         None) == INVALID and "handle" in _err()
    assert lib.dqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, None, None, None, None) == INVALID
    assert "handle" in _err()
    assert lib.dqn_replay_update(None, FAKE, FAKE, 4, None) == INVALID and "handle" in _err()
    assert lib.dqn_train_step_replay(None, None, 1, 2, None, None, None) == INVALID
    assert "handle" in _err()
    assert lib.dqn_replay_weights(None, FAKE, None, None) == INVALID and "handle" in _err()
    assert not h.value


def _entries(lib):
    """entry -> (call taking its pointer arguments by name, the names in order).  The handle is
    null and every scalar valid, so only the pointer checks can refuse the call before it."""
    return {
        "dqn_replay_bind": (lambda obs, actions, targets, priorities:
                            lib.dqn_replay_bind(None, obs, actions, targets, priorities, None),
                            ("obs", "actions", "targets", "priorities")),
        "dqn_replay_state": (lambda size, cursor: lib.dqn_replay_state(
            None, C.cast(size, C.POINTER(C.c_int64)), C.cast(cursor, C.POINTER(C.c_int64))),
            ("size", "cursor")),
        "dqn_replay_extend": (lambda obs, actions, targets:
                              lib.dqn_replay_extend(None, obs, actions, targets, None, 4, None, None),
                              ("obs", "actions", "targets")),
        "dqn_replay_extend_rollout": (lambda obs, actions, rewards, done, q_pi, q_star:
                                      lib.dqn_replay_extend_rollout(None, obs, actions, rewards, done, q_pi,
                                                                    q_star, 5, 3, 0.99, None, None),
                                      ("obs", "actions", "rewards", "done", "q_pi", "q_star")),
        "dqn_replay_sample": (lambda keys, probabilities:
                              lib.dqn_replay_sample(None, 1, 2, 4, keys, probabilities, None, None, None, None),
                              ("keys", "probabilities")),
        "dqn_replay_update": (lambda keys, priorities: lib.dqn_replay_update(None, keys, priorities, 4, None),
                              ("keys", "priorities")),
        "dqn_replay_weights": (lambda weights_out: lib.dqn_replay_weights(None, weights_out, None, None),
                               ("weights_out",)),
    }


def test_each_null_pointer_is_refused_and_named_before_the_handle_is_looked_at():
    """One null pointer at a time, every other pointer non-null, the handle null: the entry
    refuses with IMPALA_E_INVALID and dqn_last_error names that argument (not the handle), so
    the check sits ahead of anything that touches a device."""
    lib = _lib.lib()
    for entry, (call, names) in _entries(lib).items():
        for bad in names:
            args = [None if name == bad else FAKE for name in names]
            assert call(*args) == INVALID, (entry, bad)
            msg = _err()
            assert entry in msg and msg.endswith("null pointer: " + bad), (entry, bad, msg)
        assert call(*([FAKE] * len(names))) == INVALID and "handle" in _err(), entry


def test_out_array_rules_are_refused_before_the_handle_is_looked_at():
    lib = _lib.lib()
    # bind: obs 16-byte aligned
    assert lib.dqn_replay_bind(None, FAKE + 8, FAKE, FAKE, FAKE, None) == INVALID
    assert "obs must be 16-byte aligned" in _err()
    # sample: the three out arrays all or none, obs_out 16-byte aligned
    for outs in ((FAKE, None, None), (None, FAKE, None), (None, None, FAKE), (FAKE, FAKE, None),
                 (FAKE, None, FAKE), (None, FAKE, FAKE)):
        assert lib.dqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, *outs, None) == INVALID
        assert "all or none" in _err(), outs
    assert lib.dqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, FAKE + 4, FAKE, FAKE, None) == INVALID
    assert "obs_out must be 16-byte aligned" in _err()
    assert lib.dqn_replay_sample(None, 1, 2, 4, FAKE, FAKE, FAKE, FAKE, FAKE, None) == INVALID
    assert "handle" in _err()


@pytest.mark.parametrize("capacity,alpha,word", [
    (0, 0.6, "capacity"), (-5, 0.6, "capacity"), (1 << 40, 0.6, "capacity"),
    (16, -0.1, "priority_exponent"), (16, float("nan"), "priority_exponent"),
    (16, float("inf"), "priority_exponent")])
def test_create_refuses_bad_arguments(capacity, alpha, word):
    lib = _lib.lib()
    h = _lib._P()
    assert lib.dqn_replay_create(capacity, alpha, 0, C.byref(h)) == INVALID and not h.value
    assert word in _err()


def test_scalar_arguments_are_refused_and_named():
    """The checks that need no ring run before the handle is looked at, so they are visible here;
    n > capacity needs a ring: tests/dqn_replay_check.cpp and the GPU test cover it."""
    lib = _lib.lib()
    for n in (0, -3):
        assert lib.dqn_replay_extend(None, FAKE, FAKE, FAKE, None, n, None, None) == INVALID
        assert "n must be >= 1" in _err()
        assert lib.dqn_replay_sample(None, 0, 0, n, FAKE, FAKE, None, None, None, None) == INVALID
        assert "n must be >= 1" in _err()
        assert lib.dqn_replay_update(None, FAKE, FAKE, n, None) == INVALID
        assert "n must be >= 1" in _err()
    assert lib.dqn_replay_update(None, FAKE, FAKE, 4097, None) == INVALID and "DQN_MAX_BATCH" in _err()

    def rollout(L=5, n_step=3, gamma=0.99):
        return lib.dqn_replay_extend_rollout(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, L, n_step,
                                             gamma, None, None)
    for L in (1, 0, -2):
        assert rollout(L=L) == INVALID and "L must be >= 2" in _err()
    for k in (0, 17, -1):
        assert rollout(n_step=k) == INVALID and "n_step" in _err()
    for g in (-0.01, 1.01, float("nan")):
        assert rollout(gamma=g) == INVALID and "gamma" in _err()
    assert rollout() == INVALID and "handle" in _err()  # valid scalars: the null handle is next


def test_host_bookkeeping_under_sanitizers(tmp_path):
    """impala_amd/csrc/dqn_replay_host.h in a stand-alone program built with
    -fsanitize=address,undefined on the CPU (no GPU, nothing loaded into python)."""
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or \
        shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "dqn_replay_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(HERE, "dqn_replay_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dqn_replay ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the restatement
def test_mix_is_the_kernels_constant_stream():
    # splitmix64's published first outputs from state 0 are mix(0), mix(golden), ...; the first
    # is 0xE220A8397B1DCDAF
    assert rorc.mix(0) == 0xE220A8397B1DCDAF
    u = rorc.uniforms(7, 3, 1000)
    assert u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55
    assert not np.array_equal(u, rorc.uniforms(7, 4, 1000))
    assert np.array_equal(u[:10], rorc.uniforms(7, 3, 10))


def test_oracle_sample_follows_the_contract():
    w = np.array([0.0, 2.0, 0.0, 1.0, 1.0, 0.0])
    keys, probs, margin = rorc.sample(w, 6, seed=1, counter=0, n=4000)
    assert set(np.unique(keys)) == {1, 3, 4} and margin > 0
    np.testing.assert_allclose(np.bincount(keys, minlength=6) / 4000, w / 4, atol=0.03)
    np.testing.assert_allclose(probs, (w / 4)[keys].astype(np.float32))
    # only the first `size` rows count
    k2, p2, _ = rorc.sample(w, 2, seed=1, counter=0, n=50)
    assert set(k2) == {1} and np.all(p2 == 1.0)
    # zero total: uniform
    k0, p0, m0 = rorc.sample(np.zeros(5), 5, seed=1, counter=0, n=50)
    assert np.array_equal(k0, np.floor(rorc.uniforms(1, 0, 50) * 5).astype(np.int64))
    assert np.all(p0 == np.float32(0.2)) and m0 == np.inf
    np.testing.assert_allclose(rorc.weights([0.0, 4.0, 1e-3], 0.5), [0.0, 2.0, np.float64(np.float32(1e-3)) ** 0.5],
                               rtol=1e-15)


@pytest.mark.parametrize("L", [2, 3, 7, 100])
@pytest.mark.parametrize("n_step", [1, 3, 16])
def test_nstep_restatement_equals_rlax_loop(L, n_step):
    rng = np.random.default_rng(1000 * L + n_step)
    for trial in range(5):
        r = rng.standard_normal(L)
        q = rng.standard_normal(L) * 3
        done = rng.random(L) < (0.0, 0.15, 0.5, 0.15, 1.0)[trial]
        if trial == 3 and L >= 3:
            done[:] = False
            done[[0, L - 2, L - 1]] = True  # the first, the last used and the unused last step
        a = rorc.nstep_targets(r, done, q, n_step, 0.99)
        b = rorc.rlax_targets(r, done, q, n_step, 0.99)
        assert a.shape == b.shape == (L - 1,)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


def test_nstep_known_values():
    # L = 4, n = 2, gamma = 0.5, no dones: target_0 = r0 + .5 (r1 + .5 q2), target_2 = r2 + .5 q3
    r, q = np.array([1.0, 2.0, 3.0, 99.0]), np.array([7.0, 10.0, 20.0, 40.0])
    t = rorc.nstep_targets(r, np.zeros(4), q, 2, 0.5)
    np.testing.assert_allclose(t, [1 + .5 * (2 + .5 * 20), 2 + .5 * (3 + .5 * 40), 3 + .5 * 40])
    # a done at step 1 cuts every bootstrap through it
    t = rorc.nstep_targets(r, np.array([0, 1, 0, 0]), q, 2, 0.5)
    np.testing.assert_allclose(t, [1 + .5 * 2, 2.0, 3 + .5 * 40])
