"""dqn_replay on the CPU: the C boundary (declared, bound, exported, ABI 2, arguments refused before
any HIP call), the numpy restatement of the sampling contract and of the n-step recurrence
(tests/dqn_replay_oracle.py) against a transcription of rlax's loop, the ring's host
bookkeeping (impala_amd/csrc/dqn_replay_host.h) under sanitizers in a stand-alone program, and
the inputs of tests/test_gpu_dqn_replay_scale.py (tests/dqn_replay_scale_cases.py): the
restatement of the kernels' summation order against np.cumsum and an 80-bit prefix, the input
condition of every draw those tests make, and three deliberate defects that those draws notice."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dqn_replay_oracle as rorc
import dqn_replay_scale_cases as sc
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
    # the Python mirror of scan_chunk against the C one, at every legal number of blocks
    r = subprocess.run([str(exe), "scan_chunk"], capture_output=True, text=True, timeout=120)
    table = [int(x) for x in r.stdout.split()]
    assert r.returncode == 0 and len(table) == 4096, r.stderr
    assert table == [rorc.scan_chunk(nb) for nb in range(1, 4097)]


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


# ---------------------------------------------------------------- the scale tests' inputs
SCALE_RINGS = [(size, pat) for size in sc.SCAN_SHAPES for pat in sc.PATTERNS] + [(sc.BIG, "exact")]
_ring_id = lambda r: f"{r[0]}_{r[1]}"


def _ring_weights(size, pattern):
    p, alpha = sc.priorities(size, pattern)
    return rorc.weights(p, alpha)


def test_scale_geometry_is_the_issue_table():
    assert rorc.BLOCK == _lib.DQN_REPLAY_BLOCK
    for size, geo in sc.SCAN_SHAPES.items():
        assert sc.geometry(size) == geo, size
    assert sc.geometry(sc.BIG) == (704, 27, 27) and sc.geometry(1_000_000) == (1954, 45, 44)
    assert sc.BIG * sc.ROW > 2 ** 32 and (sc.BIG - 1) // 512 + 1 <= 4096
    for size in list(sc.SCAN_SHAPES) + [sc.BIG]:
        nb, chunk, T = sc.geometry(size)
        runs = sc.zero_runs(size)
        assert runs[0][0] == 0 and runs[-1][1] == size
        # one scan thread's entire run of blocks is zero; the last positive block is not the last
        assert any(lo % (chunk * 512) == 0 and hi - lo == chunk * 512 for lo, hi in runs), size
        for pat in sc.PATTERNS:
            w = _ring_weights(size, pat)
            bs = rorc.block_sums(w, size)
            assert bs[-1] == 0 and np.flatnonzero(bs > 0)[-1] == nb - 2
            per_thread = [bs[t * chunk:(t + 1) * chunk].sum() for t in range(T)]
            assert min(per_thread) == 0 and w[0] == 0 and w[-1] == 0


@pytest.mark.parametrize("size", list(sc.SCAN_SHAPES) + [sc.BIG, 1_000_000])
def test_kernel_order_cumsum_and_long_double_prefix_agree(size):
    """Pattern (i): the three prefixes differ by the measured discrepancy, which is below the
    worst-case bound of a float64 sum of `size` non-negative terms, size * 2^-53 of the total.
    Pattern (ii): the three are the same numbers."""
    assert np.finfo(np.longdouble).nmant >= 63  # the reference prefix carries 11 more bits
    if size == 1_000_000:
        p = (10.0 ** np.random.default_rng(size).uniform(-3, 3, size)).astype(np.float32)
        p[-1] = 0.0
        w = rorc.weights(p, sc.ALPHA)
    else:
        w = _ring_weights(size, "exact")
    d = rorc.prefix_discrepancy(w, size)
    print(f"rows {size}: prefix discrepancy {d:.3g} of the total")
    assert 0 < d < size * 2.0 ** -53
    assert d < 1e-13  # what the GPU tests' docstrings state for these sizes
    if size == 1_000_000:
        return
    w = _ring_weights(size, "uniform")
    K, Cs, P = rorc.kernel_prefix(w, size), np.cumsum(w), np.cumsum(w.astype(np.longdouble))
    assert np.array_equal(K, Cs) and np.array_equal(K.astype(np.longdouble), P)
    assert rorc.prefix_discrepancy(w, size) == 0.0
    assert np.array_equal(w * 8, np.round(w * 8)) and w.max() <= 8.0


def test_kernel_order_restatement_on_known_values():
    # one block: lanes 0 and 1 hold rows 0..7 and 8..15
    w = np.arange(1, 17, dtype=np.float64)
    assert rorc.block_sums(w, 16).tolist() == [136.0]
    assert np.array_equal(rorc.kernel_prefix(w, 16), np.cumsum(w))
    # 5 blocks: chunk 3, two scan threads; thread 1's offset is thread 0's total
    w = np.ones(5 * 512)
    P, total = rorc.block_prefix(rorc.block_sums(w, len(w)))
    assert P.tolist() == [512.0 * k for k in range(1, 6)] and total == 2560.0
    P, _ = rorc.block_prefix(rorc.block_sums(w, len(w)), ("drop_offset", 1))
    assert P.tolist() == [512.0, 1024.0, 1536.0, 512.0, 1024.0]
    _, total = rorc.block_prefix(rorc.block_sums(w, len(w)), ("stale_tail",))
    assert total == 2560.0 + 254 * 1024.0
    # the draw on it: the contract's keys
    k, _, _ = rorc.sample(w, len(w), 3, 0, 200)
    assert np.array_equal(rorc.sample_kernel_order(w, len(w), 3, 0, 200), k)


@pytest.mark.parametrize("ring", SCALE_RINGS, ids=_ring_id)
def test_scale_draws_satisfy_their_input_condition(ring):
    """Every (shape, pattern, n, seed) tests/test_gpu_dqn_replay_scale.py draws: the margin against
    the measured discrepancy (dqn_replay_scale_cases.condition), the contract's keys equal to the
    kernel-order restatement's, no zero-weight row drawn, and on the large ring keys on all three
    sides of the byte offsets 2^31 and 2^32."""
    size, pat = ring
    w = _ring_weights(size, pat)
    d = rorc.prefix_discrepancy(w, size)
    big = size == sc.BIG
    for n in (sc.BIG_NS if big else sc.NS):
        seed = sc.BIG_SEED if big else sc.SCAN_SEED
        keys, probs, margin = rorc.sample(w, size, seed, sc.counter(n), n)
        print(f"rows {size} {pat} n {n} seed {seed}: margin {margin:.3g} discrepancy {d:.3g}"
              + (f" keys per band {sc.bands(keys)}" if big else ""))
        assert sc.condition(pat, margin, d), f"pick another seed: margin {margin}, discrepancy {d}"
        assert np.array_equal(rorc.sample_kernel_order(w, size, seed, sc.counter(n), n), keys)
        assert np.all(w[keys] > 0)
        if big:
            assert min(sc.bands(keys)) >= 1, "pick another seed: a band without a key"


def test_update_outcomes_satisfy_the_input_condition():
    """The draw after the update at high keys, whichever of a duplicated key's values landed."""
    uniq = np.unique(sc.UPDATE_KEYS)
    outcomes = list(sc.update_outcomes())
    assert len(outcomes) == 4
    for p in outcomes:
        w = rorc.weights(p, sc.ALPHA)
        d = rorc.prefix_discrepancy(w, sc.BIG)
        keys, _, margin = rorc.sample(w, sc.BIG, sc.UPDATE_SEED, sc.UPDATE_COUNTER, sc.UPDATE_N)
        print(f"update outcome: margin {margin:.3g} discrepancy {d:.3g} draws per updated key "
              f"{[int((keys == k).sum()) for k in uniq]}")
        assert sc.condition("exact", margin, d)
        assert all((keys == k).any() for k in uniq)  # every updated key is drawn


def test_step_edge_rows_are_all_that_can_be_drawn():
    p = sc.step_priorities()
    assert np.array_equal(np.flatnonzero(p), sc.STEP_ROWS) and set(sc.STEP_MUST) <= set(sc.STEP_ROWS.tolist())
    w = rorc.weights(p, sc.ALPHA)
    keys, _, margin = rorc.sample(w, sc.BIG, sc.STEP_SEED, 0, 33)
    assert margin > 1e-9 and rorc.prefix_discrepancy(w, sc.BIG) < 1e-15
    assert set(keys.tolist()) <= set(sc.STEP_ROWS.tolist()) and len(np.unique(keys)) < 33
    assert min(sc.bands(keys)) >= 1


def test_deliberate_defects_change_the_chosen_draws():
    """The chosen inputs would notice: a scan thread's dropped offset (every thread whose offset
    and own total are positive, at every ring), an idle scan thread that holds its predecessor's
    total, and a row's byte offset truncated to 32 bits in a model of the gather."""
    for size, pat in SCALE_RINGS:
        w = _ring_weights(size, pat)
        nb, chunk, T = sc.geometry(size)
        bs = rorc.block_sums(w, size)
        n = 512
        seed = sc.BIG_SEED if size == sc.BIG else sc.SCAN_SEED
        good = rorc.sample_kernel_order(w, size, seed, sc.counter(n), n)
        noticed = 0
        for t in range(1, T):
            if bs[:t * chunk].sum() > 0 and bs[t * chunk:(t + 1) * chunk].sum() > 0:
                bad = rorc.sample_kernel_order(w, size, seed, sc.counter(n), n, ("drop_offset", t))
                assert not np.array_equal(bad, good), (size, pat, t)
                noticed += 1
        # (with two scan threads, thread 0's whole run is the zero run: thread 1's offset is 0)
        assert noticed >= (1 if T > 2 else 0), (size, pat)
        bad = rorc.sample_kernel_order(w, size, seed, sc.counter(n), n, ("stale_tail",))
        assert not np.array_equal(bad, good), (size, pat)
    # the gather: the drawn keys' 64-bit offsets against the same offsets kept to 32 bits
    w = _ring_weights(sc.BIG, "exact")
    for n in sc.BIG_NS:
        keys, _, _ = rorc.sample(w, sc.BIG, sc.BIG_SEED, sc.counter(n), n)
        full, cut = rorc.gather_offsets(keys, sc.ROW), rorc.gather_offsets(keys, sc.ROW, 32)
        assert np.array_equal(full, keys.astype(np.uint64) * np.uint64(sc.ROW))
        want, got = sc.ring_bytes(full, 16), sc.ring_bytes(cut, 16)
        high = keys >= sc.BAND[1]
        assert high.any() and np.array_equal(want[~high], got[~high])
        assert (want[high] != got[high]).any(axis=1).all(), n
    keys = sc.STEP_ROWS
    want = sc.ring_bytes(rorc.gather_offsets(keys, sc.ROW), 16)
    got = sc.ring_bytes(rorc.gather_offsets(keys, sc.ROW, 32), 16)
    assert ((want != got).any(axis=1) == (keys >= sc.BAND[1])).all()
    got31 = sc.ring_bytes(rorc.gather_offsets(keys, sc.ROW, 31), 16)
    assert ((want != got31).any(axis=1) == (keys >= sc.BAND[0])).all()


def test_large_ring_rows_are_regenerable_and_distinct():
    import torch
    rows = np.concatenate([sc.STEP_ROWS, sc.STEP_ROWS + sc.BIG, [4095, 4096, 2 * sc.BIG - 3]])
    a = sc.row_bytes(np, rows)
    b = sc.row_bytes(torch, torch.from_numpy(rows))
    assert a.shape == (len(rows), sc.ROW) and a.dtype == np.uint8 and np.array_equal(a, b.numpy())
    assert len({x.tobytes() for x in a}) == len(rows)
    assert np.array_equal(a[:3], sc.ring_bytes(rows[:3] * sc.ROW, sc.ROW))
    assert 200 < len(np.unique(a[5])) <= 256  # (not a constant fill)
    t = sc.row_targets(np, np.arange(2 * sc.BIG))
    assert t.dtype == np.float32 and np.isfinite(t).all() and len(np.unique(t)) == 2 * sc.BIG
    assert np.array_equal(t[rows], sc.row_targets(torch, torch.from_numpy(rows)).numpy())
    assert int(2 * sc.BIG * sc.ROW) * sc._MUL < 2 ** 63
