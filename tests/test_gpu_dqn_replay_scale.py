"""dqn_replay on the GPU at the ring sizes it runs at (tests/test_gpu_dqn_replay.py stops at three
block sums and 1535 rows, tests/test_gpu_dqn_inplace.py at row 999): the draw kernel's two-level
scan with 2, 3, 5, 8 and 27 active scan threads against the numpy restatement of its contract
(tests/dqn_replay_oracle.py), and a ring of 360 000 rows -- 4.42 GB of observations, the smallest
with rows on both sides of the byte offsets 2^31 (row 174 763) and 2^32 (row 349 526) -- for the
draw, the gather, the two-span append at a high cursor, the update and the learner step that
reads the drawn rows in place.  The inputs are tests/dqn_replay_scale_cases.py.

Input condition (not a tolerance on the kernel; tests/test_dqn_replay_host.py shows it on the CPU
for every draw made here): pattern (i), log-uniform priorities and alpha 0.6, needs every
u * total further from a prefix boundary than 1000 x the measured prefix discrepancy -- the largest
difference, over all rows, between the kernels' summation order, np.cumsum and an 80-bit prefix;
pattern (ii), priorities k / 8 and alpha 1, has exact sums in any order and needs 1e-13 (the two
roundings of u * total and the residual).  Both patterns hold exact zeros over the leading run,
one scan thread's entire run of blocks, and the trailing run.

Chosen on the CPU: seed 2025, counter 10 + n.  Margins and discrepancies, as fractions of the total:

    rows     discrepancy (i)   margin (i)  n = 1 / 33 / 512     margin (ii)  n = 1 / 33 / 512
    2567     9.2e-16           3.1e-3 / 2.5e-5 / 1.1e-6         3.3e-5 / 1.6e-5 / 6.4e-7
    5120     1.6e-15           1.9e-4 / 1.9e-5 / 6.4e-7         1.7e-4 / 1.3e-5 / 6.9e-8
    13311    4.0e-15           1.1e-5 / 1.9e-6 / 1.5e-7         5.5e-5 / 4.3e-7 / 2.5e-7
    33281    5.6e-15           3.5e-5 / 7.1e-8 / 4.0e-8         1.6e-6 / 7.1e-8 / 8.5e-8
    360000   2.0e-14           -      / 4.8e-8 / 2.8e-9         (keys per band 11, 21, 1 and 242, 251, 19)

after the update at high keys (seed 2025, counter 7, n 512; the four outcomes of its duplicated
keys): discrepancy 1.2e-14 .. 1.8e-14, margin 3.9e-10 .. 5.9e-9, each updated key drawn 7 to 26
times.  (At 1 000 000 rows, the size conf/agent/apex.yaml runs, the discrepancy is 1.9e-14.)

Tolerances: keys exact; probabilities 1e-6 rel in pattern (i) (a float32 rounding of a float64
quotient whose total may differ in the last places) and exact in pattern (ii) (both sides round
one exact float64 quotient once); weights 1e-14 rel; gathered rows, appended rows and the step's
outputs bitwise; n-step targets rtol 1e-6 + atol 1e-6, all as tests/test_gpu_dqn_replay.py
states them."""
import time

import numpy as np
import pytest
import torch

import dqn_replay_oracle as rorc
import dqn_replay_scale_cases as sc

pytestmark = pytest.mark.gpu
OBS = (3, 64, 64)
SLAB = 4096  # rows generated and appended at a time (50 MB of observations)
BIG = sc.BIG


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _native(dev, cap, alpha):
    from impala_amd.dqn import NativePrioritizedReplay
    return NativePrioritizedReplay(cap, priority_exponent=alpha, device=dev, seed=0)


def _rows(rows):
    """The transitions of the rows `rows` (an int64 tensor on the device), made on the device."""
    s = sc.row_bytes(torch, rows).reshape((-1,) + OBS)
    return s, sc.row_actions(rows), sc.row_targets(torch, rows)


def _fill(rb, size, pri):
    dev = rb.device
    p = torch.from_numpy(pri).to(dev)
    for lo in range(0, size, SLAB):
        rows = torch.arange(lo, min(size, lo + SLAB), device=dev)
        keys = rb.extend(_rows(rows), priorities=p[lo:lo + SLAB])
        assert torch.equal(keys, rows)
    assert len(rb) == size


def _set_priorities(rb, pri):
    """Every row's priority (and weight) through dqn_replay_update."""
    rb.update(torch.arange(len(pri)), torch.from_numpy(pri))


def _check_invariant(rb, alpha=sc.ALPHA):
    """weights == priorities ** alpha over the whole ring, to 1e-14 rel."""
    w = rb.weights().cpu().numpy()
    np.testing.assert_allclose(w, rorc.weights(rb.priorities.cpu().numpy(), alpha), rtol=1e-14, atol=0)
    return w


def _check_rows(got, keys):
    """Bitwise: the gathered (s, a, target) against the regenerated rows at `keys`."""
    s, a, t = _rows(keys)
    assert torch.equal(got[0], s) and torch.equal(got[1], a) and torch.equal(got[2], t)
    assert len(torch.unique(keys)) == len({x.cpu().numpy().tobytes() for x in got[0]})  # rows differ


def _draw_and_check(rb, pri, alpha, pattern, seed, counter, n):
    """One draw against the oracle on the priorities `pri`; -> the keys (numpy)."""
    size = len(rb)
    w = rorc.weights(pri, alpha)
    ref_keys, ref_probs, margin = rorc.sample(w, size, seed, counter, n)
    disc = rorc.prefix_discrepancy(w, size)
    print(f"rows {size} {pattern} n {n} seed {seed} counter {counter}: margin {margin:.3g} "
          f"discrepancy {disc:.3g}" + (f" keys per band {sc.bands(ref_keys)}" if size == BIG else ""))
    # a condition on the inputs, not a tolerance on the kernel
    assert sc.condition(pattern, margin, disc), f"pick another seed: margin {margin}, discrepancy {disc}"
    dw = _check_invariant(rb, alpha)
    if pattern == "uniform":
        # x ** 1 is x: the device weights are the exact ones
        off = dw[:size] != w
        assert not off.any(), (f"{int(off.sum())} of {size} weights are not their priority, by up to "
                               f"{np.max(np.abs(dw[:size][off] / w[off] - 1)):.3g} rel")
    rb.reset(seed)
    rb._counter = counter
    keys, rows, probs = rb.sample(n)
    torch.cuda.synchronize()
    k = keys.cpu().numpy()
    assert k.dtype == np.int64 and np.array_equal(k, ref_keys)
    if pattern == "uniform":
        assert np.array_equal(probs.cpu().numpy(), ref_probs)
    else:
        np.testing.assert_allclose(probs.cpu().numpy(), ref_probs, rtol=1e-6, atol=0)
    assert np.all(w[k] > 0)  # no zero-weight row is drawn
    # the gather: the regenerated rows, and torch's indexing of the ring
    _check_rows(rows, keys)
    assert torch.equal(rows[0], rb.s[keys]) and torch.equal(rows[1], rb.a[keys])
    assert torch.equal(rows[2], rb.target[keys])
    # keys and probabilities alone
    rb._counter = counter
    k2, none, p2 = rb.sample(n, gather=False)
    assert none is None and torch.equal(k2, keys) and torch.equal(p2, probs)
    return k


# ---------------------------------------------------------------- the scan
SCAN_RINGS = [(size, pat) for size in sc.SCAN_SHAPES for pat in sc.PATTERNS]


@pytest.fixture(scope="module", params=SCAN_RINGS, ids=lambda r: f"rows{r[0]}_{r[1]}")
def scan_ring(request):
    dev = _dev()
    size, pattern = request.param
    pri, alpha = sc.priorities(size, pattern)
    rb = _native(dev, size, alpha)
    _fill(rb, size, pri)
    yield rb, pri, alpha, pattern
    rb.close()
    del rb
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", sc.NS)
def test_scan_draws_equal_the_oracle(scan_ring, n):
    rb, pri, alpha, pattern = scan_ring
    assert sc.geometry(len(rb)) == sc.SCAN_SHAPES[len(rb)]
    _draw_and_check(rb, pri, alpha, pattern, sc.SCAN_SEED, sc.counter(n), n)


# ---------------------------------------------------------------- the large ring
@pytest.fixture(scope="module")
def big():
    """The one 360 000-row ring of this module, filled on the device with pattern (i); every test
    sets the priorities it needs and leaves the rows as first filled."""
    dev = _dev()
    rb = _native(dev, BIG, sc.ALPHA)
    pri, _ = sc.priorities(BIG, "exact")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _fill(rb, BIG, pri)
    torch.cuda.synchronize()
    print(f"large ring: {BIG} rows, {BIG * sc.ROW / 1e9:.2f} GB, filled in {time.perf_counter() - t0:.2f} s")
    assert (rb.size, rb._cursor) == (BIG, 0)
    yield rb
    rb.close()
    del rb
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", sc.BIG_NS)
def test_large_ring_draw_and_gather(big, n):
    rb = big
    pri, alpha = sc.priorities(BIG, "exact")
    _set_priorities(rb, pri)
    k = _draw_and_check(rb, pri, alpha, "exact", sc.BIG_SEED, sc.counter(n), n)
    # rows on all three sides of the byte offsets 2^31 and 2^32
    assert min(sc.bands(k)) >= 1, sc.bands(k)


def _advance_to(rb, target):
    """Move the cursor to `target` by appending the ring's own rows (copies of them) where they
    already lie: rows and priorities stay as they are."""
    cap, cur = rb.capacity, rb._cursor
    todo = (target - cur) % cap
    while todo:
        n = min(SLAB, todo, cap - cur)
        sl = slice(cur, cur + n)
        keys = rb.extend((rb.s[sl].clone(), rb.a[sl].clone(), rb.target[sl].clone()),
                         priorities=rb.priorities[sl].clone())
        assert int(keys[0]) == cur and int(keys[-1]) == cur + n - 1
        cur, todo = (cur + n) % cap, todo - n
    assert (rb.size, rb._cursor) == (cap, target)


def _snapshot(rb, row):
    return tuple(x[row].clone() for x in (rb.s, rb.a, rb.target, rb.priorities)) + (rb.weights()[row].clone(),)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_large_ring_wrap_at_a_high_cursor(big):
    rb = big
    dev, cap = rb.device, BIG
    base, _ = sc.priorities(BIG, "exact")
    _set_priorities(rb, base)
    touched = torch.cat([torch.arange(cap - 70, cap), torch.arange(0, 130)]).to(dev)
    try:
        # an extend of 200 rows from cursor cap - 70: 70 rows at the end, 130 at the start
        _advance_to(rb, cap - 70)
        m0 = float(rb.max_priority())
        outside = (cap - 71, 130)
        before = [_snapshot(rb, r) for r in outside]
        want_keys = (torch.arange(200, device=dev) + (cap - 70)) % cap
        s, a, t = _rows(want_keys + BIG)  # the rows a second pass writes
        p = np.random.default_rng(7).uniform(0.1, 0.9, 200).astype(np.float32)
        p[150] = 2 * m0  # raises the maximum from a row past the wrap
        keys = rb.extend((s, a, t), priorities=p)
        assert torch.equal(keys, want_keys) and (rb.size, rb._cursor) == (cap, 130)
        for ring, src in ((rb.s, s), (rb.a, a), (rb.target, t), (rb.priorities, torch.from_numpy(p).to(dev))):
            assert torch.equal(ring[cap - 70:], src[:70]) and torch.equal(ring[:130], src[70:])
        assert float(rb.max_priority()) == 2 * m0
        for r, snap in zip(outside, before):
            assert _same(_snapshot(rb, r), snap), r
            _check_rows(tuple(x[r:r + 1] for x in (rb.s, rb.a, rb.target)), torch.tensor([r], device=dev))
        _check_invariant(rb)
        # a rollout of 100 transitions from cursor cap - 40: 40 at the end, 60 at the start
        _advance_to(rb, cap - 40)
        m1 = float(rb.max_priority())
        assert m1 == 2 * m0
        outside = (cap - 41, 60)
        before = [_snapshot(rb, r) for r in outside]
        L, K = 101, 100
        want_keys = (torch.arange(K, device=dev) + (cap - 40)) % cap
        rng = np.random.default_rng(101)
        s = sc.row_bytes(torch, (torch.arange(L, device=dev) + (cap - 40)) % cap + BIG).reshape((-1,) + OBS)
        a = torch.from_numpy(rng.integers(0, 15, L))
        r = rng.standard_normal(L).astype(np.float32)
        q_pi = (rng.standard_normal(L) * 2).astype(np.float32)
        q_star = (rng.standard_normal(L) * 2).astype(np.float32)
        done = np.zeros(L, dtype=bool)
        done[[0, 39, 40, 41, 70, L - 2]] = True  # the first step, across the wrap, the last one used
        q_pi[[5, 70]] = [3 * m1, -4 * m1]  # the largest priorities: before and after the wrap
        keys = rb.extend_rollout(s, a, torch.from_numpy(r), torch.from_numpy(done), torch.from_numpy(q_pi),
                                 torch.from_numpy(q_star), n_step=3, gamma=0.99)
        assert torch.equal(keys, want_keys) and (rb.size, rb._cursor) == (cap, 60)
        # the oracle gets the kernel's own inputs: gamma crosses the C boundary as a float
        target = rorc.nstep_targets(r, done, q_star, 3, float(np.float32(0.99)))
        np.testing.assert_allclose(rb.target[keys].cpu().numpy(), target, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(rb.priorities[keys].cpu().numpy(), np.abs(target - q_pi[:K]),
                                   rtol=1e-6, atol=1e-6)
        assert torch.equal(rb.s[cap - 40:], s[:40]) and torch.equal(rb.s[:60], s[40:K])
        assert torch.equal(rb.a[cap - 40:].cpu(), a[:40]) and torch.equal(rb.a[:60].cpu(), a[40:K])
        for row, snap in zip(outside, before):
            assert _same(_snapshot(rb, row), snap), row
        assert float(rb.max_priority()) == float(rb.priorities.max()) > 3.9 * m1
        assert int(rb.priorities.argmax()) == (cap - 40 + 70) % cap
        _check_invariant(rb)
    finally:  # the rows as first filled, for the tests that follow
        s, a, t = _rows(touched)
        rb.s[touched], rb.a[touched], rb.target[touched] = s, a, t
        _set_priorities(rb, base)
    _check_rows(tuple(x[touched] for x in (rb.s, rb.a, rb.target)), touched)


def test_large_ring_update_at_high_keys(big):
    rb = big
    base, _ = sc.priorities(BIG, "exact")
    _set_priorities(rb, base)
    m0 = float(rb.max_priority())
    rb.update(torch.from_numpy(sc.UPDATE_KEYS), torch.from_numpy(sc.UPDATE_VALUES))
    p = rb.priorities.cpu().numpy()
    uniq = np.unique(sc.UPDATE_KEYS)
    for key in uniq:
        assert p[key] in sc.UPDATE_VALUES[sc.UPDATE_KEYS == key], key  # one of the supplied values
    rest = np.ones(BIG, dtype=bool)
    rest[uniq] = False
    assert np.array_equal(p[rest], base[rest])
    assert float(rb.max_priority()) == max(m0, float(sc.UPDATE_VALUES.max()))
    # the next draw follows the oracle on the updated weights (_draw_and_check holds them to 1e-14)
    k = _draw_and_check(rb, p, sc.ALPHA, "exact", sc.UPDATE_SEED, sc.UPDATE_COUNTER, sc.UPDATE_N)
    print("draws per updated key", [int((k == key).sum()) for key in uniq])
    assert all((k == key).any() for key in uniq)


def _engine(dev, dtype, N, A):
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    m = AtariDQNModel(OBS, A, device=dev, dtype=dtype, seed=0)
    e = DqnEngine(m, batch_size=N)
    m._train_engine = e
    return m, e


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_on_rows_across_the_offsets(big, dtype):
    """dqn_train_step_replay_rows (three counters) and dqn_train_step_replay (a fourth) on a ring
    whose only rows of positive priority are the 16 edge rows, against dqn_train_step on the same
    rows taken out of the ring by torch's indexing: bitwise, as test_in_place_equals_gathered_bitwise
    and test_train_step_replay_equals_its_parts hold the paths to each other at small rings."""
    rb = big
    dev, N, A = rb.device, 33, 6
    edge = torch.from_numpy(sc.STEP_ROWS).to(dev)
    _set_priorities(rb, sc.step_priorities())
    rb.a[edge] = edge % A  # the ring's actions are row % 15: in range for these six actions
    (m1, e1), (m2, e2) = _engine(dev, dtype, N, A), _engine(dev, dtype, N, A)
    assert torch.equal(m1.flat, m2.flat)
    try:
        for c in range(4):
            rb.reset(sc.STEP_SEED)
            rb._counter = c
            keys, none, probs = rb.sample(N, gather=False)
            rb._counter = c
            before = rb.priorities.clone()
            step = e1.train_step_replay_rows if c < 3 else e1.train_step_replay
            keys1, prio1 = step(rb, sc.STEP_SEED, c)
            prio2 = e2.train_step(rb.s[keys], rb.a[keys], rb.target[keys], probs)
            torch.cuda.synchronize()
            k = keys.cpu().numpy()
            print(f"{dtype} counter {c}: keys per band {sc.bands(k)}, {len(np.unique(k))} distinct")
            # every drawn key is an edge row and several are drawn twice
            assert set(k.tolist()) <= set(sc.STEP_ROWS.tolist()) and len(np.unique(k)) < N
            if c == 0:  # (the priorities of the later draws are the step's own)
                ref_keys, _, margin = rorc.sample(rorc.weights(sc.step_priorities(), sc.ALPHA), BIG,
                                                  sc.STEP_SEED, 0, N)
                assert margin > 1e-9 and np.array_equal(k, ref_keys) and min(sc.bands(k)) >= 1
            assert torch.equal(keys1, keys), c
            assert torch.equal(prio1, prio2) and bool(torch.isfinite(prio2).all()), c
            assert torch.equal(m1.flat, m2.flat), c
            assert torch.equal(e1.exp_avg, e2.exp_avg) and torch.equal(e1.exp_avg_sq, e2.exp_avg_sq), c
            assert e1.metrics.numel() == 9 and torch.equal(e1.metrics, e2.metrics), c
            # the ring's priorities are what rb.update(keys, prio2) leaves: at a drawn key one of
            # its returned values, elsewhere what was there
            ring_p, p2, b = rb.priorities.cpu().numpy(), prio2.cpu().numpy(), before.cpu().numpy()
            for key in np.unique(k):
                assert ring_p[key] in p2[k == key], (c, key)
            rest = np.ones(BIG, dtype=bool)
            rest[k] = False
            assert np.array_equal(ring_p[rest], b[rest]), c
            _check_invariant(rb)
        assert float(e1.metrics[7]) == 4.0 and bool(torch.isfinite(m1.flat).all())
    finally:
        rb.a[edge] = sc.row_actions(edge)
        e1.close()
        e2.close()
    _check_rows(tuple(x[edge] for x in (rb.s, rb.a, rb.target)), edge)
