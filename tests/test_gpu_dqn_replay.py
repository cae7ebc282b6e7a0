"""dqn_replay on the GPU (include/dqn_hip.h) against the numpy restatement of its contract
(tests/dqn_replay_oracle.py): exact keys, probabilities, the gather, extend / update / rollout
ingest, and dqn_train_step_replay against its three parts.

Tolerances: keys exact (the inputs are first shown, on the reference alone, to keep every
u * total 1e-9 * total away from a prefix boundary -- the kernels' summation order, np.cumsum and an
80-bit prefix differ by at most 1.8e-15 * total at these sizes, 1 to 1535 rows, as
dqn_replay_oracle.prefix_discrepancy measures it: 4.3e-16 at 600 rows, 5.3e-16 at 513 and 777,
1.8e-15 at 1535; the rings of tests/test_gpu_dqn_replay_scale.py, 2567 to 360 000 rows, measure 9.2e-16 to
2.0e-14 and derive their condition from it); probabilities 1e-6 rel (a float32 rounding of a float64 quotient);
weights 1e-14 rel (device pow against numpy's, both within a few ulp of 2.2e-16); n-step targets
rtol 1e-6 + atol 1e-6 (<= 16 fp32 multiply-adds against float64)."""
import numpy as np
import pytest
import torch

import dqn_oracle as orc
import dqn_replay_oracle as rorc
from impala_amd import _lib

pytestmark = pytest.mark.gpu
B = _lib.DQN_REPLAY_BLOCK
ALPHA = 0.6
OBS = (3, 64, 64)
# (capacity, size): a partial ring, one row, a full ring, one row past a block, one short of three
SHAPES = [(1000, 777), (8, 1), (B + 88, B + 88), (B + 40, B + 1), (3 * B, 3 * B - 1)]
DRAW_SEED = 2024  # margins checked on the CPU for every (shape, n) below


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rows(n, start=0, seed=0):
    """n distinguishable transitions: random obs bytes, action = row id, target = row id / 8."""
    g = torch.Generator().manual_seed(1000 + seed)
    s = torch.randint(0, 256, (n,) + OBS, dtype=torch.uint8, generator=g)
    ids = torch.arange(start, start + n)
    return s, ids.clone(), ids.float() / 8


def shape_priorities(size):
    """Log-uniform over six decades, with exact zeros over a whole block and the last row."""
    rng = np.random.default_rng(size)
    p = (10.0 ** rng.uniform(-3, 3, size)).astype(np.float32)
    nb = (size + B - 1) // B
    if size == 1:
        return p
    p[-1] = 0.0
    if nb >= 3:
        p[B:2 * B] = 0.0
    elif nb == 2 and size - B > 1:
        p[:B] = 0.0          # the whole first block: every draw lands in the partial last block
    elif nb == 2:
        p[B:] = 0.0          # the last block is the last row alone
        p[100:200] = 0.0
    else:
        p[size // 3: size // 2] = 0.0
    return p


def _native(dev, cap, alpha=ALPHA, seed=0):
    from impala_amd.dqn import NativePrioritizedReplay
    return NativePrioritizedReplay(cap, priority_exponent=alpha, device=dev, seed=seed)


def _check_invariant(rb, alpha=ALPHA):
    """weights == priorities ** alpha over the whole ring, to 1e-14 rel."""
    w = rb.weights().cpu().numpy()
    expect = rorc.weights(rb.priorities.cpu().numpy(), alpha)
    np.testing.assert_allclose(w, expect, rtol=1e-14, atol=0)
    return w


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"cap{s[0]}_size{s[1]}")
def filled(request):
    dev = _dev()
    cap, size = request.param
    rb = _native(dev, cap)
    s, a, t = _rows(size, seed=size)
    pri = shape_priorities(size)
    keys = rb.extend((s, a, t), priorities=pri)
    assert keys.tolist() == list(range(size)) and len(rb) == size
    return rb, (s, a, t), pri


@pytest.mark.parametrize("n", [1, 33, 512])
def test_sample_keys_equal_the_oracle(filled, n):
    rb, (s, a, t), pri = filled
    size = len(rb)
    w = rorc.weights(pri, ALPHA)
    counter = 10 + n
    ref_keys, ref_probs, margin = rorc.sample(w, size, DRAW_SEED, counter, n)
    # a condition on the inputs, not a tolerance on the kernel
    assert margin > 1e-9, f"pick another seed: margin {margin}"
    rb.reset(DRAW_SEED)
    rb._counter = counter
    keys, (gs, ga, gt), probs = rb.sample(n)
    torch.cuda.synchronize()
    k = keys.cpu().numpy()
    assert k.dtype == np.int64 and np.array_equal(k, ref_keys)
    np.testing.assert_allclose(probs.cpu().numpy(), ref_probs, rtol=1e-6, atol=0)
    if size > 1:
        assert np.all(w[k] > 0)  # no zero-weight row is drawn
    kc = keys.cpu()
    assert torch.equal(gs.cpu(), s[kc]) and torch.equal(ga.cpu(), a[kc]) and torch.equal(gt.cpu(), t[kc])
    # keys and probabilities alone
    rb._counter = counter
    k2, none, p2 = rb.sample(n, gather=False)
    assert none is None and torch.equal(k2, keys) and torch.equal(p2, probs)
    _check_invariant(rb)


def test_all_zero_priorities_draw_uniformly():
    dev = _dev()
    rb = _native(dev, 700)
    size = 650
    rb.extend(_rows(size), priorities=np.zeros(size, dtype=np.float32))
    rb.reset(5)
    keys, _, probs = rb.sample(512, gather=False)
    u = rorc.uniforms(5, 0, 512)
    assert np.array_equal(keys.cpu().numpy(), np.floor(u * size).astype(np.int64))
    assert np.all(probs.cpu().numpy() == np.float32(1.0 / size))


def test_draw_frequencies_and_reproducibility():
    """cap 64, 20 000 draws over 40 calls: chi-square against w / sum w at p = 1e-6, the
    significance of test_gpu_dqn.py's eps-0.4 draw test."""
    from scipy.stats import chi2 as chi2_dist
    dev = _dev()
    rb = _native(dev, 64, seed=77)
    pri = np.random.default_rng(3).uniform(0.05, 4.0, 64).astype(np.float32)
    pri[[5, 63]] = 0.0
    rb.extend(_rows(64), priorities=pri)
    w = rorc.weights(pri, ALPHA)
    counts = np.zeros(64)
    draws = []
    for c in range(40):
        k, _, _ = rb.sample(500, gather=False)
        draws.append(k)
        counts += np.bincount(k.cpu().numpy(), minlength=64)
    live = w > 0
    assert counts[~live].sum() == 0
    exp = 20000 * w[live] / w.sum()
    stat = float(((counts[live] - exp) ** 2 / exp).sum())
    print("replay draw chi2 (%d dof)" % (live.sum() - 1), stat)
    assert stat < chi2_dist.isf(1e-6, int(live.sum()) - 1)
    # the same (seed, counter) again: bitwise equal; another counter differs
    rb.reset(77)
    again = [rb.sample(500, gather=False) for _ in range(2)]
    assert torch.equal(again[0][0], draws[0]) and torch.equal(again[1][0], draws[1])
    assert not torch.equal(draws[0], draws[1])
    rb._counter = 0
    k, _, p = rb.sample(500, gather=False)
    assert torch.equal(k, again[0][0]) and torch.equal(p, again[0][2])


def test_extend_wraps_and_tracks_the_maximum():
    dev = _dev()
    alpha = 0.7
    rb = _native(dev, 10, alpha=alpha)
    s1, a1, t1 = _rows(7)
    k = rb.extend((s1, a1, t1), priorities=torch.tensor([.5, .25, 1.5, 0., 2., .125, .75]))
    assert k.tolist() == list(range(7)) and (rb.size, rb._cursor) == (7, 7)
    assert float(rb.max_priority()) == 2.0  # given priorities raise the maximum (from 1)
    _check_invariant(rb, alpha)
    rb.update(torch.tensor([1, 4]), torch.tensor([7.5, 0.5]))  # an update raises it
    assert float(rb.max_priority()) == 7.5
    s2, a2, t2 = _rows(6, start=100, seed=1)
    k = rb.extend((s2, a2, t2))  # crosses the end: rows 7, 8, 9, 0, 1, 2; no priorities
    assert k.tolist() == [7, 8, 9, 0, 1, 2] and (rb.size, rb._cursor) == (10, 3)
    assert rb.priorities.tolist() == [7.5, 7.5, 7.5, 0., .5, .125, .75, 7.5, 7.5, 7.5]
    assert rb.a.tolist() == [103, 104, 105, 3, 4, 5, 6, 100, 101, 102]
    assert rb.target.tolist() == [x / 8 for x in rb.a.tolist()]
    kc = k.cpu()
    assert torch.equal(rb.s[kc].cpu(), s2) and torch.equal(rb.s[3:7].cpu(), s1[3:7])
    _check_invariant(rb, alpha)
    # smaller given priorities leave the maximum
    rb.extend(_rows(2, start=200), priorities=[0.1, 0.2])
    assert float(rb.max_priority()) == 7.5 and (rb.size, rb._cursor) == (10, 5)
    _check_invariant(rb, alpha)
    # per-transition items, as ReplayBuffer.extend takes them
    items = [(s.unsqueeze(0), a.reshape(1), t.reshape(1)) for s, a, t in zip(*_rows(2, start=300))]
    assert rb.extend(items).tolist() == [5, 6] and rb.a[5:7].tolist() == [300, 301]
    # refused: more rows than the ring holds, straight at the entry point
    s, a, t = (x.to(dev) for x in _rows(11))
    st = _lib.lib().dqn_replay_extend(rb._h, _lib.ptr(s), _lib.ptr(a), _lib.ptr(t), None, 11, None,
                                      _lib.stream_ptr(None))
    assert st == 1001 and b"capacity" in _lib.lib().dqn_last_error()
    with pytest.raises(ValueError):
        rb.extend((s, a, t))


def test_update_with_duplicate_keys_keeps_the_invariant():
    dev = _dev()
    rb = _native(dev, 300)
    rb.extend(_rows(300), priorities=np.full(300, 0.5, dtype=np.float32))
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 300, 512)
    keys[:6] = [17, 17, 17, 250, 250, 3]
    vals = rng.uniform(0.01, 3.0, 512).astype(np.float32)
    vals[100] = 9.25  # the maximum, on whichever key it sits
    rb.update(torch.from_numpy(keys), torch.from_numpy(vals))
    p = rb.priorities.cpu().numpy()
    for key in np.unique(keys):
        assert p[key] in vals[keys == key], key  # one of the supplied values
    untouched = np.setdiff1d(np.arange(300), keys)
    assert np.all(p[untouched] == 0.5)
    _check_invariant(rb)
    assert float(rb.max_priority()) == 9.25
    rb.async_update(torch.tensor([0]), torch.tensor([0.0]))
    assert float(rb.priorities[0]) == 0.0 and float(rb.weights()[0]) == 0.0
    assert float(rb.max_priority()) == 9.25


def _rollout(L, seed):
    rng = np.random.default_rng(seed)
    s = torch.from_numpy(rng.integers(0, 256, (L,) + OBS, dtype=np.uint8))
    a = torch.from_numpy(rng.integers(0, 15, L))
    r = rng.standard_normal(L).astype(np.float32)
    q_pi = (rng.standard_normal(L) * 2).astype(np.float32)
    q_star = (rng.standard_normal(L) * 2).astype(np.float32)
    done = np.zeros(L, dtype=bool)
    done[0] = True                      # the first step
    done[L - 2] = True                  # the last step a target uses
    if L > 20:
        done[[40, 41, 42, 70]] = True   # adjacent steps
    return s, a, r, done, q_pi, q_star


@pytest.mark.parametrize("L", [2, 3, 101])
@pytest.mark.parametrize("n_step", [1, 3, 16])
def test_extend_rollout_matches_the_float64_oracle(L, n_step):
    dev = _dev()
    rb = _native(dev, 128)
    rb.extend(_rows(90), priorities=np.full(90, 0.5, dtype=np.float32))  # L = 101 wraps
    s, a, r, done, q_pi, q_star = _rollout(L, 10 * L + n_step)
    keys = rb.extend_rollout(s, a, torch.from_numpy(r), torch.from_numpy(done), torch.from_numpy(q_pi),
                             torch.from_numpy(q_star), n_step=n_step, gamma=0.99)
    K = L - 1
    assert keys.tolist() == [(90 + i) % 128 for i in range(K)]
    assert rb.size == min(128, 90 + K) and rb._cursor == (90 + K) % 128
    kc = keys.cpu()
    # the oracle gets the kernel's own inputs: gamma crosses the C boundary as a float
    target = rorc.nstep_targets(r, done, q_star, n_step, float(np.float32(0.99)))
    np.testing.assert_allclose(rb.target[keys].cpu().numpy(), target, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(rb.priorities[keys].cpu().numpy(), np.abs(target - q_pi[:K]),
                               rtol=1e-6, atol=1e-6)
    assert torch.equal(rb.s.cpu()[kc], s[:K]) and torch.equal(rb.a.cpu()[kc], a[:K])
    _check_invariant(rb)
    assert float(rb.max_priority()) == max(1.0, float(rb.priorities[keys].max()))


def test_large_ingest_over_many_workgroups_and_the_wrap():
    """extend and extend_rollout are one thread per row: more rows than one workgroup, crossing
    the end of the ring; the maximum is raised from rows on both sides of the wrap."""
    dev = _dev()
    rb = _native(dev, 1000)
    rng = np.random.default_rng(12)
    pri = rng.uniform(0.01, 0.9, 700).astype(np.float32)
    pri[650] = 3.5
    rb.extend(_rows(700), priorities=pri)
    assert float(rb.max_priority()) == 3.5 and (rb.size, rb._cursor) == (700, 700)
    L = 601
    s, a, r, done, q_pi, q_star = _rollout(L, 77)
    q_pi[[5, 450]] = [40.0, -60.0]  # the largest priorities: before and after the wrap
    keys = rb.extend_rollout(s, a, torch.from_numpy(r), torch.from_numpy(done), torch.from_numpy(q_pi),
                             torch.from_numpy(q_star), n_step=3, gamma=0.99)
    assert keys.tolist() == [(700 + i) % 1000 for i in range(600)]
    assert (rb.size, rb._cursor) == (1000, 300)
    target = rorc.nstep_targets(r, done, q_star, 3, float(np.float32(0.99)))
    np.testing.assert_allclose(rb.target[keys].cpu().numpy(), target, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(rb.priorities[keys].cpu().numpy(), np.abs(target - q_pi[:600]),
                               rtol=1e-6, atol=1e-6)
    kc = keys.cpu()
    assert torch.equal(rb.s.cpu()[kc], s[:600]) and torch.equal(rb.a.cpu()[kc], a[:600])
    assert float(rb.max_priority()) == float(rb.priorities.max()) > 50
    assert int(rb.priorities.argmax()) == (700 + 450) % 1000
    _check_invariant(rb)
    # a full-ring extend from a cursor in the middle, given priorities
    pri2 = rng.uniform(0.01, 0.9, 1000).astype(np.float32)
    pri2[990] = 99.0  # lands after the wrap
    s2, a2, t2 = _rows(1000, start=5000, seed=3)
    k2 = rb.extend((s2, a2, t2), priorities=pri2)
    assert k2.tolist() == [(300 + i) % 1000 for i in range(1000)] and (rb.size, rb._cursor) == (1000, 300)
    assert torch.equal(rb.a.cpu()[k2.cpu()], a2) and torch.equal(rb.s.cpu()[k2.cpu()], s2)
    np.testing.assert_array_equal(rb.priorities.cpu().numpy()[k2.cpu().numpy()], pri2)
    assert float(rb.max_priority()) == 99.0
    _check_invariant(rb)


def _learner_pair(dev, dtype, N=33, A=6, ring=200):
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    out = []
    for _ in range(2):
        m = AtariDQNModel(OBS, A, device=dev, dtype=dtype, seed=0)
        e = DqnEngine(m, batch_size=N)
        m._train_engine = e
        rb = _native(dev, ring)
        obs, act, tgt, _ = orc.synthetic_batch(ring, A, seed=21, probs=False)
        pri = np.random.default_rng(4).uniform(0.05, 3.0, ring).astype(np.float32)
        rb.extend(tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (obs, act, tgt)), priorities=pri)
        out.append((m, e, rb))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_step_replay_equals_its_parts(dtype):
    dev = _dev()
    (m1, e1, rb1), (m2, e2, rb2) = _learner_pair(dev, dtype)
    assert torch.equal(m1.flat, m2.flat)
    for c in range(3):
        keys1, prio1 = e1.train_step_replay(rb1, seed=99, counter=c)
        rb2.reset(99)
        rb2._counter = c
        keys2, (s, a, t), probs = rb2.sample(33)
        prio2 = e2.train_step(s, a, t, probs)
        rb2.update(keys2, prio2)
        torch.cuda.synchronize()
        assert torch.equal(keys1, keys2), c
        assert torch.equal(prio1, prio2), c
        assert torch.equal(m1.flat, m2.flat) and torch.equal(e1.exp_avg, e2.exp_avg), c
        assert torch.equal(e1.metrics, e2.metrics), c
        assert torch.equal(rb1.priorities, rb2.priorities), c
        assert torch.equal(rb1.weights(), rb2.weights()), c
    assert float(e1.metrics[7]) == 3.0
    _check_invariant(rb1)
    # refused: an empty replay
    empty = _native(dev, 16)
    with pytest.raises(RuntimeError, match="empty"):
        e1.train_step_replay(empty, 1, 0)


def test_learner_over_the_native_replay_and_the_old_path():
    from impala_amd import dqn
    from impala_amd.config import load_config
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size = 64
    b = dqn.ApexDQNBuilder(cfg)
    model = b.make_network()
    rb = b.make_replay(native=True)
    assert isinstance(rb, dqn.NativePrioritizedReplay) and rb.capacity == 64 and rb.alpha == 0.6
    assert type(b.make_replay()) is dqn.PrioritizedReplay
    obs, act, tgt, _ = orc.synthetic_batch(40, 15, seed=8, probs=False)
    items = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (obs, act, tgt))
    pri = np.random.default_rng(1).uniform(0.1, 2.0, 40).astype(np.float32)
    rb.extend(items, priorities=pri)
    kw = b.learner_kwargs()
    kw["learning_starts"] = 40
    learner = dqn.ApexLearner(model, rb, batch_size=33, **kw)
    learner.prepare()
    calls0 = dqn.REPLAY_STEP_CALLS
    expected = {"train_step/" + k for k in ("q", "target", "priorities", "loss", "grad_norm")} | {
        "debug/priority_update_time", "debug/replay_sample_per_second", "debug/gradient_per_second",
        "debug/forward_dt", "debug/target_sync_time", "debug/update_time", "debug/total_time"}
    for i in range(3):
        met = learner.train_step()
        assert set(met) == expected
        assert float(learner.engine.metrics[7]) == i + 1  # the step metric advances
        assert all(np.isfinite(float(met["train_step/" + k])) for k in ("q", "loss", "grad_norm"))
        keys, prio = learner.last_keys, learner.last_priorities
        assert keys.shape == (33,) and int(keys.min()) >= 0 and int(keys.max()) < 40
        # the ring holds the returned priority at every sampled key (of a key drawn more than
        # once: one of its returned values, as dqn_replay_update leaves it)
        ring_p, k_np, p_np = rb.priorities.cpu().numpy(), keys.cpu().numpy(), prio.cpu().numpy()
        for key in np.unique(k_np):
            assert ring_p[key] in p_np[k_np == key], (i, key)
    assert dqn.REPLAY_STEP_CALLS == calls0 + 3
    # the plain replay still takes the old path: the new entry is not called
    model2 = dqn.AtariDQNModel(OBS, 15, device=dev, seed=0)
    plain = dqn.PrioritizedReplay(64, device=dev, seed=0)
    plain.extend(tuple(x.to(dev) for x in items), priorities=pri)
    learner2 = dqn.ApexLearner(model2, plain, batch_size=33, **kw)
    before = plain.priorities.clone()
    met = learner2.train_step()
    assert set(met) == expected and dqn.REPLAY_STEP_CALLS == calls0 + 3
    assert not torch.equal(plain.priorities, before)
