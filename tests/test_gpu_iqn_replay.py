"""iqn_replay on the GPU (include/iqn_hip.h): the [W]-target ring through dqn_replay's sampler
against the numpy restatement of its contract (tests/dqn_replay_oracle.py), the wide extend, the
fused n-step ingest against iqn_nstep_targets (bitwise) and the float64 restatement
(tests/iqn_oracle.py), iqn_train_step_replay against its three parts (bitwise), and the builder ->
actor -> replay -> learner path.

Tolerances are the project's existing ones: keys exact (the inputs are first shown, on the
reference alone, to keep every u * total 1e-9 * total from a prefix boundary; the margins of the
two draws here, as dqn_replay_oracle.sample reports them, are 1.9e-3 and 9.7e-5), probabilities 1e-6 rel, weights 1e-14 rel
(tests/test_gpu_dqn_replay.py); n-step targets rtol 1e-6 + atol 1e-6 and priorities within
(n_step + W + 2) 2^-24 of the return of the magnitudes (tests/test_gpu_iqn.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dqn_oracle as dorc
import dqn_replay_oracle as rorc
import iqn_oracle as orc
import iqn_step_oracle as so
from impala_amd import _lib
from test_gpu_dqn_replay import shape_priorities

pytestmark = pytest.mark.gpu
ALPHA = 0.6
OBS = (3, 64, 64)
DRAW_SEED = 2024


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _native(dev, cap, W, alpha=ALPHA, seed=0):
    from impala_amd.iqn import NativeQuantileReplay
    return NativeQuantileReplay(cap, W, priority_exponent=alpha, device=dev, seed=seed)


def _rows(n, W, start=0, seed=0):
    """n distinguishable transitions: random obs bytes, action = row id, target[k] = row id + k / 64."""
    g = torch.Generator().manual_seed(1000 + seed)
    s = torch.randint(0, 256, (n,) + OBS, dtype=torch.uint8, generator=g)
    ids = torch.arange(start, start + n)
    return s, ids.clone(), ids.float().unsqueeze(1) + torch.arange(W).float() / 64


def _check_invariant(rb, alpha=ALPHA):
    """weights == priorities ** alpha over the whole ring, to 1e-14 rel."""
    w = rb.weights().cpu().numpy()
    np.testing.assert_allclose(w, rorc.weights(rb.priorities.cpu().numpy(), alpha), rtol=1e-14, atol=0)


# ---------------------------------------------------------------- 1. sampling
@pytest.fixture(scope="module")
def filled():
    dev = _dev()
    rb = _native(dev, 1000, 8)
    s, a, t = _rows(777, 8, seed=777)
    pri = shape_priorities(777)
    keys = rb.extend((s, a, t), priorities=pri)
    assert keys.tolist() == list(range(777)) and len(rb) == 777 and rb.target.shape == (1000, 8)
    return rb, (s, a, t), pri


@pytest.mark.parametrize("n", [1, 33])
def test_sample_through_the_new_handle(filled, n):
    rb, (s, a, t), pri = filled
    w = rorc.weights(pri, ALPHA)
    counter = 10 + n
    ref_keys, ref_probs, margin = rorc.sample(w, 777, DRAW_SEED, counter, n)
    print(f"n {n}: margin {margin:.3g}")
    assert margin > 1e-9, f"pick another seed: margin {margin}"  # a condition on the inputs
    rb.reset(DRAW_SEED)
    rb._counter = counter
    keys, (gs, ga, gt), probs = rb.sample(n)
    torch.cuda.synchronize()
    k = keys.cpu().numpy()
    assert k.dtype == np.int64 and np.array_equal(k, ref_keys)
    np.testing.assert_allclose(probs.cpu().numpy(), ref_probs, rtol=1e-6, atol=0)
    assert np.all(w[k] > 0)
    kc = keys.cpu()
    assert gt.shape == (n, 8)
    assert torch.equal(gs.cpu(), s[kc]) and torch.equal(ga.cpu(), a[kc]) and torch.equal(gt.cpu(), t[kc])
    assert torch.equal(gt, rb.target[keys]) and torch.equal(gs, rb.s[keys])
    rb._counter = counter
    k2, none, p2 = rb.sample(n, gather=False)
    assert none is None and torch.equal(k2, keys) and torch.equal(p2, probs)
    _check_invariant(rb)
    np.testing.assert_allclose(rb.probabilities().cpu().numpy(), (w / w.sum()).astype(np.float32), rtol=1e-6)


# ---------------------------------------------------------------- 2. wide extend
@pytest.mark.parametrize("W", [5, 32])
def test_wide_extend_across_the_wrap(W):
    dev = _dev()
    alpha = 0.7
    rb = _native(dev, 8, W, alpha=alpha)
    s1, a1, t1 = _rows(6, W)
    k = rb.extend((s1, a1, t1), priorities=torch.tensor([.5, .25, 1.5, 0., 2., .125]))
    assert k.tolist() == list(range(6)) and (rb.size, rb._cursor) == (6, 6)
    assert float(rb.max_priority()) == 2.0
    assert torch.equal(rb.target[:6].cpu(), t1)
    _check_invariant(rb, alpha)
    s2, a2, t2 = _rows(4, W, start=100, seed=1)
    k = rb.extend((s2, a2, t2))  # slots 6, 7, 0, 1; no priorities: the running maximum
    assert k.tolist() == [6, 7, 0, 1] and (rb.size, rb._cursor) == (8, 2)
    assert rb.priorities.tolist() == [2., 2., 1.5, 0., 2., .125, 2., 2.]
    assert rb.a.tolist() == [102, 103, 2, 3, 4, 5, 100, 101]
    kc = k.cpu()
    assert torch.equal(rb.target.cpu()[kc], t2) and torch.equal(rb.target[2:6].cpu(), t1[2:6])
    assert torch.equal(rb.s.cpu()[kc], s2) and torch.equal(rb.s[2:6].cpu(), s1[2:6])
    assert float(rb.max_priority()) == 2.0
    _check_invariant(rb, alpha)
    # per-transition items, as ReplayBuffer.extend takes them
    items = [(s.unsqueeze(0), a.reshape(1), t) for s, a, t in zip(*_rows(2, W, start=300))]
    assert rb.extend(items, priorities=[0.1, 7.5]).tolist() == [2, 3]
    assert rb.a[2:4].tolist() == [300, 301] and float(rb.max_priority()) == 7.5
    assert torch.equal(rb.target[2:4].cpu(), _rows(2, W, start=300)[2])
    # an update with duplicate keys
    keys = torch.tensor([1, 1, 1, 5, 5, 7])
    vals = torch.tensor([.3, .6, .9, 1.25, 9.5, .75])
    rb.update(keys, vals)
    p = rb.priorities.cpu().numpy()
    for key in (1, 5, 7):
        assert p[key] in vals.numpy()[keys.numpy() == key]
    assert float(rb.max_priority()) == 9.5
    _check_invariant(rb, alpha)
    # refused with a ring: more rows than it holds, straight at the entry point
    s, a, t = (x.to(dev) for x in _rows(9, W))
    st = _lib.lib().iqn_replay_extend(rb._h, _lib.ptr(s), _lib.ptr(a), _lib.ptr(t), None, 9, None,
                                      _lib.stream_ptr(None))
    assert st == 1001 and b"capacity" in _lib.lib().iqn_last_error()
    with pytest.raises(ValueError):
        rb.extend((s, a, t))


# ---------------------------------------------------------------- 3. fused ingest
def _rollout(L, W, seed):
    """tests/test_gpu_dqn_replay.py's rollout with q_star [L, W]: dones on the first step, on the
    last step a target uses, and on adjacent steps."""
    rng = np.random.default_rng(seed)
    s = torch.from_numpy(rng.integers(0, 256, (L,) + OBS, dtype=np.uint8))
    a = torch.from_numpy(rng.integers(0, 15, L))
    r = rng.standard_normal(L).astype(np.float32)
    q_pi = (rng.standard_normal(L) * 2).astype(np.float32)
    q_star = (rng.standard_normal((L, W)) * 2).astype(np.float32)
    done = np.zeros(L, dtype=bool)
    done[0] = True
    done[L - 2] = True
    if L > 20:
        done[[40, 41, 42, 70]] = True
    return s, a, r, done, q_pi, q_star


def _hold_ingest(rb, keys, r, done, q_pi, q_star, n_step, dev):
    """The ring rows at `keys` against iqn_nstep_targets (bitwise) and the float64 restatement."""
    from impala_amd.iqn import iqn_nstep_targets
    W = q_star.shape[1]
    tg, prio = iqn_nstep_targets(_t(r, dev), _t(done, dev), _t(q_pi, dev), _t(q_star, dev), n_step, 0.99)
    assert torch.equal(rb.target[keys], tg) and torch.equal(rb.priorities[keys], prio)
    # the oracle gets the kernel's own inputs: gamma crosses the C boundary as a float
    g = float(np.float32(0.99))
    want_t, want_p = orc.nstep_targets(r, done, q_pi, q_star, n_step, g)
    got_t, got_p = rb.target[keys].cpu().numpy(), rb.priorities[keys].cpu().numpy()
    np.testing.assert_allclose(got_t, want_t, rtol=1e-6, atol=1e-6)
    mag, _ = orc.nstep_targets(np.abs(r), done, q_pi, np.abs(q_star), n_step, g)
    bound = (n_step + W + 2) * 2.0 ** -24 * (mag.mean(1) + np.abs(q_pi[:-1]))
    assert np.all(np.abs(got_p - want_p) <= bound)


@pytest.mark.parametrize("n_step", [1, 3, 16])
@pytest.mark.parametrize("L", [2, 3, 101])
@pytest.mark.parametrize("W", [1, 5, 8, 32])
def test_fused_ingest_is_iqn_nstep_targets(W, L, n_step):
    dev = _dev()
    rb = _native(dev, 128, W)
    rb.extend(_rows(90, W), priorities=np.full(90, 0.5, dtype=np.float32))  # L = 101 wraps
    s, a, r, done, q_pi, q_star = _rollout(L, W, 1000 * W + 10 * L + n_step)
    keys = rb.extend_rollout(s, a, torch.from_numpy(r), torch.from_numpy(done), torch.from_numpy(q_pi),
                             torch.from_numpy(q_star), n_step=n_step, gamma=0.99)
    K = L - 1
    assert keys.tolist() == [(90 + i) % 128 for i in range(K)]
    assert rb.size == min(128, 90 + K) and rb._cursor == (90 + K) % 128
    _hold_ingest(rb, keys, r, done, q_pi, q_star, n_step, dev)
    kc = keys.cpu()
    assert torch.equal(rb.s.cpu()[kc], s[:K]) and torch.equal(rb.a.cpu()[kc], a[:K])
    _check_invariant(rb)
    assert float(rb.max_priority()) == max(1.0, float(rb.priorities[keys].max()))


# ---------------------------------------------------------------- 4. many workgroups
def test_large_ingest_over_many_workgroups_and_the_wrap():
    """L = 601 at W = 32 is 75 workgroups of 8 transitions; the ring of 1000 wraps after 300 of
    them and the two largest priorities sit on either side of the wrap."""
    dev = _dev()
    W = 32
    rb = _native(dev, 1000, W)
    rng = np.random.default_rng(12)
    pri = rng.uniform(0.01, 0.9, 700).astype(np.float32)
    pri[650] = 3.5
    rb.extend(_rows(700, W), priorities=pri)
    assert float(rb.max_priority()) == 3.5 and (rb.size, rb._cursor) == (700, 700)
    s, a, r, done, q_pi, q_star = _rollout(601, W, 77)
    q_pi[[5, 450]] = [40.0, -60.0]  # the largest priorities: before and after the wrap
    keys = rb.extend_rollout(s, a, torch.from_numpy(r), torch.from_numpy(done), torch.from_numpy(q_pi),
                             torch.from_numpy(q_star), n_step=3, gamma=0.99)
    assert keys.tolist() == [(700 + i) % 1000 for i in range(600)]
    assert (rb.size, rb._cursor) == (1000, 300)
    _hold_ingest(rb, keys, r, done, q_pi, q_star, 3, dev)
    kc = keys.cpu()
    assert torch.equal(rb.s.cpu()[kc], s[:600]) and torch.equal(rb.a.cpu()[kc], a[:600])
    assert float(rb.max_priority()) == float(rb.priorities.max()) > 50
    assert int(rb.priorities.argmax()) == (700 + 450) % 1000
    second = rb.priorities.clone()
    second[150] = 0
    assert int(second.argmax()) == 705 and float(second.max()) > 30
    _check_invariant(rb)
    # refused with a ring: a rollout longer than it
    z = torch.zeros(1002, device=dev)
    st = _lib.lib().iqn_replay_extend_rollout(rb._h, _lib.ptr(rb.s), _lib.ptr(rb.a), _lib.ptr(z), _lib.ptr(z),
                                              _lib.ptr(z), _lib.ptr(z), 1002, 3, 0.99, None,
                                              _lib.stream_ptr(None))
    assert st == 1001 and b"capacity" in _lib.lib().iqn_last_error()


# ---------------------------------------------------------------- 5. the one call and its parts
STEP_CASES = [c for c in so.CASES if c[:3] in ((3, 8, 6), (2, 5, 15), (5, 32, 6))]


def _triples(dev, case, dtype, ring=200):
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    N, W, A, _ = case
    out = []
    for _ in range(2):
        m = DistributionalAtariDQN(OBS, A, W, device=dev, dtype=dtype, seed=0)
        flat = so.flat0(A)
        m.load_flat(flat, flat)
        e = IqnEngine(m, batch_size=N, train=True)
        m._train_engine = e
        rb = _native(dev, ring, W)
        obs, act, _, _ = dorc.synthetic_batch(ring, A, seed=21, probs=False)
        tgt = np.random.default_rng(6).standard_normal((ring, W)).astype(np.float32)
        pri = np.random.default_rng(4).uniform(0.05, 3.0, ring).astype(np.float32)
        rb.extend(tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (obs, act, tgt)), priorities=pri)
        out.append((m, e, rb))
    return out


@pytest.mark.parametrize("case", STEP_CASES, ids=str)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_step_replay_equals_its_parts(dtype, case):
    dev = _dev()
    assert len(STEP_CASES) == 3
    N, W, A, _ = case
    (m1, e1, rb1), (m2, e2, rb2) = _triples(dev, case, dtype)
    assert torch.equal(m1.flat, m2.flat)
    explicit = _t(np.random.default_rng(8).random((N, W)).astype(np.float32), dev)
    for c in range(4):
        taus = explicit if c == 3 else None
        keys1, prio1, taus1 = e1.train_step_replay(rb1, seed=99, counter=c, taus=taus, tau_seed=7,
                                                   tau_counter=100 + c)
        rb2.reset(99)
        rb2._counter = c
        keys2, (s, a, t), probs = rb2.sample(N)
        prio2, taus2 = e2.train_step(s, a, t, probs, taus=taus, seed=7, counter=100 + c)
        rb2.update(keys2, prio2)
        torch.cuda.synchronize()
        assert torch.equal(keys1, keys2) and torch.equal(prio1, prio2) and torch.equal(taus1, taus2), c
        if c == 3:
            assert torch.equal(taus1, explicit)
        assert torch.equal(m1.flat, m2.flat), c
        assert torch.equal(e1.exp_avg, e2.exp_avg) and torch.equal(e1.exp_avg_sq, e2.exp_avg_sq), c
        assert torch.equal(e1.metrics, e2.metrics), c
        assert torch.equal(rb1.priorities, rb2.priorities), c
        assert torch.equal(rb1.weights(), rb2.weights()), c
    assert float(e1.metrics[7]) == 4.0
    assert np.isfinite(m1.flat.cpu().numpy()).all()
    _check_invariant(rb1)


def test_train_step_replay_refusals():
    from impala_amd.dqn import NativePrioritizedReplay
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    dev = _dev()
    (m, e, rb), _ = _triples(dev, (3, 8, 6, True), "fp32", ring=16)
    lib = _lib.lib()
    sp = _lib.stream_ptr(None)
    step0 = float(e.metrics[7])

    def call(h, r):
        return lib.iqn_train_step_replay(h, r, 1, 0, None, 2, 0, None, None, None, sp), lib.iqn_last_error().decode()
    st, msg = call(None, rb._h)
    assert st == 1001 and "null handle" in msg
    st, msg = call(e._h, None)
    assert st == 1001 and "null replay handle" in msg
    with pytest.raises(RuntimeError, match="empty"):
        e.train_step_replay(_native(dev, 16, 8), 1, 0)
    # a learner without iqn_bind_state
    infer = IqnEngine(DistributionalAtariDQN(OBS, 6, 8, device=dev, seed=0), batch_size=3)
    st, msg = call(infer._h, rb._h)
    assert st != 0 and "iqn_bind_state" in msg
    with pytest.raises(RuntimeError, match="inference"):
        infer.train_step_replay(rb, 1, 0)
    # another width: refused by the wrapper, and by the entry point itself
    other = _native(dev, 16, 5)
    other.extend(_rows(4, 5))
    with pytest.raises(ValueError, match="target_width"):
        e.train_step_replay(other, 1, 0)
    st, msg = call(e._h, other._h)
    assert st == 1001 and "n_tau" in msg
    # a replay that was never bound
    raw = _lib._P()
    assert lib.iqn_replay_create(16, 8, 0.6, 0, C.byref(raw)) == 0
    st, msg = call(e._h, raw)
    assert st != 0 and "iqn_replay_bind" in msg
    assert lib.iqn_replay_destroy(raw) == 0
    # a scalar replay's handle never reaches the IQN entry point, nor this one the scalar step's
    with pytest.raises(TypeError):
        e.train_step_replay(NativePrioritizedReplay(16, device=dev), 1, 0)
    with pytest.raises(ValueError, match="taus"):
        e.train_step_replay(rb, 1, 0, taus=torch.zeros(3, 7))
    torch.cuda.synchronize()
    assert float(e.metrics[7]) == step0  # nothing ran


# ---------------------------------------------------------------- 6. end to end
def test_builder_actor_replay_learner():
    from impala_amd import iqn
    from impala_amd.config import load_config
    from impala_amd.dqn import PrioritizedReplay
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size = 64
    cfg.agent.rollout_length = 6
    b = iqn.ApexDistributionalBuilder(cfg)
    torch.manual_seed(0)
    model = b.make_network()
    W = model.n_tau_samples
    assert W == 8
    rb = b.make_replay(native=True)
    assert isinstance(rb, iqn.NativeQuantileReplay) and rb.target.shape == (64, 8)
    assert rb.capacity == 64 and rb.alpha == 0.6 and rb.target_width == 8
    assert type(b.make_replay()) is PrioritizedReplay
    with pytest.raises(NotImplementedError, match="in-place"):
        b.make_replay(native=True, in_place=True)
    actor_model = b._actor_model
    actor = b.make_actor(actor_model, rb)(0)
    rollouts = []
    real = rb.extend_rollout
    rb.extend_rollout = lambda *args: rollouts.append(args) or real(*args)
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, size=(19, 3, 64, 64), dtype=np.uint8)
    rew = rng.standard_normal(19).astype(np.float32)
    done = rng.random(19) < 0.15
    ts = (torch.from_numpy(frames[0]), 0.0, False, None)
    actor.observe_init(ts)
    for i in range(18):
        action = actor.act(ts)
        ts = (torch.from_numpy(frames[i + 1]), float(rew[i]), bool(done[i]), None)
        actor.observe(action, ts)
    assert len(rb) == 15 and len(rollouts) == 3
    # the same recorded rollouts through today's path into the torch replay
    plain = PrioritizedReplay(64, priority_exponent=0.6, device=dev, seed=0, target_width=W)
    for s, a, r, d, q_pi, q_star, n_step, gamma in rollouts:
        assert s.shape == (6, 3, 64, 64) and q_star.shape == (6, W)
        tg, prio = iqn.iqn_nstep_targets(r, d, q_pi, q_star.to(dev), n_step, gamma)
        plain.extend((s[:-1], a[:-1].to(torch.int64), tg), prio)
    for name in ("s", "a", "target", "priorities"):
        assert torch.equal(getattr(rb, name), getattr(plain, name)), name
    assert float(rb.max_priority()) == float(plain._max_priority)
    _check_invariant(rb)

    kw = b.learner_kwargs()
    kw["learning_starts"] = 15
    learner = iqn.DistributionalApexLearner(model, rb, batch_size=5, **kw)
    learner.prepare()
    calls0 = iqn.REPLAY_STEP_CALLS
    expected = {"train_step/" + k for k in ("q", "target", "priorities", "loss", "grad_norm")} | {
        "debug/priority_update_time", "debug/replay_sample_per_second", "debug/gradient_per_second",
        "debug/forward_dt", "debug/target_sync_time", "debug/update_time", "debug/total_time"}
    for i in range(3):
        met = learner.train_step()
        assert set(met) == expected
        assert float(learner.engine.metrics[7]) == i + 1  # the step metric advances
        assert all(np.isfinite(float(met["train_step/" + k])) for k in ("q", "loss", "grad_norm"))
        keys, prio, taus = learner.last_keys, learner.last_priorities, learner.last_taus
        assert keys.shape == (5,) and prio.shape == (5,) and taus.shape == (5, W)
        assert int(keys.min()) >= 0 and int(keys.max()) < 15
        ring_p, k_np, p_np = rb.priorities.cpu().numpy(), keys.cpu().numpy(), prio.cpu().numpy()
        for key in np.unique(k_np):
            assert ring_p[key] in p_np[k_np == key], (i, key)
    assert iqn.REPLAY_STEP_CALLS == calls0 + 3
    _check_invariant(rb)
    # the torch replay still takes the three-part path: the new entry is not called
    model2 = iqn.DistributionalAtariDQN(OBS, 15, W, device=dev, seed=0)
    learner2 = iqn.DistributionalApexLearner(model2, plain, batch_size=5, **kw)
    before = plain.priorities.clone()
    met = learner2.train_step()
    assert set(met) == expected and iqn.REPLAY_STEP_CALLS == calls0 + 3
    assert not torch.equal(plain.priorities, before)
