"""dqn_train_step_replay_rows on the GPU: the Ape-X step reading the sampled ring rows in place
(conv1.h ObsKeys) against dqn_train_step_replay, which gathers them first -- bit for bit -- and
the loop builder -> ApexActor -> native replay -> ApexLearner.

The shapes are the smallest at which the key map can go wrong: one transition; one full
32-transition head workgroup plus one, over a ring of 5 live rows whose other rows are poisoned
(every key drawn several times; a read outside the drawn rows shows in the parameters or as NaN);
300 transitions (past ObsRows' 256, ragged last workgroups) over 777 rows in two replay blocks.
Tolerances: none for the step (both paths run the same arithmetic on the same values); the n-step
targets as tests/test_gpu_dqn_replay.py states them (rtol 1e-6 + atol 1e-6)."""
import numpy as np
import pytest
import torch

import dqn_oracle as orc
import dqn_replay_oracle as rorc
from impala_amd import _lib

pytestmark = pytest.mark.gpu
OBS = (3, 64, 64)
ALPHA = 0.6
SEED = 99
# (N, A, capacity, rows stored)
CASES = {"n1": (1, 6, 200, 200), "n33_dups": (33, 6, 8, 5), "n300_blocks": (300, 15, 1000, 777)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _learner(dev, dtype, N, A, cap, size):
    """A model, its training engine and a native replay of `size` stored rows (as
    test_gpu_dqn_replay.py::_learner_pair builds them); the rows >= size are poisoned."""
    from impala_amd.dqn import AtariDQNModel, DqnEngine, NativePrioritizedReplay
    m = AtariDQNModel(OBS, A, device=dev, dtype=dtype, seed=0)
    e = DqnEngine(m, batch_size=N)
    m._train_engine = e
    rb = NativePrioritizedReplay(cap, priority_exponent=ALPHA, device=dev, seed=0)
    obs, act, tgt, _ = orc.synthetic_batch(size, A, seed=21, probs=False)
    pri = np.random.default_rng(4).uniform(0.05, 3.0, size).astype(np.float32)
    rb.extend(tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (obs, act, tgt)), priorities=pri)
    if size < cap:
        rb.s[size:] = 0xFF
        rb.a[size:] = 99
        rb.target[size:] = float("nan")
    torch.cuda.synchronize()
    return m, e, rb


def _check_keys(case, keys, size):
    k = keys.cpu().numpy()
    assert k.min() >= 0 and k.max() < size
    if case == "n33_dups":
        assert len(np.unique(k)) < len(k)  # a key drawn more than once
    if case == "n300_blocks":
        assert (k < _lib.DQN_REPLAY_BLOCK).any() and (k >= _lib.DQN_REPLAY_BLOCK).any()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_in_place_equals_gathered_bitwise(case, dtype):
    dev = _dev()
    N, A, cap, size = CASES[case]
    m1, e1, rb1 = _learner(dev, dtype, N, A, cap, size)
    m2, e2, rb2 = _learner(dev, dtype, N, A, cap, size)
    assert torch.equal(m1.flat, m2.flat)
    stored = tuple(x.clone() for x in (rb2.s, rb2.a, rb2.target, rb2.priorities))
    drawn = torch.zeros(cap, dtype=torch.bool, device=dev)
    for c in range(3):
        keys1, prio1 = e1.train_step_replay(rb1, SEED, c)
        keys2, prio2 = e2.train_step_replay_rows(rb2, SEED, c)
        torch.cuda.synchronize()
        _check_keys(case, keys2, size)
        assert torch.equal(keys1, keys2), c
        assert torch.equal(prio1, prio2) and bool(torch.isfinite(prio2).all()), c
        assert torch.equal(m1.flat, m2.flat), c
        assert torch.equal(e1.exp_avg, e2.exp_avg) and torch.equal(e1.exp_avg_sq, e2.exp_avg_sq), c
        assert e2.metrics.numel() == 9 and torch.equal(e1.metrics, e2.metrics), c
        assert torch.equal(rb1.priorities, rb2.priorities), c
        assert torch.equal(rb1.weights(), rb2.weights()), c
        drawn[keys2] = True
    assert float(e2.metrics[7]) == 3.0 and bool(torch.isfinite(m2.flat).all())
    # the ring is left alone: s, a, target bitwise what was stored (NaN targets compared as bits);
    # priorities changed at drawn keys only
    assert torch.equal(rb2.s, stored[0]) and torch.equal(rb2.a, stored[1])
    assert torch.equal(rb2.target.view(torch.int32), stored[2].view(torch.int32))
    assert torch.equal(rb2.priorities[~drawn], stored[3][~drawn])
    assert not torch.equal(rb2.priorities[drawn], stored[3][drawn])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_in_place_step_is_deterministic(dtype):
    dev = _dev()
    N, A, cap, size = CASES["n33_dups"]
    flats = []
    for _ in range(2):
        m, e, rb = _learner(dev, dtype, N, A, cap, size)
        for c in range(3):
            e.train_step_replay_rows(rb, SEED, c)
        torch.cuda.synchronize()
        flats.append((m.flat.clone(), rb.priorities.clone()))
    assert torch.equal(flats[0][0], flats[1][0]) and torch.equal(flats[0][1], flats[1][1])


def test_refusals_and_target_sync():
    from impala_amd.dqn import NativePrioritizedReplay
    dev = _dev()
    m, e, rb = _learner(dev, "fp32", 33, 6, 8, 5)
    empty = NativePrioritizedReplay(16, priority_exponent=ALPHA, device=dev, seed=0)
    with pytest.raises(RuntimeError, match="empty"):
        e.train_step_replay_rows(empty, 1, 0)
    # after a target sync the step reads the online weights it packed: same result as a fresh pair
    m2, e2, rb2 = _learner(dev, "fp32", 33, 6, 8, 5)
    e.sync_target()
    k1, p1 = e.train_step_replay_rows(rb, SEED, 0)
    k2, p2 = e2.train_step_replay_rows(rb2, SEED, 0)
    torch.cuda.synchronize()
    assert torch.equal(k1, k2) and torch.equal(p1, p2) and torch.equal(m.flat, m2.flat)
    assert torch.equal(m.target_flat, m2.target_flat)  # (both still the initial copy)


def test_off_the_default_path_the_learner_falls_back(monkeypatch):
    """IMPALA_LC12=0 (read when a handle is created) splits the fused per-frame backward, which
    then does not read through the key map: the entry reports unsupported before any launch and
    ApexLearner takes the gather path from then on."""
    from impala_amd import dqn
    dev = _dev()
    monkeypatch.setenv("IMPALA_LC12", "0")
    m, e, rb = _learner(dev, "fp32", 33, 6, 8, 5)
    monkeypatch.delenv("IMPALA_LC12")
    with pytest.raises(_lib.Unsupported, match="default kernel path"):
        e.train_step_replay_rows(rb, SEED, 0)
    before = m.flat.clone()
    rb.in_place = True
    m3 = dqn.AtariDQNModel(OBS, 6, device=dev, seed=0)
    monkeypatch.setenv("IMPALA_LC12", "0")
    learner = dqn.ApexLearner(m3, rb, batch_size=33, learning_starts=5)
    monkeypatch.delenv("IMPALA_LC12")
    learner.prepare()
    rows0, gath0 = dqn.REPLAY_ROWS_STEP_CALLS, dqn.REPLAY_STEP_CALLS
    for i in range(2):
        met = learner.train_step()
        assert np.isfinite(float(met["train_step/loss"])) and float(learner.engine.metrics[7]) == i + 1
    # one refused in-place call, then the gather path for good
    assert dqn.REPLAY_ROWS_STEP_CALLS == rows0 + 1 and dqn.REPLAY_STEP_CALLS == gath0 + 2
    assert rb.in_place is False and torch.equal(m.flat, before)


def test_builder_actor_replay_learner_end_to_end():
    from impala_amd import dqn
    from impala_amd.config import load_config
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size, cfg.agent.rollout_length, cfg.agent.n_step = 64, 9, 3
    b = dqn.ApexDQNBuilder(cfg)
    model = b.make_network()
    rb = b.make_replay(native=True, in_place=True)
    assert isinstance(rb, dqn.NativePrioritizedReplay) and rb.in_place
    actor = b.make_actor(b._actor_model, rb)(0)
    assert isinstance(actor, dqn.ApexActor) and float(actor._eps) == pytest.approx(0.4)
    # 18 synthetic steps: random frames, seeded rewards, two episode ends
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (19,) + OBS, dtype=torch.uint8, generator=g)
    rewards = torch.randn(18, generator=g).tolist()
    done_at = (4, 12)
    rec = []
    ts = (frames[0], 0.0, False, {})
    actor.observe_init(ts)
    for i in range(18):
        action = actor.act(ts)
        a, info = action
        assert a.shape == (1, 1) and 0 <= int(a) < 15
        ts = (frames[i + 1], rewards[i], i in done_at, {})
        actor.observe(action, ts)
        rec.append((int(a), rewards[i], i in done_at, float(info["q"]), float(info["v"])))
    torch.cuda.synchronize()
    assert rb.size == 16 and rb._cursor == 16 and actor._trajectory == []
    gamma = float(np.float32(0.99))  # the actor's default, as it crosses the C boundary
    for k in range(2):  # each rollout stands alone: 9 steps -> 8 transitions
        part = rec[9 * k:9 * k + 9]
        a, r, d, q_pi, q_star = (np.array(x) for x in zip(*part))
        r32, qp32, qs32 = (x.astype(np.float32) for x in (r, q_pi, q_star))
        rows = slice(8 * k, 8 * k + 8)
        assert torch.equal(rb.s[rows].cpu(), frames[9 * k:9 * k + 8])
        assert rb.a[rows].tolist() == a[:8].tolist()
        target = rorc.nstep_targets(r32, d, qs32, 3, gamma)
        np.testing.assert_allclose(rb.target[rows].cpu().numpy(), target, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(rb.priorities[rows].cpu().numpy(), np.abs(target - qp32[:8]),
                                   rtol=1e-6, atol=1e-6)
    # the learner over that ring, in place
    kw = b.learner_kwargs()
    kw["learning_starts"] = 16
    learner = dqn.ApexLearner(model, rb, batch_size=33, **kw)
    learner.prepare()
    rows0, gath0 = dqn.REPLAY_ROWS_STEP_CALLS, dqn.REPLAY_STEP_CALLS
    for i in range(3):
        met = learner.train_step()
        assert float(learner.engine.metrics[7]) == i + 1  # the step metric advances
        assert all(np.isfinite(float(met["train_step/" + k])) for k in ("q", "loss", "grad_norm"))
        keys, prio = learner.last_keys, learner.last_priorities
        assert keys.shape == (33,) and int(keys.min()) >= 0 and int(keys.max()) < 16
        ring_p, k_np, p_np = rb.priorities.cpu().numpy(), keys.cpu().numpy(), prio.cpu().numpy()
        for key in np.unique(k_np):
            assert ring_p[key] in p_np[k_np == key], (i, key)
    assert dqn.REPLAY_ROWS_STEP_CALLS == rows0 + 3 and dqn.REPLAY_STEP_CALLS == gath0
    assert rb.in_place is True
