"""PPO on the device: the lambda-return ingest (impala_ppo_extend_rollout) against the fp32
restatement bit for bit, the step on ring rows read in place (impala_ppo_train_step_rows)
against the step on the gathered rows bit for bit, and PPOBuilder's actor / device replay /
learner against the same learner over a host replay.  Nothing here has a tolerance: the kernels
and the draws are the same on both sides of every comparison, only the data path differs."""
import itertools

import numpy as np
import pytest
import torch

import ppo_rollout_oracle as orc
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DONES = ("none", "all", "first", "last")
LAMBDAS = (0.0, 0.95, 1.0)
SENT_ACT, SENT_TGT, SENT_MU, SENT_OBS = -7, -123.25, -77.5, 0xAB


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


_ROLLOUTS = {}


def _rollout(L, A, done):
    """One scripted rollout and its expected targets per lambda (computed once, shared)."""
    key = (L, A, done)
    if key not in _ROLLOUTS:
        rng = np.random.default_rng(1000 * L + 10 * A + DONES.index(done))
        d = np.zeros(L, dtype=bool)
        if done == "all":
            d[:] = True
        elif done == "first":
            d[0] = True
        elif done == "last":
            d[L - 2] = True  # the last step the targets read (done[L-1] is never used)
        ro = dict(obs=rng.integers(0, 256, (L, 3, 64, 64), dtype=np.uint8),
                  act=rng.integers(0, A, L).astype(np.int64),
                  rew=rng.standard_normal(L).astype(np.float32), done=d,
                  mu=rng.standard_normal((L, A)).astype(np.float32),
                  v=(3 * rng.standard_normal(L)).astype(np.float32))
        ro["tgt"] = {lam: orc.lambda_returns_f32(ro["rew"], d, ro["v"], 0.99, lam) for lam in LAMBDAS}
        _ROLLOUTS[key] = ro
    return _ROLLOUTS[key]


def _sentinel_ring(dev, C, A):
    from impala_amd.replay import DeviceTransitionBuffer
    rb = DeviceTransitionBuffer(C, A, device=dev, seed=0)
    rb.obs.fill_(SENT_OBS)
    rb.act.fill_(SENT_ACT)
    rb.tgt.fill_(SENT_TGT)
    rb.mu.fill_(SENT_MU)
    return rb


def _check_ingest(rb, ro, lam, cursor, on_device):
    """Ingest `ro` at `cursor` into the sentinel ring; every array must equal the expected one
    byte for byte: the K rows written, every other row still the sentinel."""
    dev, C, A = rb.device, rb.capacity, rb.A
    L = ro["rew"].size
    K = L - 1
    rb._cursor = cursor
    size0 = len(rb)
    ins = [torch.from_numpy(ro[k]) for k in ("obs", "act", "rew", "done", "mu", "v")]
    if on_device:
        ins = [t.to(dev) for t in ins]
    else:  # as an actor stacks them: trailing unit dims
        ins = [ins[0], ins[1].reshape(L, 1), ins[2].reshape(L, 1), ins[3].reshape(L, 1), ins[4],
               ins[5].reshape(L, 1)]
    keys = rb.extend_rollout(*ins, gamma=0.99, lambda_=lam)
    slots = (cursor + np.arange(K)) % C
    assert len(keys) == K and rb._cursor == (cursor + K) % C and len(rb) == min(C, size0 + K)
    exp_obs = np.full((C, 3, 64, 64), SENT_OBS, np.uint8)
    exp_act = np.full(C, SENT_ACT, np.int64)
    exp_tgt = np.full(C, SENT_TGT, np.float32)
    exp_mu = np.full((C, A), SENT_MU, np.float32)
    exp_obs[slots], exp_act[slots] = ro["obs"][:K], ro["act"][:K]
    exp_tgt[slots], exp_mu[slots] = ro["tgt"][lam], ro["mu"][:K]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rb.tgt), _bits(exp_tgt)), "targets"
    assert np.array_equal(rb.act.cpu().numpy(), exp_act), "actions"
    assert np.array_equal(_bits(rb.mu), _bits(exp_mu)), "logits"
    assert np.array_equal(rb.obs.cpu().numpy(), exp_obs), "obs"
    # back to the sentinel for the next case
    rb.obs[slots] = SENT_OBS
    rb.act[slots] = SENT_ACT
    rb.tgt[slots] = SENT_TGT
    rb.mu[slots] = SENT_MU


# inside: the K rows in the middle of a larger ring; wrap: they cross the ring's end (two obs
# copies); full: K == capacity, from a cursor in the middle (every row written, wrapping)
@pytest.mark.parametrize("layout", ["inside", "wrap", "full"])
@pytest.mark.parametrize("L", [2, 3, 65, 129])
def test_ingest_is_bitwise_the_restatement(L, layout):
    dev = _dev()
    K = L - 1
    for A in (1, 6, 15):
        C = K if layout == "full" else K + 3
        cursor = {"inside": 1, "wrap": C - 1, "full": K // 2}[layout]
        rb = _sentinel_ring(dev, C, A)
        for i, (done, lam) in enumerate(itertools.product(DONES, LAMBDAS)):
            _check_ingest(rb, _rollout(L, A, done), lam, cursor, on_device=i % 2 == 1)


def test_ingest_at_the_longest_rollout():
    """L = 1025: K = 1024 steps, all the kernel stages in LDS, four rows per thread."""
    dev = _dev()
    rb = _sentinel_ring(dev, 1030, 15)
    _check_ingest(rb, _rollout(1025, 15, "last"), 0.95, 1027, on_device=True)


def test_ingest_refuses_what_the_ring_cannot_take():
    dev = _dev()
    rb = _sentinel_ring(dev, 4, 6)
    ro = _rollout(65, 6, "none")
    ins = [torch.from_numpy(ro[k]) for k in ("obs", "act", "rew", "done", "mu", "v")]
    with pytest.raises(RuntimeError, match="capacity"):
        rb.extend_rollout(*ins)
    with pytest.raises(RuntimeError, match="lambda"):
        rb.extend_rollout(*[t[:3] for t in ins], lambda_=1.5)
    torch.cuda.synchronize()
    assert len(rb) == 0 and rb._cursor == 0 and bool((rb.act == SENT_ACT).all())


# ---------------------------------------------------------------- the step on ring rows
def _engine(dev, N, dtype, A=15):
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    m = AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
    e = Engine(m, batch_size=N, algo="ppo", dtype=dtype)
    m._train_engine = e
    return m, e


def _state(m, e):
    return (m.flat, e.exp_avg, e.exp_avg_sq, m.flat_grad, e.metrics)


def _same_state(a, b):
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "post-clip grad", "metrics"), a, b):
        assert torch.equal(x, y), name


def _rows_step(e, ring, rows):
    from impala_amd import _lib
    try:
        e.ppo_train_step_rows(ring, rows)
    except _lib.Unsupported as ex:  # a fallback here would hide a failure
        pytest.fail(f"impala_ppo_train_step_rows refused the default handle: {ex}")


# N = 1: one row; 65: a second head workgroup holding a single row; 256: the full row map
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [1, 65, 256])
def test_step_on_ring_rows_is_bitwise_the_gathered_step(N, dtype):
    dev = _dev()
    from impala_amd.engine import gather_rollouts
    C = N + 7  # a ring larger than the batch
    ring = tuple(torch.from_numpy(x).to(dev) for x in ref_cpu.synthetic_ppo_batch(C, 15, seed=40 + N))
    rng = np.random.default_rng(N)
    row_sets = [rng.permutation(C)[:N].astype(np.int64) for _ in range(2)]  # permuted maps
    if N > 1:
        row_sets[1][N // 2] = row_sets[1][0]  # a slot twice in one batch
    m1, e1 = _engine(dev, N, dtype)
    m2, e2 = _engine(dev, N, dtype)
    rb2 = e2.ppo_ring_batch(ring)
    for rows in row_sets:
        e1.train_step(*gather_rollouts(ring, rows))
        _rows_step(e2, rb2, rows)
    torch.cuda.synchronize()
    _same_state(_state(m1, e1), _state(m2, e2))
    assert float(e2.metrics[7]) == 2.0  # both steps ran


def test_row_step_argument_checks_on_a_live_handle():
    dev = _dev()
    from impala_amd import _lib
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    N, C = 8, 12
    ring = tuple(torch.from_numpy(x).to(dev) for x in ref_cpu.synthetic_ppo_batch(C, 15, seed=3))
    m, e = _engine(dev, N, "fp32")
    before = m.flat.clone()
    rows = np.arange(N, dtype=np.int64)
    bad = rows.copy()
    bad[2] = C
    with pytest.raises(RuntimeError, match="out of range"):
        e.ppo_train_step_rows(ring, bad)
    with pytest.raises(RuntimeError, match="n must equal batch_size"):
        e.ppo_train_step_rows(ring, rows[:5])
    # the IMPALA entry still refuses a PPO handle, and the PPO entry an IMPALA handle
    b4, cap = e.ppo_ring_batch(ring)
    b5 = _lib.ImpalaBatch(b4.obs, b4.actions, b4.targets, b4.targets, b4.behaviour_logits)
    with pytest.raises(_lib.Unsupported):
        e._train_step_rows(b5, cap, rows, None)
    mi = AtariPPOModel((3, 64, 64), 15, device=dev, seed=0)
    ei = Engine(mi, batch_size=N, rollout_length=2)
    with pytest.raises(_lib.Unsupported):
        ei.ppo_train_step_rows((b4, cap), rows)
    torch.cuda.synchronize()
    assert torch.equal(m.flat, before)


def test_overwrite_after_the_draw_is_read_by_the_step():
    """sample_rows, then an ingest over two of the drawn slots, then the step: the draw is of
    slots and the stream orders the work, so the step reads the new rows."""
    dev = _dev()
    from impala_amd.engine import gather_rollouts
    from impala_amd.replay import DeviceTransitionBuffer
    N, C, A = 16, 24, 15
    rb = DeviceTransitionBuffer(C, A, device=dev, seed=5)
    rb.extend(tuple(torch.from_numpy(x) for x in ref_cpu.synthetic_ppo_batch(C, A, seed=77)))
    assert len(rb) == C and rb._cursor == 0
    _, rs, _ = rb.sample_rows(N)
    drawn = set(int(i) for i in rs.idx)
    c = next(i for i in range(C) if i in drawn and (i + 1) % C in drawn)
    old = [f[[c, (c + 1) % C]].clone() for f in rb.fields]
    rb._cursor = c
    ro = _rollout(3, A, "none")
    m2, e2 = _engine(dev, N, "fp32")
    rb.extend_rollout(*[torch.from_numpy(ro[k]) for k in ("obs", "act", "rew", "done", "mu", "v")])
    _rows_step(e2, rb.fields, rs.idx)  # (enqueued right behind the ingest, no host wait between)
    torch.cuda.synchronize()
    new = [f[[c, (c + 1) % C]] for f in rb.fields]
    assert not torch.equal(old[0], new[0]) and not torch.equal(old[2], new[2])
    assert np.array_equal(_bits(new[2]), _bits(ro["tgt"][0.95]))
    m1, e1 = _engine(dev, N, "fp32")
    e1.train_step(*gather_rollouts(rb.fields, rs.idx))  # the ring's current contents
    torch.cuda.synchronize()
    _same_state(_state(m1, e1), _state(m2, e2))


# ---------------------------------------------------------------- builder, actor, learner
def _timesteps(n, seed):
    rng = np.random.default_rng(seed)
    return [(torch.from_numpy(rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)),
             float(rng.standard_normal()), bool(rng.random() < 0.15)) for _ in range(n)]


def _metric_bits(out):
    return {k: _bits(v.reshape(1))[0] for k, v in out.items() if not k.startswith("debug/")}


def _host_twin(dev, flat0, items, seed, batch, rows=None):
    """A PPOLearner from the parameters `flat0` over a host ReplayBuffer holding `items`."""
    from impala_amd.learner import ImpalaAdam
    from impala_amd.model import AtariPPOModel
    from impala_amd.ppo import PPOLearner
    from impala_amd.replay import ReplayBuffer
    m = AtariPPOModel((3, 64, 64), 15, device=dev, dtype="fp32", seed=0)
    m.load_flat(flat0)
    rb = ReplayBuffer(rows or len(items), seed=seed)
    rb.extend(items)
    ln = PPOLearner(m, rb, ImpalaAdam(lr=1e-4, eps=1e-5), batch_size=batch, learning_starts=len(items))
    ln.prepare()
    return m, ln


def test_builder_actor_device_replay_learner_equal_the_host_replay_learner():
    dev = _dev()
    from impala_amd import _lib
    from impala_amd.builder import PPOBuilder
    from impala_amd.config import load_config
    from impala_amd.learner import ImpalaAdam
    from impala_amd.ppo import PPOActor, PPOLearner
    from impala_amd.replay import DeviceTransitionBuffer
    L, R, B, cap, seed = 9, 3, 16, 64, 11
    cfg = load_config(agent="ppo")
    cfg.distributed.train_device = cfg.distributed.infer_device = "cuda:0"
    cfg.agent.replay_buffer_size = cap
    cfg.training.seed = seed
    cfg.learner = {"replay": "device"}
    b = PPOBuilder(cfg)
    model = b.make_network()
    flat0 = model.flat.cpu().numpy().copy()
    rb = b.make_replay()
    assert isinstance(rb, DeviceTransitionBuffer) and rb.capacity == cap and rb.A == 15
    actor = b.make_actor(b.actor_model, rb)(0)
    assert isinstance(actor, PPOActor)
    steps = _timesteps(R * L + 1, seed=21)
    actor.observe_init(steps[0])
    items = []
    for k in range(R):
        rec = []
        for i in range(k * L, (k + 1) * L):
            action = actor.act(steps[i])
            rec.append((steps[i][0], action[0].reshape(1), steps[i + 1][1], steps[i + 1][2],
                        action[1]["logpi"].reshape(1, -1), float(action[1]["v"])))
            actor.observe(action, steps[i + 1])
        actor.update()  # L steps -> L - 1 transitions
        tgt = orc.lambda_returns_f32([r[2] for r in rec], [r[3] for r in rec], [r[5] for r in rec],
                                     0.99, 0.95)
        items += [[rec[t][0][None], rec[t][1], torch.from_numpy(tgt[t:t + 1]), rec[t][4]]
                  for t in range(L - 1)]
    assert len(rb) == R * (L - 1) == 24
    ln = PPOLearner(model, rb, ImpalaAdam(lr=1e-4, eps=1e-5), batch_size=B, learning_starts=24)
    ln.prepare()
    m2, ln2 = _host_twin(dev, flat0, items, seed, B, rows=cap)
    calls = []
    orig = ln.engine.ppo_train_step_rows
    ln.engine.ppo_train_step_rows = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    for step in range(3):
        a, h = ln.train_step(), ln2.train_step()
        torch.cuda.synchronize()
        assert set(a) == set(h)
        assert _metric_bits(a) == _metric_bits(h), step
    assert len(calls) == 3 and ln._rows  # every step read the ring in place
    assert torch.equal(model.flat, m2.flat)
    assert _lib.MAX_ROWS == 256


def test_a_refused_handle_gathers_and_equals_the_host_replay_learner(monkeypatch):
    """A handle on the separate per-frame backward kernels (IMPALA_LC12=0), which do not read
    the batch through the row map: the in-place entry refuses it before anything is enqueued,
    and the learner gathers from then on with the host-replay learner's result."""
    dev = _dev()
    from impala_amd.learner import ImpalaAdam
    from impala_amd.model import AtariPPOModel
    from impala_amd.ppo import PPOLearner
    from impala_amd.replay import DeviceTransitionBuffer
    monkeypatch.setenv("IMPALA_LC12", "0")
    B, C, seed = 16, 40, 4
    obs, act, tgt, mu = (torch.from_numpy(x) for x in ref_cpu.synthetic_ppo_batch(C, 15, seed=19))
    items = [[obs[i:i + 1], act[i:i + 1], tgt[i:i + 1], mu[i:i + 1]] for i in range(C)]
    model = AtariPPOModel((3, 64, 64), 15, device=dev, dtype="fp32", seed=0)
    flat0 = model.flat.cpu().numpy().copy()
    rb = DeviceTransitionBuffer(C, 15, device=dev, seed=seed)
    for it in items:
        rb.append(it)
    ln = PPOLearner(model, rb, ImpalaAdam(lr=1e-4, eps=1e-5), batch_size=B, learning_starts=C)
    ln.prepare()
    m2, ln2 = _host_twin(dev, flat0, items, seed, B)
    for step in range(2):
        a, h = ln.train_step(), ln2.train_step()
        torch.cuda.synchronize()
        assert _metric_bits(a) == _metric_bits(h), step
        assert ln._rows is False
    assert torch.equal(model.flat, m2.flat)


def test_a_batch_over_256_gathers_and_equals_the_host_replay_learner():
    dev = _dev()
    from impala_amd.learner import ImpalaAdam
    from impala_amd.model import AtariPPOModel
    from impala_amd.ppo import PPOLearner
    from impala_amd.replay import DeviceTransitionBuffer
    B, C, seed = 300, 320, 2
    obs, act, tgt, mu = (torch.from_numpy(x) for x in ref_cpu.synthetic_ppo_batch(C, 15, seed=9))
    items = [[obs[i:i + 1], act[i:i + 1], tgt[i:i + 1], mu[i:i + 1]] for i in range(C)]
    model = AtariPPOModel((3, 64, 64), 15, device=dev, dtype="fp32", seed=0)
    flat0 = model.flat.cpu().numpy().copy()
    rb = DeviceTransitionBuffer(C, 15, device=dev, seed=seed)
    rb.extend(items[:200])  # items, then a collated tuple
    rb.extend((obs[200:], act[200:], tgt[200:], mu[200:]))
    ln = PPOLearner(model, rb, ImpalaAdam(lr=1e-4, eps=1e-5), batch_size=B, learning_starts=C)
    ln.prepare()
    ln.engine.ppo_train_step_rows = None  # the in-place entry must not be reached
    m2, ln2 = _host_twin(dev, flat0, items, seed, B)
    a, h = ln.train_step(), ln2.train_step()
    torch.cuda.synchronize()
    assert _metric_bits(a) == _metric_bits(h)
    assert torch.equal(model.flat, m2.flat)
