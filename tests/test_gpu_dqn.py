"""Ape-X DQN learner on the shared CNN kernels with the 512-wide projection
against the reference's own outputs (tests/golden/make_dqn_golden.py) and the oracle
(tests/dqn_oracle.py).

Tolerances as the PPO parity tests (test_gpu_ppo.py): loss head on identical inputs 1e-5 rel;
fp32 train step metrics 1e-4 rel, post-clip grads 1e-3 rel-L2, post-Adam params 2e-6 abs,
priorities 1e-4 rel; forward 1e-4 rel; bf16 vs fp32 metrics 5e-2, grad cosine > 0.99.
"""
import os

import numpy as np
import pytest
import torch

import dqn_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("q", "target", "priorities", "loss", "grad_norm")
SLOT = dict(q=0, target=1, priorities=2, loss=3, grad_norm=6, step=7)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _setup(dev, N, A=15, dtype="fp32", flat=None, target=None, **kw):
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    m = AtariDQNModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
    if flat is not None:
        m.load_flat(flat, target)
    e = DqnEngine(m, batch_size=N, **kw)
    m._train_engine = e
    return m, e


def _metrics(e):
    met = e.metrics.cpu().numpy()
    return {k: met[i] for k, i in SLOT.items()}


def _step(e, batch, dev):
    obs, act, tgt, p = batch
    return e.train_step(_t(obs, dev), _t(act, dev), _t(tgt, dev), _t(p, dev)).cpu().numpy()


def test_dqn_loss_head_matches_reference():
    from impala_amd.dqn import dqn_loss_head
    dev = _dev()
    d = np.load(os.path.join(G, "dqn_head.npz"))
    out = dqn_loss_head(_t(d["adv"], dev), _t(d["v"], dev), _t(d["act"], dev), _t(d["target"], dev),
                        _t(d["prob"], dev), float(d["beta"]))
    np.testing.assert_allclose(out["metrics"].cpu().numpy(), d["scalars"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["dadv"].cpu().numpy(), d["dadv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["dv"].cpu().numpy(), d["dv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["priorities"].cpu().numpy(), d["priorities"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("N,A,probs", [(1, 15, True), (33, 2, False), (300, 6, True), (1536, 15, True)])
def test_dqn_loss_head_shapes_vs_oracle(N, A, probs):
    """More than one block of 256, a single transition, A < 15 (padded rows out of the mean), and
    N > 1024: a second pass of the batch-minimum loop over the probabilities."""
    from impala_amd.dqn import dqn_loss_head
    dev = _dev()
    rng = np.random.default_rng(N)
    adv = rng.standard_normal((N, A)).astype(np.float32)
    v = rng.standard_normal(N).astype(np.float32)
    _, act, tgt, p = orc.synthetic_batch(N, A, seed=N + 1, probs=probs)
    exp = orc.loss_from_heads(adv.astype(np.float64), v.astype(np.float64), act, tgt.astype(np.float64),
                              None if p is None else p.astype(np.float64))
    out = dqn_loss_head(_t(adv, dev), _t(v, dev), _t(act, dev), _t(tgt, dev), _t(p, dev))
    np.testing.assert_allclose(out["metrics"].cpu().numpy(), exp["metrics"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["dadv"].cpu().numpy(), exp["dadv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["dv"].cpu().numpy(), exp["dv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["priorities"].cpu().numpy(), exp["priorities"], rtol=1e-5, atol=1e-7)


def test_dqn_three_steps_match_reference():
    dev = _dev()
    d = orc.load_train_fixture()
    m, e = _setup(dev, 16, flat=d["params0"])
    for i in range(3):
        prio = _step(e, (d[f"obs{i}"], d[f"act{i}"], d[f"tgt{i}"], d[f"prob{i}"]), dev)
        met = _metrics(e)
        for k in KEYS:
            print(f"step {i} {k}: got {met[k]:.8g} ref {d[k][i]:.8g}")
            np.testing.assert_allclose(met[k], d[k][i], rtol=1e-4, atol=1e-7, err_msg=f"step {i} {k}")
        assert met["step"] == i + 1
        np.testing.assert_allclose(prio, d[f"prio{i}"], rtol=1e-4, atol=1e-6)
        if i == 0:
            g = m.flat_grad.cpu().numpy()
            print("step-1 grads rel-L2", _rel_l2(g, d["grads1"]))
            assert _rel_l2(g, d["grads1"]) < 1e-3
            err1 = np.abs(m.flat.cpu().numpy() - d["params1"]).max()
            print("params after step 1: max abs err", err1)
            assert err1 < 2e-6
    err3 = np.abs(m.flat.cpu().numpy() - d["params3"]).max()
    print("params after step 3: max abs err", err3)
    assert err3 < 2e-6


@pytest.fixture(scope="module")
def flat0():
    from impala_amd.dqn import AtariDQNModel
    return {A: AtariDQNModel((3, 64, 64), A, device="cpu", seed=0).flat.numpy().copy()
            for A in (2, 6, 15)}


@pytest.mark.parametrize("probs", [True, False], ids=["probs", "noprobs"])
@pytest.mark.parametrize("A", [2, 6, 15])
@pytest.mark.parametrize("N", [1, 33, 100])
def test_dqn_step_shapes_vs_oracle(N, A, probs, flat0):
    """N = 33: a full head block of 32 plus one row; A < 15: padded head rows."""
    dev = _dev()
    batch = orc.synthetic_batch(N, A, seed=100 * N + A, probs=probs)
    net = orc.make_net(flat0[A], A)
    exp = orc.train_step(net, orc.make_optimizer(net), *batch)
    m, e = _setup(dev, N, A=A, flat=flat0[A])
    prio = _step(e, batch, dev)
    met = _metrics(e)
    for k in KEYS:
        np.testing.assert_allclose(met[k], exp[k], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(prio, exp["prio"], rtol=1e-4, atol=1e-6)
    assert _rel_l2(m.flat_grad.cpu().numpy(), exp["grads"]) < 1e-3
    assert np.abs(m.flat.cpu().numpy() - orc.flat_params(net)).max() < 2e-6


def test_dqn_step_default_batch_vs_oracle(flat0):
    """The default batch, N = 512 (16 head blocks), with probabilities."""
    test_dqn_step_shapes_vs_oracle(512, 15, True, flat0)


def test_dqn_bf16_tracks_fp32(flat0):
    dev = _dev()
    batch = orc.synthetic_batch(64, 15, seed=5)
    res = {}
    for dt in ("fp32", "bf16"):
        m, e = _setup(dev, 64, dtype=dt, flat=flat0[15])
        _step(e, batch, dev)
        res[dt] = (_metrics(e), m.flat_grad.cpu().numpy().astype(np.float64))
    for k in KEYS:
        np.testing.assert_allclose(res["bf16"][0][k], res["fp32"][0][k], rtol=5e-2, atol=1e-3, err_msg=k)
    a, b = res["bf16"][1], res["fp32"][1]
    cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    print("bf16 vs fp32 grad cosine", cos)
    assert cos > 0.99


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dqn_step_is_deterministic(dtype, flat0):
    dev = _dev()
    batch = orc.synthetic_batch(33, 15, seed=6)
    out = []
    for _ in range(2):
        m, e = _setup(dev, 33, dtype=dtype, flat=flat0[15])
        prio = _step(e, batch, dev)
        out.append((m.flat.cpu().numpy(), m.flat_grad.cpu().numpy(), e.metrics.cpu().numpy(), prio))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def _act_fixture(dev):
    """dqn_act.npz's model (seed 0, target net nudged) and frames, regenerated from its seeds."""
    from impala_amd.dqn import AtariDQNModel, net_specs
    d = np.load(os.path.join(G, "dqn_act.npz"))
    online = orc.load_train_fixture()["params0"]  # the same seed-0 model
    rng = np.random.default_rng(int(d["target_delta_seed"]))
    delta = np.concatenate([(0.01 * rng.standard_normal(s)).astype(np.float32).reshape(-1)
                            for _, s in net_specs(15)])
    obs = rng.integers(0, 256, size=(128, 3, 64, 64), dtype=np.uint8)
    m, e = _setup(dev, 128, flat=online, target=online + delta, inference_only=True)
    return d, m, e, _t(obs, dev)


@pytest.fixture(scope="module")
def act_fix():
    return _act_fixture(_dev())


def test_dqn_forward_online_and_target(act_fix):
    d, m, e, obs = act_fix
    for which, key in ((False, "q_online"), (True, "q_target")):
        q = e.forward(obs, target=which).cpu().numpy()
        print(key, "rel-L2", _rel_l2(q, d[key]))
        np.testing.assert_allclose(q, d[key], rtol=1e-4, atol=1e-5)
    # fewer frames than the handle's batch
    np.testing.assert_allclose(e.forward(obs[:3]).cpu().numpy(), d["q_online"][:3], rtol=1e-4, atol=1e-5)


def test_dqn_sync_target_is_bitwise(act_fix):
    d, m, e, obs = act_fix
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    m2 = AtariDQNModel((3, 64, 64), 15, device=obs.device, seed=0)
    m2.load_flat(m.flat.cpu().numpy(), m.target_flat.cpu().numpy())
    e2 = DqnEngine(m2, batch_size=128, inference_only=True)
    assert not torch.equal(e2.forward(obs, target=True), e2.forward(obs))
    e2.sync_target()
    assert torch.equal(e2.forward(obs, target=True), e2.forward(obs))
    assert torch.equal(m2.target_flat, m2.flat)


def test_dqn_act_greedy_and_q(act_fix):
    d, m, e, obs = act_fix
    q_on, q_tg = e.forward(obs).cpu().numpy(), e.forward(obs, target=True).cpu().numpy()
    greedy = q_on.argmax(-1)
    assert np.array_equal(greedy, d["greedy"])
    a, q_pi, q_star, g = [x.cpu().numpy() for x in e.act(obs, 0.0, seed=1, counter=1)]
    assert np.array_equal(g, greedy) and np.array_equal(a, greedy)
    assert np.array_equal(q_pi, q_on[np.arange(128), greedy])
    assert np.array_equal(q_star, q_tg[np.arange(128), greedy])
    a, q_pi, q_star, g = [x.cpu().numpy() for x in e.act(obs, 1.0, seed=1, counter=2)]
    assert np.array_equal(g, greedy) and not np.any(a == greedy)
    assert np.array_equal(q_pi, q_on[np.arange(128), a])
    assert np.array_equal(q_star, q_tg[np.arange(128), greedy])
    # per-frame eps: even frames greedy, odd frames never greedy
    eps = torch.tensor([0.0, 1.0] * 64)
    a = e.act(obs, eps, seed=1, counter=3)[0].cpu().numpy()
    assert np.array_equal(a[0::2], greedy[0::2]) and not np.any(a[1::2] == greedy[1::2])


def test_dqn_act_draw_frequencies(act_fix):
    """eps = 0.4 over fixed (seed, counters): per frame the draw is greedy with probability 0.6,
    else uniform over the other 14 actions.  Pooled over frames by rank (greedy -> 0, the others
    in index order -> 1..14): chi-square with 14 degrees of freedom against its critical value at
    p = 1e-6."""
    from scipy.stats import chi2 as chi2_dist
    d, m, e, obs = act_fix
    greedy = d["greedy"]
    counts = np.zeros(15)
    reps = 40
    for c in range(reps):
        a = e.act(obs, 0.4, seed=1234, counter=100 + c)[0].cpu().numpy()
        rank = np.where(a == greedy, 0, np.where(a < greedy, a + 1, a))
        counts += np.bincount(rank, minlength=15)
    n = reps * 128
    exp = np.array([0.6] + [0.4 / 14] * 14) * n
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print("act draw chi2 (14 dof)", chi2, counts)
    assert chi2 < chi2_dist.isf(1e-6, 14)


def test_apex_learner_end_to_end():
    """Builder -> learner -> PrioritizedReplay, 4 steps at N = 8: each step's metrics against the
    oracle run from the learner's own pre-step parameters; the replay's priorities at the sampled
    keys are the step's |err|; target sync and push fire on their periods."""
    from impala_amd.config import load_config
    from impala_amd.dqn import ApexDQNBuilder, ApexLearner, PrioritizedReplay
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size = 64
    b = ApexDQNBuilder(cfg)
    torch.manual_seed(0)
    model = b.make_network()
    rb = b.make_replay()
    assert isinstance(rb, PrioritizedReplay)
    obs, act, tgt, _ = orc.synthetic_batch(40, 15, seed=8, probs=False)
    rb.extend((_t(obs, dev), _t(act, dev), _t(tgt, dev)),
              priorities=np.random.default_rng(1).uniform(0.1, 2.0, 40).astype(np.float32))
    kw = b.learner_kwargs()
    kw["learning_starts"] = 40  # what the ring holds: prepare() returns at once
    learner = ApexLearner(model, rb, batch_size=8, target_sync_period=2, model_push_period=3, **kw)
    learner.prepare()
    pushes = []
    model.push = lambda: pushes.append(learner._step_counter)
    for i in range(4):
        flat_before = model.flat.cpu().numpy().copy()
        target_before = model.target_flat.cpu().numpy().copy()
        sampled = {}
        real_sample = rb.sample

        def sample(n, _s=real_sample, _o=sampled):
            _o["out"] = _s(n)
            return _o["out"]
        rb.sample = sample
        met = learner.train_step()
        rb.sample = real_sample
        keys, (s, a, t), probs = sampled["out"]
        net = orc.make_net(flat_before, 15)
        opt = orc.make_optimizer(net, lr=float(cfg.agent.optimizer.lr), eps=float(cfg.agent.optimizer.eps))
        # the oracle's Adam state: step i of a fresh optimizer only at i = 0, so compare the
        # quantities that do not depend on it
        exp = orc.train_step(net, opt, s.cpu().numpy(), a.cpu().numpy(), t.cpu().numpy(), probs.cpu().numpy())
        for k in KEYS:
            np.testing.assert_allclose(float(met["train_step/" + k]), exp[k], rtol=1e-4, atol=1e-7,
                                       err_msg=f"step {i} {k}")
        # (duplicate keys in a draw hold equal transitions, so equal |err|)
        np.testing.assert_allclose(rb.priorities[keys].cpu().numpy(), exp["prio"], rtol=1e-4, atol=1e-6)
        synced = (i + 1) % 2 == 0
        if synced:
            assert torch.equal(model.target_flat, model.flat)
        else:
            assert np.array_equal(model.target_flat.cpu().numpy(), target_before)
    assert pushes == [3]
