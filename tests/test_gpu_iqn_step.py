"""The distributional (IQN) Ape-X training step on the GPU against the float64
reference tests/iqn_step_oracle.py (autograd + clip_grad_norm_ + Adam on tests/iqn_oracle.IqnNet).

The project's bounds (tests/test_gpu_dqn.py): fp32 metrics 1e-4 rel, priorities 1e-4
rel, pre-clip gradient 1e-3 rel-L2 -- on the flat vector and on every parameter tensor alone, so that
Wq's 65,536 entries do not hide behind Wfc's 524,288 -- post-Adam parameters 2e-6 abs; bf16 against
fp32 metrics 5e-2, gradient cosine > 0.99.  tests/test_iqn_step_host.py shows that a float32
evaluation of the reference keeps a quarter of each at every shape used here.  Every measured value
is printed (profiles/iqn_step/new_tests.txt).
"""
import numpy as np
import pytest
import torch

import iqn_oracle as orc
import iqn_step_oracle as so

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _setup(dev, case, dtype="fp32", flat=None):
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    N, W, A, _ = case
    m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
    flat = so.flat0(A) if flat is None else flat
    m.load_flat(flat, flat)
    e = IqnEngine(m, batch_size=N, train=True)
    m._train_engine = e
    return m, e


def _run(e, dev, b, entry="train_step"):
    obs, act, taus, tgt, prob = b
    prio, used = getattr(e, entry)(_t(obs, dev), _t(act, dev), _t(tgt, dev), _t(prob, dev), taus=_t(taus, dev))
    torch.cuda.synchronize()
    assert np.array_equal(used.cpu().numpy(), taus)  # the taus used are handed back
    return prio.cpu().numpy()


def _metrics(e):
    m = e.metrics.cpu().numpy()
    return dict(q=m[0], target=m[1], priorities=m[2], loss=m[3], grad_norm=m[6]), m


def _hold_metrics(met, ref, label, names=so.MET_NAMES):
    for k in names:
        print(f"{label} {k}: {met[k]:.9g} vs {ref[k]:.9g}  rel {abs(met[k] - ref[k]) / max(abs(ref[k]), 1e-30):.2e}")
    for k in names:
        np.testing.assert_allclose(met[k], ref[k], rtol=so.MET_RTOL, atol=so.MET_ATOL, err_msg=f"{label} {k}")


def _hold_grad(g, ref, A, label):
    worst = {"flat": so.rel_l2(g, ref)}
    for name, sl in so.tensor_slices(A).items():
        worst[name] = so.rel_l2(g[sl], ref[sl])
    print(label, "pre-clip gradient rel-L2:", "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v < so.GRAD_RL2}
    assert not bad, bad


# ---------------------------------------------------------------- one step, fp32, every shape
@pytest.mark.parametrize("case", so.CASES, ids=str)
def test_iqn_step_fp32_vs_float64(case):
    """iqn_compute_grads (metrics, priorities, the pre-clip gradient per tensor), then
    iqn_apply_update (grad_norm, the parameters), which together are iqn_train_step bit for bit
    (test_iqn_grads_then_update_is_train_step)."""
    dev = _dev()
    N, W, A, _ = case
    ref = so.reference(case)
    m, e = _setup(dev, case)
    prio = _run(e, dev, so.batch(case), "compute_grads")
    met, _ = _metrics(e)
    _hold_metrics(met, ref["met"], f"{case}", names=so.MET_NAMES[:4])
    err = np.abs(prio - ref["prio"])
    print(f"{case} priorities: max abs err {err.max():.2e}, max rel {float((err / np.abs(ref['prio'])).max()):.2e}")
    np.testing.assert_allclose(prio, ref["prio"], rtol=so.PRIO_RTOL, atol=so.PRIO_ATOL)
    g = m.flat_grad.cpu().numpy()
    assert np.isfinite(g).all()
    _hold_grad(g, ref["grad"], A, f"{case}")
    e.apply_update()
    torch.cuda.synchronize()
    met, raw = _metrics(e)
    _hold_metrics(met, ref["met"], f"{case}", names=("grad_norm",))
    assert raw[7] == 1.0  # the step counter
    err = float(np.abs(m.flat.cpu().numpy() - ref["params"]).max())
    print(f"{case} post-Adam parameters: max abs err {err:.2e}")
    assert err < so.PARAM_ABS
    # the clipped gradient torch leaves behind: g * min(1, max_norm / (norm + 1e-6))
    coef = min(1.0, so.OPT["max_grad_norm"] / (ref["met"]["grad_norm"] + 1e-6))
    assert so.rel_l2(m.flat_grad.cpu().numpy(), coef * ref["grad"]) < so.GRAD_RL2


# ---------------------------------------------------------------- three steps
def test_iqn_three_steps_and_reemitted_weights():
    """Three consecutive steps at (3, 8): metrics, priorities and parameters at every step (the Adam
    state, and the kernel-layout weights each step re-emits, Wq / bq included).  After step 3,
    iqn_forward on the updated handle equals a fresh handle bound to the same flat parameters, bit
    for bit."""
    dev = _dev()
    case = so.MULTI
    N, W, A, _ = case
    refs = so.reference_steps(case, 3)
    m, e = _setup(dev, case)
    for i in range(3):
        prio = _run(e, dev, so.batch(case, i))
        met, raw = _metrics(e)
        _hold_metrics(met, refs[i]["met"], f"step {i}")
        np.testing.assert_allclose(prio, refs[i]["prio"], rtol=so.PRIO_RTOL, atol=so.PRIO_ATOL)
        err = float(np.abs(m.flat.cpu().numpy() - refs[i]["params"]).max())
        print(f"step {i} post-Adam parameters: max abs err {err:.2e}")
        assert err < so.PARAM_ABS and raw[7] == i + 1
    obs, _, taus, _, _ = so.batch(case, 0)
    q_upd, _ = e.forward(_t(obs, dev), taus=_t(taus, dev))
    m2, e2 = _setup(dev, case, flat=m.flat.cpu().numpy())
    q_new, _ = e2.forward(_t(obs, dev), taus=_t(taus, dev))
    assert torch.equal(q_upd, q_new)
    assert not np.array_equal(m.flat.cpu().numpy(), so.flat0(A))


# ---------------------------------------------------------------- determinism, both dtypes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [so.CASES[1], so.CASES[4]], ids=str)
def test_iqn_step_is_bitwise_reproducible(case, dtype):
    dev = _dev()
    out = []
    for _ in range(2):
        m, e = _setup(dev, case, dtype)
        prio = _run(e, dev, so.batch(case))
        out.append((prio, m.flat_grad.cpu().numpy(), m.flat.cpu().numpy(), e.metrics.cpu().numpy(),
                    e.exp_avg.cpu().numpy(), e.exp_avg_sq.cpu().numpy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_iqn_grads_then_update_is_train_step(dtype):
    dev = _dev()
    case = so.CASES[1]
    m1, e1 = _setup(dev, case, dtype)
    p1 = _run(e1, dev, so.batch(case))
    m2, e2 = _setup(dev, case, dtype)
    p2 = _run(e2, dev, so.batch(case), "compute_grads")
    assert np.array_equal(m2.flat.cpu().numpy(), so.flat0(case[2]))  # no update yet
    e2.apply_update()
    torch.cuda.synchronize()
    assert np.array_equal(p1, p2)
    for a, b in ((m1.flat, m2.flat), (m1.flat_grad, m2.flat_grad), (e1.metrics, e2.metrics),
                 (e1.exp_avg, e2.exp_avg), (e1.exp_avg_sq, e2.exp_avg_sq)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- bf16 against fp32
@pytest.mark.parametrize("case", [so.CASES[1], so.CASES[4], so.CASES[5]], ids=str)
def test_iqn_step_bf16_vs_fp32(case):
    dev = _dev()
    res = {}
    for dtype in ("fp32", "bf16"):
        m, e = _setup(dev, case, dtype)
        _run(e, dev, so.batch(case))
        res[dtype] = (_metrics(e)[0], m.flat_grad.cpu().numpy().astype(np.float64))
    for k in so.MET_NAMES:
        a, b = res["bf16"][0][k], res["fp32"][0][k]
        print(f"{case} {k}: bf16 {a:.7g} fp32 {b:.7g}  rel {abs(a - b) / max(abs(b), 1e-30):.2e}")
    ga, gb = res["bf16"][1], res["fp32"][1]
    cos = float(ga @ gb / (np.linalg.norm(ga) * np.linalg.norm(gb)))
    print(f"{case} gradient cosine bf16 / fp32: {cos:.6f}")
    for k in so.MET_NAMES:
        np.testing.assert_allclose(res["bf16"][0][k], res["fp32"][0][k], rtol=so.BF16_MET_RTOL,
                                   atol=so.BF16_MET_ATOL, err_msg=k)
    assert cos > so.BF16_COS


# ---------------------------------------------------------------- library taus, refusals
def test_iqn_step_draws_its_taus_and_refuses_bad_arguments():
    from impala_amd import _lib
    dev = _dev()
    case = so.CASES[2]
    N, W, A, _ = case
    obs, act, _, tgt, prob = so.batch(case)
    m, e = _setup(dev, case)
    _, used = e.train_step(_t(obs, dev), _t(act, dev), _t(tgt, dev), _t(prob, dev), seed=5, counter=9)
    assert np.array_equal(used.cpu().numpy().reshape(-1), orc.draw_taus(5, 9, 0, N * W))
    with pytest.raises(ValueError):
        e.train_step(_t(obs, dev), _t(act, dev), _t(tgt[:, :1], dev))
    with pytest.raises(ValueError):
        e.train_step(_t(obs[:1], dev), _t(act[:1], dev), _t(tgt[:1], dev))
    with pytest.raises(RuntimeError, match="iqn_bind_state"):  # an inference handle has no training state
        from impala_amd.iqn import IqnEngine
        inf = IqnEngine(m, batch_size=N)
        b = _lib.IqnBatch(_lib.ptr(_t(obs, dev)), 0, 0, 0, 0, 0, 0, 0, 0)
        import ctypes as C
        _lib.check(_lib.lib().iqn_train_step(inf._h, C.byref(b), _lib.stream_ptr(None)), "iqn_train_step",
                   "iqn_last_error")


# ---------------------------------------------------------------- the learner, end to end
def test_distributional_learner_end_to_end():
    """make_network -> make_replay -> the actor's update with a synthetic rollout ->
    make_learner(...).train_step() twice: metrics match the reference run on the sampled batch from
    the learner's own pre-step parameters, priorities are written back at the sampled keys, and the
    target net syncs at the period."""
    from impala_amd.config import load_config
    from impala_amd.iqn import ApexDistributionalBuilder, DistributionalApexLearner
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size = 64
    W, A, L = int(cfg.agent.n_tau_samples), 15, 41
    b = ApexDistributionalBuilder(cfg)
    model = b.make_network()
    model.load_flat(so.flat0(A), so.flat0(A))
    rb = b.make_replay()
    actor = b.make_actor(model, rb)(0)
    rng = np.random.default_rng(11)
    s = torch.from_numpy(orc.fixture_obs(77, L))
    actor._trajectory = [(s[t], torch.tensor(int(rng.integers(0, A))), torch.tensor(float(rng.standard_normal())),
                          torch.tensor(bool(rng.random() < 0.1)), torch.tensor(float(rng.standard_normal())),
                          torch.from_numpy(rng.standard_normal(W).astype(np.float32))) for t in range(L)]
    actor.update()
    assert len(rb) == L - 1 and rb.target.shape == (64, W)
    assert isinstance(b.make_learner(model, rb), DistributionalApexLearner)
    kw = b.learner_kwargs()
    kw["learning_starts"] = L - 1  # what the ring holds: prepare() returns at once
    learner = DistributionalApexLearner(model, rb, batch_size=8, target_sync_period=2, **kw)
    learner.prepare()
    for i in range(2):
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
        keys, (so_, a, t), probs = sampled["out"]
        # (a fresh optimizer: its Adam state matters for the parameters alone, which the step tests hold)
        exp = so.Step(flat_before, A, opt=dict(lr=float(cfg.agent.optimizer.lr), eps=float(cfg.agent.optimizer.eps))
                      ).step(so_.cpu().numpy(), a.cpu().numpy(), learner.last_taus.cpu().numpy(), t.cpu().numpy(),
                             probs.cpu().numpy())
        for k in so.MET_NAMES:
            got = float(met["train_step/" + k])
            print(f"learner step {i} {k}: {got:.9g} vs {exp['met'][k]:.9g}")
            np.testing.assert_allclose(got, exp["met"][k], rtol=so.MET_RTOL, atol=so.MET_ATOL, err_msg=f"step {i} {k}")
        # (a key drawn twice holds one transition under two rows of taus: two priorities, and the
        # ring keeps the one written last -- so the key's priority is one of its draws')
        pr = rb.priorities[keys].cpu().numpy()
        kk = keys.cpu().numpy()
        for j in range(len(kk)):
            cand = exp["prio"][kk == kk[j]]
            assert np.any(np.abs(pr[j] - cand) <= so.PRIO_ATOL + so.PRIO_RTOL * np.abs(cand)), (j, pr[j], cand)
        if (i + 1) % 2 == 0:
            assert torch.equal(model.target_flat, model.flat)
        else:
            assert np.array_equal(model.target_flat.cpu().numpy(), target_before)
            assert not np.array_equal(model.flat.cpu().numpy(), flat_before)
