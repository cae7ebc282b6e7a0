"""Every launch of the SAC learner step against a float64 reference of that launch alone,
evaluated on the step's own exported tensors (SACEngine.debug_tensor / sac_debug_read;
oracle/sac_stages.py; cases, bounds and the checks themselves in tests/stage_checks.py, SAC
section; the same checks run on a float32 stand-in in tests/test_sac_stages_host.py).

Per case (N, D, K) and dtype:
 (a) one step on the per-layer path (SAC_FUSED=0): every exported tensor to its stage reference;
     transposed copies equal their row-major tensors bit for bit, ones rows are 1, padding is 0,
     pack and the kernel-layout weights are RNE of their fp32 sources; each of the 12 + 8 gradient
     blocks; the clip; Adam, Polyak and log_alpha given the device's own clipped gradient; the
     metrics.
 (b) where Cp <= 256 the same step on the default (fused) path: every buffer both paths write,
     and the whole bound state, bit for bit -- which carries (a) over to the chain kernels, the wide
     first-layer branch included.  Cp = 288: the default handle must itself run the per-layer path
     (phase timer), with the same bits.
 (c) a second step on the default path (stale workspace in place, Adam step counters at 2): the
     final state teacher-forced at the Adam stage.

Bounds (tests/stage_checks.py): fp32 tensors F32_NORMWISE; bf16 tensors the element bound and a
share != RNE of at most CAP; gradient blocks BLOCK_RL2 after scaling the reference by its own clip
coefficient; grad-norm metrics GRAD_NORM_RTOL; other metrics MET_RTOL; parameters and targets
2e-6, log_alpha 1e-6 absolute after Adam.  An actor-loss row whose reference |q1 - q2| is within
1e-5 (|q1| + |q2|) is undecided: either assignment is accepted, at most one such row per case.
Measured figures: profiles/sac_stages/new_tests.txt.
"""
import os

import numpy as np
import pytest
import torch

import stage_checks as sc
from oracle import sac_stages as sst

pytestmark = pytest.mark.gpu
DTYPES = ("fp32", "bf16")
# what the fused path writes to HBM too (it keeps the other tiles in LDS)
FUSED_WRITES = ("xs", "xs1", "xc", "xt", "xp", "xst", "xct", "hc1_0", "hc1_1", "hc2_0", "hc2_1",
                "hc1t_0", "hc1t_1", "hc2t_0", "hc2t_1", "ha1", "ha2", "ha1t", "ha2t", "q1", "q2",
                "logp1", "logp", "logp2", "save", "rowm", "dh2t_0", "dh2t_1", "dqt_0", "dqt_1",
                "dhc1t_0", "dhc1t_1", "dha2t", "dha1t", "gmt", "gut", "sq_c", "sq_a")
STATE = ("actor", "critic", "tactor", "tcritic", "actor_grad", "critic_grad", "actor_m", "actor_v",
         "critic_m", "critic_v", "la_buf", "metrics", "prio")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Run:
    """One engine on a case's parameters (per-layer or default path)."""

    def __init__(self, dev, case, dtype, inputs=None, env=(), N=None, **kw):
        from impala_amd.sac import SACEngine, SoftActor, SoftCritic
        n, D, K = case
        i = inputs or sc.sac_inputs(case)
        self.dev, self.case = dev, case
        self.critic = SoftCritic((D,), (K,), device=dev, init=False)
        self.actor = SoftActor((D,), (K,), device=dev, dtype=dtype, init=False)
        self.tactor = self.actor.clone_to(dev)
        with torch.no_grad():
            self.actor.flat.copy_(torch.from_numpy(i["actor0"]))
            self.tactor.flat.copy_(torch.from_numpy(i.get("tactor0", i["actor0"])))
            self.critic.flat.copy_(torch.from_numpy(i["critic0"]))
            self.critic.target_flat.copy_(torch.from_numpy(i.get("tcritic0", i["critic0"])))
            self.critic.la_buf[0] = sc.SAC_LA0
        for k, v in env:
            os.environ[k] = v
        try:
            self.eng = SACEngine(self.actor, self.critic, self.tactor, batch_size=N or n, dtype=dtype,
                                 **(kw or sc.sac_kw(case, dtype)))
        finally:
            for k, _ in env:
                os.environ.pop(k, None)
        self.actor._train_engine = self.eng
        self.critic._engine = self.eng
        self.prio = torch.zeros(N or n, dtype=torch.float32, device=dev)

    def tensors(self, i):
        """A batch as device tensors the step reads in place (kept by the caller)."""
        s, a, r, s1, d = i["batch"]
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(self.dev) for x in (s, a, r, s1)]
        t.append(torch.from_numpy(np.ascontiguousarray(d)).to(self.dev).to(torch.uint8))
        t.append(None if i["probs"] is None else torch.from_numpy(i["probs"]).to(self.dev))
        t.append(torch.from_numpy(i["eps"]).to(self.dev))
        return t

    def step(self, t):
        s, a, r, s1, d, p, eps = t
        self.eng.train_step(s, a, r, s1, d, probabilities=p, noise=eps, priorities=self.prio)
        torch.cuda.synchronize()

    def state(self):
        e = self.eng
        v = dict(actor=self.actor.flat, critic=self.critic.flat, tactor=self.tactor.flat,
                 tcritic=self.critic.target_flat, actor_grad=self.actor.flat_grad,
                 critic_grad=self.critic.flat_grad, actor_m=e.actor_m, actor_v=e.actor_v,
                 critic_m=e.critic_m, critic_v=e.critic_v, la_buf=self.critic.la_buf,
                 metrics=e.metrics, prio=self.prio)
        return {k: x.detach().cpu().numpy().copy() for k, x in v.items()}

    def raw(self, names):
        return {k: self.eng.debug_tensor(k) for k in names}

    def close(self):
        self.eng.close()


def _same(a, b, names, what):
    return [f"{what} {k}: {int(np.sum(a[k] != b[k]))} elements differ" for k in names
            if not np.array_equal(a[k], b[k])]


def _hold_second_step(before, after, logp2, case, dtype, label):
    """(c): the state after a second step given the state before it and the device's own clipped
    gradients of that step -> violations."""
    kw = sc.sac_kw(case, dtype)
    f = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
    bad = []
    for net, lr in (("critic", 3e-3), ("actor", 3e-4)):
        p, m, v = sst.adam(f(before[net]), f(after[net + "_grad"]), f(before[net + "_m"]),
                           f(before[net + "_v"]), 2, lr)
        tgt = sst.polyak(p, f(before["t" + net]), 0.005)
        figs = []
        for k, want, tol in ((net, p, sc.SAC_PARAM_ATOL), ("t" + net, tgt, sc.SAC_PARAM_ATOL)):
            d = float(np.max(np.abs(after[k].astype(np.float64) - want.numpy())))
            figs.append(f"{k} {d:.1e}")
            if not d <= tol:
                bad.append(f"step 2 {k} after Adam: max |d| {d:.2e}")
        for k, want in ((net + "_m", m), (net + "_v", v)):
            w = sc.rs.f32_figures(after[k], want.numpy())
            figs.append(f"{k} {w:.1e}")
            if not w <= sc.F32_NORMWISE:
                bad.append(f"step 2 {k}: normwise {w:.2e}")
        print(f"{label} step 2 {net} Adam (given the clipped gradient) max |d|: " + ", ".join(figs))
    la0, la1 = before["la_buf"].astype(np.float64), after["la_buf"].astype(np.float64)
    if kw["tune_alpha"]:
        _, g, la, m, v = sst.alpha_step(f(logp2), f(la0[0]), f(la0[2]), f(la0[3]), 2, -float(case[2]), 3e-3)
        d = abs(la1[0] - float(la))
        print(f"{label} step 2 log_alpha |d| {d:.1e}")
        if not d <= sc.SAC_LA_ATOL:
            bad.append(f"step 2 log_alpha: |d| {d:.2e}")
        for j, want in ((1, g), (2, m), (3, v)):
            if not abs(la1[j] - float(want)) <= sc.MET_RTOL * abs(float(want)):
                bad.append(f"step 2 log_alpha state {j}: {la1[j]} against {float(want)}")
    elif not np.array_equal(la0, la1):
        bad.append("step 2: log_alpha moved with tune_alpha off")
    if int(after["metrics"][11]) != 2:
        bad.append(f"step counter {after['metrics'][11]} after two steps")
    return bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sc.SAC_CASES, ids=lambda c: "N%d-D%d-K%d" % c)
def test_sac_step_stages(case, dtype):
    dev = _dev()
    label = "N%d D%d K%d %s" % (case + (dtype,))
    d = sc.sac_dims(case)
    names = [k for k in _Run_names() if k != "wmax"]
    # (a) the per-layer path
    per = _Run(dev, case, dtype, env=(("SAC_FUSED", "0"),))
    t0 = per.tensors(sc.sac_inputs(case))
    per.step(t0)
    raw, state = per.raw(names), per.state()
    per.close()
    bad, fig, ref = sc.hold_sac_step(raw, state, case, dtype, label)
    bad = [f"{s}: {m}" for s, m in bad]
    # (b) the default path: the same bits
    run = _Run(dev, case, dtype)
    t0 = run.tensors(sc.sac_inputs(case))
    if d["Cp"] > 256:  # the handle must have chosen the per-layer path by itself
        phases = run.eng.phase_names()
        run.eng.timer_start(phases.index("fwd_l1"), 1)
        run.step(t0)
        _, launches = run.eng.timer_read()
        print(f"{label} Cp = {d['Cp']}: fwd_l1 launches in the default handle's step: {launches}")
        if launches != 1:
            bad.append("the default handle did not run the per-layer path at Cp > 256")
        common = names
    else:
        run.step(t0)
        common = [k for k in names if k in FUSED_WRITES or k.startswith("k")]
        if not sc.sac_kw(case, dtype)["tune_alpha"]:
            common = [k for k in common if k != "logp2"]
    raw_f, state_f = run.raw(common), run.state()
    same = _same(raw, raw_f, common, "default path against per-layer,") + \
        _same(state, state_f, STATE, "default path against per-layer, state")
    print(f"{label} default path against per-layer: {len(common)} buffers and {len(STATE)} state "
          f"tensors compared bit for bit, {len(same)} differ")
    bad += same
    # (c) a second step on the default path
    t1 = run.tensors(sc.sac_inputs(case, step=1))
    run.step(t1)
    after = run.state()
    logp2 = run.eng.debug_tensor("logp2")[0, :case[0]]
    run.close()
    bad += _hold_second_step(state_f, after, logp2, case, dtype, label)
    assert not bad, bad


_NAMES = []


def _Run_names():
    if not _NAMES:
        from impala_amd.sac import SACEngine
        _NAMES.extend(SACEngine.debug_names())
    return _NAMES


def test_sac_policy_where_one_minus_y2_is_small():
    """sac_policy at n = 5 with fc_mean's bias raised (some |x| > 9, some y exactly +-1): y against
    tanh of the device's own x, logp against the formula in float64 on the device's own float32
    mean, std and y, within the bound hold_sac_policy derives from the roundings of
    1 - y y + 1e-6 (stage_checks.py); everything finite.  Both paths, both dtypes."""
    dev = _dev()
    n, D, K = sc.SAC_POLICY_CASE
    a0, obs, eps = sc.sac_policy_inputs()
    base = sc.sac_inputs((37, D, K))
    bad = []
    for dtype in DTYPES:
        for env in ((), (("SAC_FUSED", "0"),)):
            run = _Run(dev, (37, D, K), dtype, inputs=dict(base, actor0=a0), env=env)
            mean, ls, act, logp, std = (x.cpu().numpy() for x in run.eng.policy(
                torch.from_numpy(obs).to(dev), torch.from_numpy(eps).to(dev)))
            run.close()
            label = f"policy {dtype} {'per-layer' if env else 'fused'}"
            bad += [f"{label}: {m}" for m in sc.hold_sac_policy(mean, std, act, logp, eps, label)]
            if not np.array_equal(std, np.exp(ls.astype(np.float64)).astype(np.float32)) and \
                    not np.allclose(std, np.exp(ls.astype(np.float64)), rtol=4 * sc.SAC_U, atol=0):
                bad.append(f"{label}: std is not exp(log_std) within 4 ulp")
    assert not bad, bad


def test_sac_graph_cache_evicts_and_replays_bitwise():
    """Six distinct sets of batch tensors (kept alive: six sets of pointers) cycled twice through
    one engine -- the hipGraph cache holds four, so every step past the fourth evicts the least
    recently used graph and captures again -- against a SAC_GRAPH=0 engine fed the same sequence."""
    dev = _dev()
    case = (37, 11, 6)
    outs = []
    for env in ((), (("SAC_GRAPH", "0"),)):
        run = _Run(dev, case, "bf16", env=env)
        sets = [run.tensors(sc.sac_inputs(case, step=j)) for j in range(6)]
        assert len({t[0].data_ptr() for t in sets}) == 6
        for _ in range(2):
            for t in sets:
                run.step(t)
        outs.append(run.state())
        run.close()
    assert int(outs[0]["metrics"][11]) == 12
    bad = _same(outs[0], outs[1], STATE, "graph replay against direct launches,")
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
def test_sac_inference_between_steps_leaves_the_step_unchanged(dtype):
    """sac_policy, sac_q_forward and sac_act share the step's workspace: step, policy (n = 5),
    q_forward (n = 3), act (n = 1), step against step, step."""
    dev = _dev()
    case = (37, 60, 6)
    N, D, K = case
    rng = np.random.default_rng(2)
    obs = torch.from_numpy(rng.standard_normal((5, D)).astype(np.float32)).to(dev)
    act = torch.from_numpy(rng.uniform(-1, 1, (5, K)).astype(np.float32)).to(dev)
    noise = torch.from_numpy(rng.standard_normal((5, K)).astype(np.float32)).to(dev)
    outs = []
    for between in (True, False):
        run = _Run(dev, case, dtype)
        t0, t1 = run.tensors(sc.sac_inputs(case)), run.tensors(sc.sac_inputs(case, step=1))
        run.step(t0)
        if between:
            pol = run.eng.policy(obs, noise)
            q = run.eng.q_forward(obs[:3], act[:3], 0)
            a = run.eng.act(obs[:1], noise[:1], 0.3, 1.0, 0.0)
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(x).all()) for x in (*pol, *q, a))
        run.step(t1)
        outs.append(run.state())
        run.close()
    bad = _same(outs[0], outs[1], STATE, "with inference calls between the steps,")
    assert not bad, bad
