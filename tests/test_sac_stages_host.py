"""The SAC stage references (oracle/sac_stages.py) and the checks built on them
(tests/stage_checks.py, SAC section), on the CPU, at every case of tests/test_gpu_sac_stages.py:

* chained in float64 without rounding they are the autograd step of oracle/sac_cpu.py to 1e-10;
* the float32 stand-in (the same chain in torch float32, rounding where the kernels round, laid
  out as the device exports it) holds every bound of the GPU test with a quarter of each cap, and
  the reference's actor loss has no undecided row: the conditions the batch seeds were chosen by;
* a planted defect per stage family breaks its own stage's check and no earlier one.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import stage_checks as sc
from oracle import sac_cpu
from oracle import sac_stages as sst

DTYPES = ("fp32", "bf16")
_RUNS = {}


def _stand_in(case, dtype, defect=None):
    """(the stand-in's run, what it would export, the violations of hold_sac_step at a quarter)."""
    key = (case, dtype, defect)
    if key not in _RUNS:
        run_defect = None if defect == "pad_col" else defect
        s = sc.sac_reference(case, dtype, torch_dtype=torch.float32, defect=run_defect)
        raw, state = sc.sac_export(s, case, dtype, defect)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            bad, fig, ref = sc.hold_sac_step(raw, state, case, dtype, f"{case} {dtype}",
                                             cap=sc.STAND_IN_CAP)
        _RUNS[key] = (s, bad, fig, ref, out.getvalue())
    return _RUNS[key]


@pytest.mark.parametrize("case", sc.SAC_CASES)
def test_chained_references_are_the_autograd_step(case):
    """float64, nothing rounded: every gradient block, both clipped norms, the parameters, targets
    and log_alpha after the step, the priorities and the metrics against torch autograd +
    torch.optim.Adam on the same float64 inputs."""
    N, D, K = case
    i = sc.sac_inputs(case)
    kw = sc.sac_kw(case, "bf16")
    r = sc.sac_reference(case, "bf16", quant=False)  # (the options of kw, nothing rounded)
    actor, critic = sac_cpu.make_models(D, K, seed=0)
    actor, critic = actor.double(), critic.double()
    sac_cpu.load_flat(list(actor.parameters()), i["actor0"].astype(np.float64))
    sac_cpu.load_flat(list(critic.critic.parameters()), i["critic0"].astype(np.float64))
    sac_cpu.load_flat(list(critic.target_critic.parameters()), i["tcritic0"].astype(np.float64))
    with torch.no_grad():
        critic.log_alpha.fill_(float(np.float32(sc.SAC_LA0)))
    st = sac_cpu.SACState(actor, critic, max_grad_norm=kw["max_grad_norm"], tune_alpha=kw["tune_alpha"])
    sac_cpu.load_flat(list(st.target_actor.parameters()), i["tactor0"].astype(np.float64))
    s, a, rr, s1, d = i["batch"]
    tb = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) for x in (s, a, rr, s1)]
    tb.append(torch.from_numpy(np.ascontiguousarray(d)))
    probs = torch.ones(N, dtype=torch.float64) if i["probs"] is None else \
        torch.from_numpy(i["probs"].astype(np.float64))
    eps = [torch.from_numpy(i["eps"][j].astype(np.float64)) for j in range(3)]
    # the unclipped gradients of the two losses, before the step moves anything
    w = probs.pow(-0.4)
    w = w / w.max()
    loss, _, _ = sac_cpu.critic_loss(st.target_actor, st.critic, tb, w, eps[0])
    gc = torch.autograd.grad(loss, list(st.critic.critic.parameters()))
    gc = torch.cat([g.reshape(-1) for g in gc]).numpy()
    want = np.concatenate([r["cgrads"][k].reshape(-1) for k in sst.C_BLOCKS])
    assert np.max(np.abs(want - gc)) <= 1e-10 * max(1.0, np.max(np.abs(gc)))
    # sac_cpu.train_step's body with the float64 weights (train_step itself takes them to float32)
    loss, prio, met = sac_cpu.critic_loss(st.target_actor, st.critic, tb, w, eps[0])
    st.critic_opt.zero_grad(set_to_none=True)
    loss.backward()
    met["train/critic_grad_norm"] = torch.nn.utils.clip_grad_norm_(st.critic.parameters(), st.max_grad_norm)
    st.critic_opt.step()
    loss, am = sac_cpu.actor_loss(st.actor, st.critic, tb, eps[1])
    st.actor_opt.zero_grad(set_to_none=True)
    loss.backward()
    am["train/actor_grad_norm"] = torch.nn.utils.clip_grad_norm_(st.actor.parameters(), st.max_grad_norm)
    ga = torch.cat([p.grad.reshape(-1) for p in st.actor.parameters()]).numpy().copy()  # clipped
    want = np.concatenate([r["agrads"][k].reshape(-1) for k in sst.A_BLOCKS]) * r["acoef"]
    assert np.max(np.abs(want - ga)) <= 1e-10 * max(1.0, np.max(np.abs(ga)))
    st.actor_opt.step()
    met.update(am)
    if st.tune_alpha:
        loss, alm = sac_cpu.alpha_loss(st.actor, st.critic, tb, eps[2])
        st.critic_opt.zero_grad(set_to_none=True)
        loss.backward()
        st.critic_opt.step()
        met.update(alm)
    with torch.no_grad():
        for p, tp in zip(st.critic.critic.parameters(), st.critic.target_critic.parameters()):
            tp.data.copy_(st.tau * p.data + (1 - st.tau) * tp.data)
        for p, tp in zip(st.actor.parameters(), st.target_actor.parameters()):
            tp.data.copy_(st.tau * p.data + (1 - st.tau) * tp.data)
    met["prio"] = prio
    for k, got in (("critic1", st.critic.critic.parameters()), ("actor1", st.actor.parameters()),
                   ("tcritic1", st.critic.target_critic.parameters()),
                   ("tactor1", st.target_actor.parameters())):
        assert np.max(np.abs(r[k] - sac_cpu.flat(got))) <= 1e-10, k
    assert abs(r["la"]["la"] - float(st.critic.log_alpha.detach())) <= 1e-10
    np.testing.assert_allclose(r["t"]["prio"], met["prio"].numpy(), rtol=0, atol=1e-10)
    for k in sc.SAC_KEYS if kw["tune_alpha"] else sc.SAC_KEYS[:9]:
        assert abs(r["met"][k] - float(torch.as_tensor(met["train/" + k]).detach())) <= 1e-10 * max(1.0, abs(r["met"][k])), k


def test_the_clip_is_active_where_the_case_says_so():
    for dtype in DTYPES:
        r = sc.sac_reference(sc.SAC_CLIP_CASE, dtype)
        assert r["cnorm"] > 2 * sc.SAC_CLIP_NORM and r["anorm"] > 2 * sc.SAC_CLIP_NORM
        assert r["ccoef"] < 0.5 and r["acoef"] < 0.5
    d = sc.sac_dims(sc.SAC_CLIP_CASE)
    assert 2 * (272 + 17 + 16 * ((d["DK"] + 1 + 15) // 16)) == 2114  # nsq_c: a second trip of the re-sum


def test_the_tail_case_has_its_largest_weight_last():
    p = sc.sac_inputs(sc.SAC_TAIL_CASE)["probs"]
    assert int(np.argmin(p)) == 519 and 519 >= 512


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sc.SAC_CASES)
def test_stand_in_holds_every_bound_with_a_quarter(case, dtype):
    s, bad, fig, ref, log = _stand_in(case, dtype)
    print(log)
    assert not bad, list(bad)
    # no undecided row: in the reference on the stand-in's tensors, in the chained reference, and in
    # the stand-in itself
    assert ref["undecided"] == [] and s["undecided"] == []
    assert sc.sac_reference(case, dtype)["undecided"] == []


# defect -> (the stage whose check it must break, the case it is planted at)
PLANTED = {
    "ones_row": ("critic_wgrad", (37, 60, 6)),
    "pad_col": ("layout", (17, 11, 16)),
    "swap_head_row": ("heads", (37, 60, 6)),
    "actor_min_q1": ("actor_loss", (37, 60, 6)),
    "wrong_n": ("critic_loss", (16, 3, 1)),
    "clip_off": ("critic_clip", sc.SAC_CLIP_CASE),
    "polyak_first": ("critic_adam", (37, 26, 6)),
    "w1_shift": ("actor_head_bwd", (17, 11, 16)),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", sorted(PLANTED))
def test_planted_defect_breaks_its_own_stage_and_no_earlier_one(defect, dtype):
    stage, case = PLANTED[defect]
    assert defect == "pad_col" or defect in sst.DEFECTS
    _, bad, _, _, log = _stand_in(case, dtype, defect)
    stages = [s for s, _ in bad]
    assert stage in stages, (defect, list(bad))
    assert bad.first_stage() == sc.SAC_STAGES.index(stage), (defect, list(bad))


def test_policy_head_bound_holds_on_the_stand_in_with_a_quarter():
    """The small-(1 - y^2) case of sac_policy: the float32 stand-in of the head (numpy float32, one
    rounding per operation as the kernel's) against hold_sac_policy's derived bound."""
    n, D, K = sc.SAC_POLICY_CASE
    a0, obs, eps = sc.sac_policy_inputs()
    P = sst.split_actor(a0, D, K, torch.float32)
    with torch.no_grad():
        h = torch.relu(torch.from_numpy(obs) @ P["w1"].T + P["b1"])
        h = torch.relu(h @ P["w2"].T + P["b2"])
        o = sst.policy_head(h, P, torch.from_numpy(eps))
    f = np.float32
    mean, sd = o["mean"].numpy(), o["sd"].numpy()
    x = (mean + eps * sd).astype(f)
    y = np.tanh(x).astype(f)
    xm = (x - mean).astype(f)
    lp = ((-(xm * xm).astype(f) / (f(2) * (sd * sd).astype(f)).astype(f)).astype(f) - np.log(sd).astype(f)).astype(f)
    lp = (lp - f(sst.LOG_SQRT_2PI)).astype(f)
    lp = (lp - np.log(((f(1) - (y * y).astype(f)).astype(f) + f(1e-6)).astype(f)).astype(f)).astype(f)
    logp = np.zeros(n, f)
    for k in range(K):
        logp = (logp + lp[:, k]).astype(f)
    assert sc.hold_sac_policy(mean, sd, y, logp, eps, "stand-in", share=0.25) == []
    # a log-prob off by the ill-conditioned term's own size is caught
    assert sc.hold_sac_policy(mean, sd, y, logp + f(0.5), eps, "stand-in +0.5") != []
