"""The distributional (IQN) actor path on the GPU: forward, act, the library's
taus, target sync, the actor's n-step targets and the quantile-regression loss head against the
reference's own outputs (tests/golden/make_iqn_golden.py) and the oracle (tests/iqn_oracle.py).

Tolerances: fp32 forward rtol 1e-4 / atol 1e-5 (what test_gpu_dqn.py holds the dueling forward
to); loss head 1e-5 rel on identical inputs (as test_dqn_loss_head_matches_reference); n-step
targets bitwise the scalar ingest's, priorities 1e-6 rel; bf16 forward at most 3x the dueling
forward's bf16-vs-fp32 rel-L2 on the same frames (two more bf16 roundings: the Wq operand and y
after the modulation, whose features have heavier tails).
"""
import os

import numpy as np
import pytest
import torch

import iqn_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FWD = dict(rtol=1e-4, atol=1e-5)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _setup(dev, n, A, W, online, target=None, dtype="fp32"):
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
    m.load_flat(online, online if target is None else target)
    e = IqnEngine(m, batch_size=n)
    m._train_engine = e
    return m, e


@pytest.fixture(scope="module")
def fix():
    """The fixtures' model (A = 6, W = 8, the target net nudged) on a 16-frame handle, and the
    64 candidate frames, regenerated from the fixtures' seeds."""
    dev = _dev()
    f = np.load(os.path.join(G, "iqn_forward.npz"))
    a = np.load(os.path.join(G, "iqn_act.npz"))
    A, W = int(f["A"]), int(f["W"])
    online = orc.fixture_params(A, int(f["param_seed"]))
    target = (online + 0.05 * (orc.fixture_params(A, int(f["target_seed"])) - online)).astype(np.float32)
    m, e = _setup(dev, 16, A, W, online, target)
    obs = orc.fixture_obs(int(f["obs_seed"]))
    return dict(f=f, a=a, A=A, W=W, online=online, target=target, m=m, e=e, obs=obs, dev=dev,
                act_obs=_t(obs[a["frame_idx"]], dev))


# ---------------------------------------------------------------- forward
def test_iqn_forward_matches_reference(fix):
    f, e, dev = fix["f"], fix["e"], fix["dev"]
    obs = _t(fix["obs"][:4], dev)
    for which, key in ((False, "online"), (True, "target")):
        q, used = e.forward(obs, target=which, taus=_t(f["taus_" + key], dev))
        q = q.cpu().numpy()
        print(key, "max |q|", np.abs(f["q_" + key]).max(), "max abs err", np.abs(q - f["q_" + key]).max(),
              "rel-L2", _rel_l2(q, f["q_" + key]))
        assert np.array_equal(used.cpu().numpy(), f["taus_" + key])  # the taus used are handed back
        np.testing.assert_allclose(q, f["q_" + key], **FWD)


@pytest.mark.parametrize("n,W,A", [(1, 1, 2), (3, 8, 6), (5, 32, 15), (2, 5, 15)])
def test_iqn_forward_edge_shapes_vs_oracle(n, W, A):
    """R = 1; R = 24 (a 16-row tile crossing frames, the last one ragged); R = 160; a W that is no
    power of two.  The taus hold 0 and the two largest float32 below 1.  Against the oracle in
    float64 (the fp32 reference itself sits about 1e-5 from it)."""
    dev = _dev()
    online, target = orc.fixture_params(A, 31 + A), orc.fixture_params(A, 32 + A)
    obs = orc.fixture_obs(100 + n, n)
    taus = orc.edge_taus(n, W, seed=n)
    assert taus.min() == 0.0 and taus.max() < 1.0
    m, e = _setup(dev, n, A, W, online, target)
    for which, flat in ((False, online), (True, target)):
        with torch.no_grad():
            want = orc.make_net(flat, A, torch.float64)(torch.from_numpy(obs), torch.from_numpy(taus)).numpy()
        q = e.forward(_t(obs, dev), target=which, taus=_t(taus, dev))[0].cpu().numpy()
        assert q.shape == (n, W, A)
        print((n, W, A), "target" if which else "online", "max abs err", np.abs(q - want).max(),
              "rel-L2", _rel_l2(q, want))
        np.testing.assert_allclose(q, want, **FWD)


def test_iqn_fewer_frames_than_the_handle(fix):
    f, e, dev = fix["f"], fix["e"], fix["dev"]
    q = e.forward(_t(fix["obs"][:3], dev), taus=_t(f["taus_online"][:3], dev))[0].cpu().numpy()
    np.testing.assert_allclose(q, f["q_online"][:3], **FWD)
    with pytest.raises(RuntimeError, match="batch_size"):
        e.forward(_t(fix["obs"][:17], dev))


def test_iqn_library_taus(fix):
    """n W = 4096 library-drawn taus: in [0, 1), the restatement's bits, the same for one
    (seed, counter), other values for another counter and for the target stream, and a mean within
    6 sigma of 1/2 (sigma = 1 / sqrt(12 * 4096) = 0.0045)."""
    dev = fix["dev"]
    m, e = _setup(dev, 128, fix["A"], 32, fix["online"], fix["target"])
    obs = _t(orc.fixture_obs(9, 128), dev)
    q1, t1 = e.forward(obs, seed=7, counter=3)
    q2, t2 = e.forward(obs, seed=7, counter=3)
    _, t3 = e.forward(obs, seed=7, counter=4)
    _, t4 = e.forward(obs, target=True, seed=7, counter=3)
    u = t1.cpu().numpy()
    assert u.shape == (128, 32) and u.min() >= 0.0 and u.max() < 1.0
    assert torch.equal(t1, t2) and torch.equal(q1, q2)
    assert not torch.equal(t1, t3) and not torch.equal(t1, t4)
    print("mean of 4096 taus", float(u.mean()))
    assert abs(float(u.mean()) - 0.5) < 0.027
    assert np.array_equal(u.reshape(-1), orc.draw_taus(7, 3, 0, 4096))
    assert np.array_equal(t4.cpu().numpy().reshape(-1), orc.draw_taus(7, 3, 1, 4096))
    # the drawn taus are the ones the net ran on
    q3, _ = e.forward(obs, taus=t1)
    assert torch.equal(q3, q1)


# ---------------------------------------------------------------- act
def _act_oracle(fix):
    a = fix["a"]
    obs = torch.from_numpy(fix["obs"][a["frame_idx"]])
    with torch.no_grad():
        q_on = orc.make_net(fix["online"], fix["A"])(obs, torch.from_numpy(a["taus_online"])).numpy()
        q_tg = orc.make_net(fix["target"], fix["A"])(obs, torch.from_numpy(a["taus_target"])).numpy()
    return orc.act_parts(q_on, q_tg)


def test_iqn_act_greedy(fix):
    a, e, dev = fix["a"], fix["e"], fix["dev"]
    parts = _act_oracle(fix)
    assert orc.top2_gap(parts["qbar"]).min() > 1e-3  # on the oracle alone: every frame decides
    assert np.array_equal(parts["greedy"], a["greedy"])
    t_on, t_tg = _t(a["taus_online"], dev), _t(a["taus_target"], dev)
    act, q_pi, q_star, g = [x.cpu().numpy() for x in e.act(fix["act_obs"], 0.0, seed=1, counter=1,
                                                          taus_online=t_on, taus_target=t_tg)]
    assert np.array_equal(g, parts["greedy"]) and np.array_equal(act, parts["greedy"])
    np.testing.assert_allclose(q_pi, a["qbar"][np.arange(16), a["greedy"]], **FWD)
    assert q_star.shape == (16, fix["W"])
    np.testing.assert_allclose(q_star, a["q_star"], **FWD)
    # eps = 1: never the greedy action; q_pi is qbar at the action drawn
    act, q_pi, _, g = [x.cpu().numpy() for x in e.act(fix["act_obs"], 1.0, seed=1, counter=2,
                                                     taus_online=t_on, taus_target=t_tg)]
    assert np.array_equal(g, parts["greedy"]) and not np.any(act == g)
    np.testing.assert_allclose(q_pi, a["qbar"][np.arange(16), act], **FWD)
    # per-frame eps: even frames greedy, odd frames never greedy
    eps = torch.tensor([0.0, 1.0] * 8)
    act = e.act(fix["act_obs"], eps, seed=1, counter=3, taus_online=t_on, taus_target=t_tg)[0].cpu().numpy()
    assert np.array_equal(act[0::2], g[0::2]) and not np.any(act[1::2] == g[1::2])


def test_iqn_act_draw_frequencies(fix):
    """eps = 0.4 over fixed (seed, counters): greedy with probability 0.6, else uniform over the
    other A - 1 actions.  Pooled over frames by rank (greedy -> 0, the others in index order):
    chi-square with A - 1 degrees of freedom against its critical value at p = 1e-6."""
    from scipy.stats import chi2 as chi2_dist
    a, e, dev, A = fix["a"], fix["e"], fix["dev"], fix["A"]
    t_on, t_tg = _t(a["taus_online"], dev), _t(a["taus_target"], dev)
    greedy = a["greedy"]
    counts = np.zeros(A)
    reps = 60
    for c in range(reps):
        act = e.act(fix["act_obs"], 0.4, seed=1234, counter=100 + c, taus_online=t_on,
                    taus_target=t_tg)[0].cpu().numpy()
        rank = np.where(act == greedy, 0, np.where(act < greedy, act + 1, act))
        counts += np.bincount(rank, minlength=A)
    n = reps * 16
    exp = np.array([0.6] + [0.4 / (A - 1)] * (A - 1)) * n
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print(f"act draw chi2 ({A - 1} dof)", chi2, counts)
    assert chi2 < chi2_dist.isf(1e-6, A - 1)


def test_iqn_act_refuses_one_action():
    dev = _dev()
    m, e = _setup(dev, 2, 1, 4, orc.fixture_params(1, 3))
    with pytest.raises(_unsupported()):
        e.act(_t(orc.fixture_obs(1, 2), dev), 0.0, seed=0, counter=0)


def _unsupported():
    from impala_amd._lib import Unsupported
    return Unsupported


# ---------------------------------------------------------------- target sync, refresh
def test_iqn_sync_target_is_bitwise_and_refresh_repacks(fix):
    from impala_amd.iqn import net_specs
    a, dev = fix["a"], fix["dev"]
    m, e = _setup(dev, 16, fix["A"], fix["W"], fix["online"], fix["target"])
    taus = _t(a["taus_online"], dev)
    q_on = e.forward(fix["act_obs"], taus=taus)[0]
    assert not torch.equal(e.forward(fix["act_obs"], target=True, taus=taus)[0], q_on)
    e.sync_target()
    assert torch.equal(e.forward(fix["act_obs"], target=True, taus=taus)[0], q_on)
    assert torch.equal(m.target_flat, m.flat)
    # a host write of Wq reaches the kernels through iqn_refresh_weights (params_changed)
    off = 0
    for k, shape in net_specs(fix["A"]):
        if k == "q.quantile_layer.output_layer.0.weight":
            break
        off += int(np.prod(shape))
    with torch.no_grad():
        m.flat[off:off + 1024 * 64] *= 1.5
    assert torch.equal(e.forward(fix["act_obs"], taus=taus)[0], q_on)  # the packed copy, until told
    m.params_changed()
    q_new = e.forward(fix["act_obs"], taus=taus)[0]
    assert not torch.equal(q_new, q_on)
    with torch.no_grad():
        want = orc.make_net(m.flat.cpu().numpy(), fix["A"], torch.float64)(
            torch.from_numpy(fix["obs"][a["frame_idx"]]), torch.from_numpy(a["taus_online"])).numpy()
    np.testing.assert_allclose(q_new.cpu().numpy(), want, **FWD)


# ---------------------------------------------------------------- actor ingest
def _rollout(L, W, seed):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal(L).astype(np.float32)
    done = np.zeros(L, dtype=bool)
    done[L - 1] = True  # one on the last step
    if L > 2:
        done[L // 2] = True  # one mid-rollout
    q_pi = rng.standard_normal(L).astype(np.float32)
    q_star = rng.standard_normal((L, W)).astype(np.float32)
    return r, done, q_pi, q_star


@pytest.mark.parametrize("n_step", [1, 3, 16])
@pytest.mark.parametrize("L", [2, 5, 100])
def test_iqn_nstep_targets(L, n_step):
    """Bitwise the scalar ingest's targets (dqn_replay_extend_rollout) at W = 1 and for every
    fourth column of W = 8; the numpy restatement in float64 for W in {1, 8, 32}."""
    from impala_amd.dqn import NativePrioritizedReplay
    from impala_amd.iqn import iqn_nstep_targets
    dev = _dev()
    s = torch.zeros(L, 3, 64, 64, dtype=torch.uint8, device=dev)
    act = torch.zeros(L, dtype=torch.int64, device=dev)

    def scalar_ingest(r, done, q_pi, col, gamma):
        rb = NativePrioritizedReplay(128, device=dev, seed=0)
        keys = rb.extend_rollout(s, act, _t(r, dev), _t(done, dev), _t(q_pi, dev), _t(col, dev), n_step, gamma)
        return rb.target[keys].cpu().numpy(), rb.priorities[keys].cpu().numpy()

    for gamma in (0.0, 0.99):
        for W in (1, 8, 32):
            r, done, q_pi, q_star = _rollout(L, W, seed=L * 100 + W)
            tg, prio = iqn_nstep_targets(_t(r, dev), _t(done, dev), _t(q_pi, dev), _t(q_star, dev), n_step, gamma)
            tg, prio = tg.cpu().numpy(), prio.cpu().numpy()
            assert tg.shape == (L - 1, W) and prio.shape == (L - 1,)
            want_t, want_p = orc.nstep_targets(r, done, q_pi, q_star, n_step, gamma)
            np.testing.assert_allclose(tg, want_t, rtol=1e-6, atol=1e-6)
            # the priority stage on the kernel's own targets, in the order the header defines (a
            # k-ordered fp32 sum, divided by W): 1e-6 rel
            acc = np.zeros(L - 1, np.float32)
            for k in range(W):
                acc = acc + tg[:, k]
            np.testing.assert_allclose(prio, np.abs(acc / np.float32(W) - q_pi[:-1]), rtol=1e-6, atol=0)
            # against float64 the priority inherits the targets' roundings: one per FMA (n_step of
            # them, each at most 2^-24 of the return of the magnitudes, an upper bound of every
            # intermediate), W additions and a division for the mean, one subtraction
            mag, _ = orc.nstep_targets(np.abs(r), done, q_pi, np.abs(q_star), n_step, gamma)
            bound = (n_step + W + 2) * 2.0 ** -24 * (mag.mean(1) + np.abs(q_pi[:-1]))
            assert np.all(np.abs(prio - want_p) <= bound)
            if W == 1 or W == 8:
                for k in range(0, W, 4):
                    t1, p1 = scalar_ingest(r, done, q_pi, q_star[:, k].copy(), gamma)
                    assert np.array_equal(tg[:, k], t1), (gamma, W, k)
                    if W == 1:
                        assert np.array_equal(prio, p1)
            if gamma == 0.0:
                assert np.array_equal(tg, np.repeat(r[:-1, None], W, 1))


# ---------------------------------------------------------------- loss head
@pytest.mark.parametrize("tag,kappa", [("k1", 1.0), ("k0", 0.0)])
def test_iqn_loss_head_matches_reference(tag, kappa):
    from impala_amd.iqn import iqn_loss_head
    dev = _dev()
    d = np.load(os.path.join(G, "iqn_head.npz"))
    x = {k: d[f"{k}_{tag}"] for k in ("adv", "v", "act", "taus", "target", "prob", "scalars", "dadv",
                                      "dv", "priorities")}
    out = iqn_loss_head(_t(x["adv"], dev), _t(x["v"], dev), _t(x["act"], dev), _t(x["taus"], dev),
                        _t(x["target"], dev), _t(x["prob"], dev), kappa, float(d["beta"]))
    np.testing.assert_allclose(out["metrics"].cpu().numpy(), x["scalars"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["dadv"].cpu().numpy(), x["dadv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["dv"].cpu().numpy(), x["dv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["priorities"].cpu().numpy(), x["priorities"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("kappa", [1.0, 0.0])
@pytest.mark.parametrize("probs", [True, False], ids=["probs", "noprobs"])
@pytest.mark.parametrize("Ws,Wt", [(1, 1), (8, 8), (32, 8), (8, 32)])
@pytest.mark.parametrize("N,A", [(1, 2), (1, 15), (33, 2), (33, 15), (300, 6)])
def test_iqn_loss_head_shapes_vs_oracle(N, A, Ws, Wt, probs, kappa):
    """One transition, a ragged block, more than one block of 256; the inputs hold the exact ties
    delta = 0 and |delta| = kappa (iqn_oracle.head_inputs).  Against the oracle in float64 at the
    reference test's relative tolerance; the gradients' absolute floor is one rounding of a
    quantile's sum: dq = (w / (N Wt)) sum_j rho g with |rho g| <= 1 and w <= 1, so |sum| <= Wt and
    its fp32 rounding is at most Wt 2^-24, i.e. 2^-24 / N on dq.  Two runs are bitwise equal."""
    from impala_amd.iqn import iqn_loss_head
    dev = _dev()
    adv, v, act, taus, tgt, p = orc.head_inputs(N, Ws, Wt, A, kappa, seed=N + Ws, probs=probs)
    exp = orc.loss_from_heads(adv, v, act, taus, tgt, p, kappa, dtype=torch.float64)
    args = [_t(x, dev) for x in (adv, v, act, taus, tgt, p)]
    out = iqn_loss_head(*args, kappa)
    floor = 2.0 ** -24 / N
    np.testing.assert_allclose(out["metrics"].cpu().numpy(), exp["metrics"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["dadv"].cpu().numpy(), exp["dadv"], rtol=1e-5, atol=floor)
    np.testing.assert_allclose(out["dv"].cpu().numpy(), exp["dv"], rtol=1e-5, atol=floor)
    np.testing.assert_allclose(out["priorities"].cpu().numpy(), exp["priorities"], rtol=1e-5, atol=1e-7)
    again = iqn_loss_head(*args, kappa)
    for k in ("metrics", "dadv", "dv", "priorities"):
        assert torch.equal(out[k], again[k]), k


# ---------------------------------------------------------------- bf16
def test_iqn_bf16_tracks_fp32(fix):
    """rel-L2 of the bf16 forward's q against the fp32 forward's on the same frames and taus, at
    most 3x what the dueling forward (the same trunk, projection and heads without the quantile
    layer) shows on those frames."""
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    from impala_amd.iqn import net_specs
    dev, A, W = fix["dev"], fix["A"], fix["W"]
    obs = _t(fix["obs"], dev)  # 64 frames
    taus = _t(np.random.default_rng(2).random((64, W)).astype(np.float32), dev)
    q = {}
    for dt in ("fp32", "bf16"):
        m, e = _setup(dev, 64, A, W, fix["online"], fix["target"], dtype=dt)
        q[dt] = e.forward(obs, taus=taus)[0].cpu().numpy()
    # the dueling net on the same parameters: the flat layout without the quantile layer's segment
    keep, off = [], 0
    for k, shape in net_specs(A):
        n = int(np.prod(shape))
        if "quantile_layer" not in k:
            keep.append(fix["online"][off:off + n])
        off += n
    dflat = np.concatenate(keep)
    qd = {}
    for dt in ("fp32", "bf16"):
        dm = AtariDQNModel((3, 64, 64), A, device=dev, dtype=dt, seed=0)
        dm.load_flat(dflat, dflat)
        qd[dt] = DqnEngine(dm, batch_size=64, inference_only=True).forward(obs).cpu().numpy()
    iqn_err, dqn_err = _rel_l2(q["bf16"], q["fp32"]), _rel_l2(qd["bf16"], qd["fp32"])
    print("bf16 vs fp32 rel-L2: iqn", iqn_err, "dueling", dqn_err, "ratio", iqn_err / dqn_err)
    assert iqn_err <= 3.0 * dqn_err


# ---------------------------------------------------------------- end to end
def test_iqn_actor_end_to_end():
    """Builder -> network -> actor -> 3 rollouts of L = 6 into PrioritizedReplay(target_width=W):
    the ring's targets and priorities are the oracle's on what the model's act returned, and the
    first step's outputs are the oracle net's on the taus the library drew."""
    from impala_amd.config import load_config
    from impala_amd.iqn import ApexDistributionalBuilder
    dev = _dev()
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = str(dev)
    cfg.agent.replay_buffer_size = 32
    cfg.agent.rollout_length = 6
    b = ApexDistributionalBuilder(cfg)
    torch.manual_seed(0)
    model = b.make_network()
    W, A = model.n_tau_samples, model.action_dim
    with torch.no_grad():  # a target net that differs, published to the actor's copy
        model.target_flat.mul_(1.01)
    model.params_changed()
    model.push()
    actor_model = b._actor_model
    actor_model._act_seed = 20240  # the library's taus and draws, the same in every run
    rb = b.make_replay()
    actor = b.make_actor(actor_model, rb)(0)
    log = []
    real_act = actor_model.act
    actor_model.act = lambda obs, eps: log.append(real_act(obs, eps)) or log[-1]
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
    assert len(rb) == 15 and len(log) == 18
    # step 1 against the oracle net on the drawn taus
    seed = actor_model._act_seed
    on = orc.make_net(actor_model.flat.cpu().numpy(), A, torch.float64)
    tg = orc.make_net(actor_model.target_flat.cpu().numpy(), A, torch.float64)
    x = torch.from_numpy(frames[:1])
    with torch.no_grad():
        parts = orc.act_parts(on(x, torch.from_numpy(orc.draw_taus(seed, 1, 0, W)).reshape(1, W)).numpy(),
                              tg(x, torch.from_numpy(orc.draw_taus(seed, 1, 1, W)).reshape(1, W)).numpy())
    a0, q_pi0, q_star0 = log[0]
    assert a0.shape == (1, 1) and q_pi0.shape == (1, 1) and q_star0.shape == (1, W)
    if orc.top2_gap(parts["qbar"])[0] > 1e-3:
        np.testing.assert_allclose(q_star0.numpy(), parts["q_star"], **FWD)
        np.testing.assert_allclose(float(q_pi0), parts["qbar"][0, int(a0)], **FWD)
    # the ring against the oracle's targets and priorities, rollout by rollout
    for k in range(3):
        sl = slice(6 * k, 6 * k + 6)
        q_pi = np.array([float(x[1]) for x in log[sl]], np.float32)
        q_star = np.stack([x[2].numpy().reshape(-1) for x in log[sl]])
        want_t, want_p = orc.nstep_targets(rew[sl], done[sl], q_pi, q_star, int(cfg.agent.n_step), 0.99)
        rows = slice(5 * k, 5 * k + 5)
        np.testing.assert_allclose(rb.target[rows].cpu().numpy(), want_t, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(rb.priorities[rows].cpu().numpy(), want_p, rtol=1e-5, atol=1e-6)
        assert np.array_equal(rb.s[rows].cpu().numpy(), frames[sl][:5])
        assert np.array_equal(rb.a[rows].cpu().numpy(), np.array([int(x[0]) for x in log[sl]][:5]))
