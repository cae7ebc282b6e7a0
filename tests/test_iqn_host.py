"""The distributional (IQN) actor path's boundary and host logic on CPU: the oracle
(tests/iqn_oracle.py) against the reference's own fixtures, include/iqn_hip.h vs the binding vs the
library's exports, argument validation without a device, state_dict keys, the wide-target
PrioritizedReplay, the builder's surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dqn_replay_oracle as rorc
import iqn_oracle as orc
from impala_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "iqn_hip.h")
G = os.path.join(REPO, "tests", "golden")


def _fixture_nets(d):
    A = int(d["A"])
    online = orc.fixture_params(A, int(d["param_seed"]))
    target = (online + 0.05 * (orc.fixture_params(A, int(d["target_seed"])) - online)).astype(np.float32)
    return A, online, target


# ---------------------------------------------------------------- oracle vs reference
def test_oracle_forward_matches_reference():
    d = np.load(os.path.join(G, "iqn_forward.npz"))
    A, online, target = _fixture_nets(d)
    obs = torch.from_numpy(orc.fixture_obs(int(d["obs_seed"]))[:4])
    with torch.no_grad():
        q_on = orc.make_net(online, A)(obs, torch.from_numpy(d["taus_online"])).numpy()
        q_tg = orc.make_net(target, A)(obs, torch.from_numpy(d["taus_target"])).numpy()
    assert q_on.shape == (4, int(d["W"]), A)
    np.testing.assert_allclose(q_on, d["q_online"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(q_tg, d["q_target"], rtol=1e-5, atol=1e-6)
    assert np.abs(q_on - q_tg).max() > 1e-3  # the target net is a different net


def test_oracle_act_matches_reference():
    f, d = np.load(os.path.join(G, "iqn_forward.npz")), np.load(os.path.join(G, "iqn_act.npz"))
    A, online, target = _fixture_nets(f)
    obs = torch.from_numpy(orc.fixture_obs(int(f["obs_seed"]))[d["frame_idx"]])
    with torch.no_grad():
        q_on = orc.make_net(online, A)(obs, torch.from_numpy(d["taus_online"])).numpy()
        q_tg = orc.make_net(target, A)(obs, torch.from_numpy(d["taus_target"])).numpy()
    np.testing.assert_allclose(q_on, d["q_online"], rtol=1e-5, atol=1e-6)
    parts = orc.act_parts(q_on, q_tg)
    assert orc.top2_gap(parts["qbar"]).min() > 1e-3
    np.testing.assert_allclose(parts["qbar"], d["qbar"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(parts["greedy"], d["greedy"])
    np.testing.assert_allclose(parts["q_star"], d["q_star"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("tag,kappa", [("k1", 1.0), ("k0", 0.0)])
def test_oracle_head_matches_reference(tag, kappa):
    d = np.load(os.path.join(G, "iqn_head.npz"))
    x = {k: d[f"{k}_{tag}"] for k in ("adv", "v", "act", "taus", "target", "prob", "scalars", "dadv",
                                      "dv", "priorities")}
    out = orc.loss_from_heads(x["adv"], x["v"], x["act"], x["taus"], x["target"], x["prob"], kappa,
                              float(d["beta"]))
    np.testing.assert_allclose(out["metrics"], x["scalars"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(out["dadv"], x["dadv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["dv"], x["dv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["priorities"], x["priorities"], rtol=1e-6, atol=1e-7)
    assert x["prob"].max() / x["prob"].min() > 50  # spread over about two decades
    # the inputs hold the exact ties: delta = 0 and |delta| = kappa on transition 0
    q00 = np.float32(x["v"][0, 0] + x["adv"][0, 0, x["act"][0]])
    assert x["target"][0, 0] == q00 and x["target"][0, 1] == np.float32(q00 + np.float32(kappa))


def test_nstep_restatement_at_one_column_is_the_scalar_one():
    rng = np.random.default_rng(3)
    L = 23
    r, q_star = rng.standard_normal(L), rng.standard_normal((L, 1))
    done = rng.random(L) < 0.2
    q_pi = rng.standard_normal(L)
    for n_step in (1, 3, 16):
        tg, prio = orc.nstep_targets(r, done, q_pi, q_star, n_step, 0.99)
        want = rorc.nstep_targets(r, done, q_star[:, 0], n_step, 0.99)
        assert np.array_equal(tg[:, 0], want)
        assert np.array_equal(prio, np.abs(want - q_pi[:-1]))


def test_tau_draw_restatement():
    u = orc.draw_taus(5, 9, 0, 4096)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.027  # 6 sigma of a uniform mean at n = 4096
    assert not np.array_equal(u, orc.draw_taus(5, 9, 1, 4096))
    assert not np.array_equal(u, orc.draw_taus(5, 10, 0, 4096))


# ---------------------------------------------------------------- C boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(iqn_\w+)\s*\(", src)))


def test_header_declares_what_the_binding_expects():
    assert _declared() == sorted(_lib.IQN_EXPORTS)


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\b(iqn_\w+)\b", out))
    for name in _declared():
        assert name in exported, name
        assert hasattr(lib, name)
    assert lib.iqn_abi_version() == _lib.IQN_ABI_VERSION


def test_struct_layout_matches_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct iqn_config \{(.*?)\} iqn_config;", src, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [f for f, _ in _lib.IqnConfig._fields_]
    assert all(t is C.c_int for _, t in _lib.IqnConfig._fields_)
    assert int(re.search(r"#define IQN_MAX_TAU (\d+)", src).group(1)) == _lib.IQN_MAX_TAU
    assert int(re.search(r"#define IQN_MAX_ROWS (\d+)", src).group(1)) == _lib.IQN_MAX_ROWS


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "hdr.c"
    src.write_text('#include "iqn_hip.h"\n'
                   "int main(void) { iqn_config c; c.n_tau = IQN_MAX_TAU; return c.n_tau == 32 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c",
                        str(src), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_param_count_and_defaults():
    from impala_amd import dqn, iqn
    lib = _lib.lib()
    assert lib.iqn_param_count(15) == 677552 == iqn.param_count(15)
    assert iqn.param_count(15) - dqn.param_count(15) == 66560
    for A in (1, 6):
        assert lib.iqn_param_count(A) == iqn.param_count(A)
    cfg = iqn.default_config()
    assert (cfg.batch_size, cfg.num_actions, cfg.n_tau, cfg.dtype) == (128, 15, 8, 0)


@pytest.mark.parametrize("field,value", [("batch_size", 0), ("num_actions", 0), ("num_actions", 16),
                                         ("n_tau", 0), ("n_tau", 33), ("batch_size", 2049),
                                         ("dtype", 7)])
def test_create_rejects_bad_config_without_touching_the_device(field, value):
    from impala_amd import iqn
    lib = _lib.lib()
    cfg = iqn.default_config()  # n_tau 8: 2049 frames are 16392 rows, past IQN_MAX_ROWS
    setattr(cfg, field, value)
    h = _lib._P()
    status = lib.iqn_create(C.byref(cfg), 0, C.byref(h))
    assert status in (1001, 1003) and not h.value
    assert lib.iqn_last_error()


def test_entry_points_validate_before_launch():
    lib = _lib.lib()
    assert lib.iqn_forward(None, None, 1, 0, None, 0, 0, None, None, None) == 1001
    assert lib.iqn_forward(None, None, 1, 2, None, 0, 0, None, None, None) == 1001
    assert lib.iqn_act(None, None, 1, None, 0.0, 0, 0, None, None, None, None, None, None, None) == 1001
    assert lib.iqn_bind_params(None, None, None, None) == 1001
    assert lib.iqn_sync_target(None, None) == 1001
    assert lib.iqn_refresh_weights(None, None) == 1001
    assert lib.iqn_destroy(None) == 0
    # the handle-free entries: every bad size, then the null pointers, before any launch
    nstep = lambda L, W, n, g: lib.iqn_nstep_targets(None, None, None, None, L, W, n, g, None, None, None)
    for args in ((1, 8, 3, 0.99), (5, 0, 3, 0.99), (5, 33, 3, 0.99), (5, 8, 0, 0.99), (5, 8, 17, 0.99),
                 (5, 8, 3, 1.5), (5, 8, 3, 0.99)):
        assert nstep(*args) == 1001, args
    head = lambda N, Ws, Wt, A, k: lib.iqn_loss_head(None, None, None, None, None, None, N, Ws, Wt, A, k,
                                                     0.4, None, None, None, None, None)
    for args in ((0, 8, 8, 6, 1.0), (4, 0, 8, 6, 1.0), (4, 8, 33, 6, 1.0), (4, 8, 8, 16, 1.0),
                 (4, 8, 8, 6, -1.0), (4, 8, 8, 6, 1.0)):
        assert head(*args) == 1001, args


# ---------------------------------------------------------------- model
def test_state_dict_keys_shapes_dtypes_match_reference():
    from impala_amd.iqn import DistributionalAtariDQN
    d = np.load(os.path.join(G, "iqn_forward.npz"))
    m = DistributionalAtariDQN((3, 64, 64), int(d["A"]), int(d["W"]), device="cpu", seed=0)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in d["state_dict_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in d["state_dict_shapes"]]
    assert [str(v.dtype) for v in sd.values()] == [str(s) for s in d["state_dict_dtypes"]]
    assert "online_net.q.quantile_layer.embedding_range" in sd
    assert all(p.requires_grad for p in m.online_net.parameters())
    assert not any(p.requires_grad for p in m.target_net.parameters())
    assert torch.equal(m.flat, m.target_flat)
    assert [k for k, _ in m.online_net.named_parameters()] == [k for k, _ in __import__(
        "impala_amd.iqn", fromlist=["net_specs"]).net_specs(int(d["A"]))]
    with pytest.raises(RuntimeError):
        m.forward(torch.zeros(1, 3, 64, 64, dtype=torch.uint8))


def test_strict_load_from_a_reference_shaped_state_dict():
    from impala_amd.iqn import DistributionalAtariDQN
    d = np.load(os.path.join(G, "iqn_forward.npz"))
    A = int(d["A"])
    ref = {}
    for half, seed in (("online_net", 1), ("target_net", 2)):  # the oracle net has the reference's keys
        net = orc.make_net(orc.fixture_params(A, seed), A)
        ref.update({f"{half}.{k}": v.clone() for k, v in net.state_dict().items()})
    assert list(ref.keys()) == [str(k) for k in d["state_dict_keys"]]
    m = DistributionalAtariDQN((3, 64, 64), A, 8, device="cpu", seed=0)
    v0 = m._version
    res = m.load_state_dict(ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and m._version > v0
    assert np.array_equal(m.flat.numpy(), orc.fixture_params(A, 1))
    assert np.array_equal(m.target_flat.numpy(), orc.fixture_params(A, 2))
    rng_buf = m.state_dict()["target_net.q.quantile_layer.embedding_range"]
    assert rng_buf.dtype == torch.int64 and rng_buf.reshape(-1).tolist() == list(range(1, 65))


def test_model_pickles_and_clones(tmp_path):
    from impala_amd.iqn import DistributionalAtariDQN
    m = DistributionalAtariDQN((3, 64, 64), 6, 8, device="cpu", seed=3)
    m.target_flat.add_(1.0)
    torch.save(m, tmp_path / "m.pt")
    m2 = torch.load(tmp_path / "m.pt", weights_only=False)
    assert torch.equal(m2.flat, m.flat) and torch.equal(m2.target_flat, m.target_flat)
    assert m2.n_tau_samples == 8 and list(m2.state_dict().keys()) == list(m.state_dict().keys())
    m2.flat[0] = 7.0  # still views after unpickling
    assert float(m2.get_parameter("online_net.body.body.0.weight").detach().reshape(-1)[0]) == 7.0
    c = m.clone_to("cpu")
    assert torch.equal(c.flat, m.flat) and not any(p.requires_grad for p in c.parameters())
    assert c.n_tau_samples == 8
    m.sync_target_net()
    assert torch.equal(m.target_flat, m.flat)


def test_init_is_seeded_and_ordered():
    from impala_amd.iqn import DistributionalAtariDQN, net_specs
    a = DistributionalAtariDQN((3, 64, 64), 6, 8, device="cpu", seed=0)
    b = DistributionalAtariDQN((3, 64, 64), 6, 8, device="cpu", seed=0)
    assert torch.equal(a.flat, b.flat)
    sd = a.state_dict()
    for k, shape in net_specs(6):
        t = sd["online_net." + k]
        if k.endswith(".bias"):
            assert float(t.abs().max()) == 0.0
        elif k == "q.project.0.weight":
            assert bool((t == 1).all())
        else:  # truncated normal of std sqrt(1 / fan_in) / 0.8796, cut at 2
            assert 0 < float(t.abs().max()) <= 2.0


# ---------------------------------------------------------------- replay
def _items(n, W, start=0):
    s = torch.zeros(n, 3, 64, 64, dtype=torch.uint8)
    s[:, 0, 0, 0] = torch.arange(start, start + n).to(torch.uint8)
    t = torch.arange(start, start + n, dtype=torch.float32).unsqueeze(1) + 0.01 * torch.arange(W)
    return s, torch.arange(start, start + n), t


def test_wide_target_replay_wraps_extends_and_samples():
    from impala_amd.dqn import PrioritizedReplay
    W = 8
    rb = PrioritizedReplay(8, device="cpu", seed=0, target_width=W)
    assert rb.target.shape == (8, W) and rb.target_width == W
    k = rb.extend(_items(6, W), priorities=torch.tensor([1., 2, 3, 4, 5, 0.5]))
    assert k.tolist() == [0, 1, 2, 3, 4, 5] and len(rb) == 6
    k = rb.extend(_items(4, W, start=6))  # wraps: slots 6, 7, 0, 1
    assert k.tolist() == [6, 7, 0, 1] and len(rb) == 8
    assert rb.target[:, 0].tolist() == [8., 9, 2, 3, 4, 5, 6, 7]
    assert torch.equal(rb.target[0], _items(1, W, start=8)[2][0])
    assert rb.priorities.tolist() == [5., 5, 3, 4, 5, 0.5, 5, 5]
    per_item = [(s.unsqueeze(0), a.reshape(1), t.unsqueeze(0)) for s, a, t in zip(*_items(2, W, start=20))]
    per_item[1] = tuple(x.squeeze(0) for x in per_item[1])  # target [W], no leading dim
    assert rb.extend(per_item).tolist() == [2, 3]
    assert rb.target[2:4, 0].tolist() == [20., 21.]
    keys, (s, a, t), probs = rb.sample(32)
    assert s.shape == (32, 3, 64, 64) and a.shape == (32,) and t.shape == (32, W) and probs.shape == (32,)
    assert torch.equal(t, rb.target[keys])
    with pytest.raises(ValueError):
        PrioritizedReplay(8, device="cpu", target_width=0)


def test_target_width_one_is_the_ring_of_today():
    from impala_amd.dqn import NativePrioritizedReplay, PrioritizedReplay
    a = PrioritizedReplay(8, device="cpu", seed=4)
    b = PrioritizedReplay(8, device="cpu", seed=4, target_width=1)
    for rb in (a, b):
        s, act, t = _items(6, 1)
        rb.extend((s, act, t[:, 0]), priorities=torch.tensor([1., 2, 3, 4, 5, 0.5]))
        rb.extend([(s[i], act[i], t[i, 0]) for i in range(3)])
    assert a.target.shape == b.target.shape == (8,)
    for x in ("s", "a", "target", "priorities"):
        assert torch.equal(getattr(a, x), getattr(b, x))
    ka, (_, _, ta), pa = a.sample(50)
    kb, (_, _, tb), pb = b.sample(50)
    assert torch.equal(ka, kb) and torch.equal(ta, tb) and torch.equal(pa, pb) and ta.shape == (50,)
    with pytest.raises(NotImplementedError, match="target_width"):
        NativePrioritizedReplay(8, device="cuda", target_width=8)


# ---------------------------------------------------------------- builder
def test_builder_surface():
    import impala_amd
    from impala_amd.config import load_config
    from impala_amd.dqn import ApexDQNBuilder, PrioritizedReplay
    from impala_amd.iqn import (ApexDistributionalActor, ApexDistributionalBuilder,
                                DistributionalAtariDQN)
    assert impala_amd.DistributionalAtariDQN is DistributionalAtariDQN
    assert impala_amd.ApexDistributionalBuilder is ApexDistributionalBuilder
    cfg = load_config(agent="apex")
    assert cfg.agent.n_tau_samples == 8
    cfg.distributed.train_device = cfg.distributed.infer_device = "cpu"
    cfg.agent.replay_buffer_size = 32
    b = ApexDistributionalBuilder(cfg)
    assert isinstance(b, ApexDQNBuilder)
    model = b.make_network()
    assert isinstance(model, DistributionalAtariDQN) and model.n_tau_samples == 8
    assert b._actor_model is model.downstream and b._actor_model is not model
    assert b._actor_model.n_tau_samples == 8
    rb = b.make_replay()
    assert isinstance(rb, PrioritizedReplay) and rb.target.shape == (32, 8) and rb.alpha == 0.6
    with pytest.raises(NotImplementedError):
        b.make_replay(native=True)
    actor = b.make_actor(model, rb)(0)
    assert isinstance(actor, ApexDistributionalActor) and actor._n_step == 3
    assert actor._rollout_length == cfg.agent.rollout_length
    assert float(actor._eps) == pytest.approx(0.4)
    assert float(b.make_actor(model, deterministic=True)(5)._eps) == pytest.approx(0.01)
    with pytest.raises(ValueError):
        b.make_actor(model, PrioritizedReplay(4, device="cpu", target_width=2))
    with pytest.raises(NotImplementedError, match="training step"):
        b.make_learner(model, rb)
    with pytest.raises(RuntimeError):  # act runs on the HIP path only
        model.act(torch.zeros(1, 3, 64, 64, dtype=torch.uint8), torch.tensor([0.4]))
