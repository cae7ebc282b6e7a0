"""Ape-X DQN boundary and host logic on CPU: the oracle (tests/dqn_oracle.py) against the
reference's own fixtures, include/dqn_hip.h vs the binding vs the library's exports, argument
validation without a device, state_dict keys, PrioritizedReplay, the builder's config surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dqn_oracle as orc
from impala_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dqn_hip.h")
G = os.path.join(REPO, "tests", "golden")
KEYS = ("q", "target", "priorities", "loss", "grad_norm")


# ---------------------------------------------------------------- oracle vs reference
def test_oracle_head_matches_reference():
    d = np.load(os.path.join(G, "dqn_head.npz"))
    out = orc.loss_from_heads(d["adv"], d["v"], d["act"], d["target"], d["prob"], float(d["beta"]))
    np.testing.assert_allclose(out["metrics"], d["scalars"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(out["dadv"], d["dadv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["dv"], d["dv"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(out["priorities"], d["priorities"], rtol=1e-6, atol=1e-7)
    p = d["prob"]
    assert p.max() / p.min() > 50  # spread over about two decades


def test_oracle_train_steps_match_reference():
    """ApexLearner._train_step (agents/dqn/learning.py:159-191) restated, 3 steps."""
    d = orc.load_train_fixture()
    net = orc.make_net(d["params0"], 15)
    opt = orc.make_optimizer(net)
    for i in range(3):
        out = orc.train_step(net, opt, d[f"obs{i}"], d[f"act{i}"], d[f"tgt{i}"], d[f"prob{i}"])
        np.testing.assert_allclose([out[k] for k in KEYS], [d[k][i] for k in KEYS], rtol=1e-5,
                                   atol=1e-7, err_msg=f"step {i}")
        np.testing.assert_allclose(out["prio"], d[f"prio{i}"], rtol=1e-5, atol=1e-7)
        if i == 0:
            np.testing.assert_allclose(out["grads"], d["grads1"], rtol=1e-4, atol=1e-8)
            np.testing.assert_allclose(orc.flat_params(net), d["params1"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(orc.flat_params(net), d["params3"], rtol=0, atol=1e-7)


def test_oracle_forward_and_pi_match_reference():
    from impala_amd.dqn import net_specs
    d = np.load(os.path.join(G, "dqn_act.npz"))
    online = orc.load_train_fixture()["params0"]
    rng = np.random.default_rng(int(d["target_delta_seed"]))
    delta = np.concatenate([(0.01 * rng.standard_normal(s)).astype(np.float32).reshape(-1)
                            for _, s in net_specs(15)])
    obs = torch.from_numpy(rng.integers(0, 256, size=(128, 3, 64, 64), dtype=np.uint8))
    with torch.no_grad():
        q_on = orc.make_net(online)(obs).numpy()
        q_tg = orc.make_net(online + delta)(obs).numpy()
    np.testing.assert_allclose(q_on, d["q_online"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(q_tg, d["q_target"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(q_on.argmax(-1), d["greedy"])
    pi = orc.act_pi(q_on, 0.4)
    np.testing.assert_allclose(pi.sum(-1), 1.0, atol=1e-12)
    assert np.allclose(pi[np.arange(128), d["greedy"]], 0.6) and np.isclose(pi.min(), 0.4 / 14)


# ---------------------------------------------------------------- C boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dqn_\w+)\s*\(", src)))


def test_header_declares_what_the_binding_expects():
    assert _declared() == sorted(_lib.DQN_EXPORTS)


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\b(dqn_\w+)\b", out))
    for name in _declared():
        assert name in exported, name
        assert hasattr(lib, name)
    assert lib.dqn_abi_version() == _lib.DQN_ABI_VERSION


def test_struct_layouts_match_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct dqn_config \{(.*?)\} dqn_config;", src, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [f for f, _ in _lib.DqnConfig._fields_]
    body = re.search(r"typedef struct dqn_batch \{(.*?)\} dqn_batch;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in _lib.DqnBatch._fields_]


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "hdr.c"
    src.write_text('#include "dqn_hip.h"\n'
                   "int main(void) { dqn_config c; c.batch_size = DQN_NUM_METRICS; return c.batch_size == 9 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c",
                        str(src), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_param_count_and_defaults():
    from impala_amd import dqn
    lib = _lib.lib()
    assert lib.dqn_param_count(15) == 610992 == dqn.param_count(15)
    for A in (1, 6):
        assert lib.dqn_param_count(A) == dqn.param_count(A)
    cfg = dqn.default_config()
    assert (cfg.batch_size, cfg.num_actions, cfg.dtype) == (512, 15, 0)
    assert cfg.lr == pytest.approx(6.25e-5) and cfg.adam_eps == pytest.approx(1e-4)
    assert cfg.max_grad_norm == 40.0 and cfg.importance_sampling_exponent == pytest.approx(0.4)


@pytest.mark.parametrize("field,value", [("batch_size", 0), ("num_actions", 0), ("num_actions", 16),
                                         ("dtype", 7)])
def test_create_rejects_bad_config_without_touching_the_device(field, value):
    from impala_amd import dqn
    lib = _lib.lib()
    cfg = dqn.default_config()
    setattr(cfg, field, value)
    h = _lib._P()
    status = lib.dqn_create(C.byref(cfg), 0, C.byref(h))
    assert status in (1001, 1003) and not h.value
    assert lib.dqn_last_error()


def test_entry_points_validate_before_launch():
    lib = _lib.lib()
    assert lib.dqn_train_step(None, None, None) == 1001
    assert lib.dqn_forward(None, None, 1, 0, None, None) == 1001
    assert lib.dqn_forward(None, None, 1, 2, None, None) == 1001
    assert lib.dqn_act(None, None, 1, None, 0.0, 0, 0, None, None, None, None, None) == 1001
    assert lib.dqn_loss_head(None, None, None, None, None, 4, 15, 0.4, None, None, None, None, None) == 1001
    assert lib.dqn_destroy(None) == 0


# ---------------------------------------------------------------- model
def test_state_dict_keys_and_shapes_match_reference():
    from impala_amd.dqn import AtariDQNModel
    d = np.load(os.path.join(G, "dqn_train_step.npz"))
    m = AtariDQNModel((3, 64, 64), 15, device="cpu", seed=0)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in d["state_dict_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in d["state_dict_shapes"]]
    assert all(p.requires_grad for p in m.online_net.parameters())
    assert not any(p.requires_grad for p in m.target_net.parameters())
    assert torch.equal(m.flat, m.target_flat)
    # the parameters are views of the flat buffers; load_state_dict writes through them
    m2 = AtariDQNModel((3, 64, 64), 15, device="cpu", seed=1)
    m2.load_state_dict(sd)
    assert torch.equal(m2.flat, m.flat) and torch.equal(m2.target_flat, m.target_flat)
    with pytest.raises(RuntimeError):
        m.forward(torch.zeros(1, 3, 64, 64, dtype=torch.uint8))


def test_model_pickles_and_clones(tmp_path):
    from impala_amd.dqn import AtariDQNModel
    m = AtariDQNModel((3, 64, 64), 6, device="cpu", seed=3)
    m.target_flat.add_(1.0)
    torch.save(m, tmp_path / "m.pt")
    m2 = torch.load(tmp_path / "m.pt", weights_only=False)
    assert torch.equal(m2.flat, m.flat) and torch.equal(m2.target_flat, m.target_flat)
    m2.flat[0] = 7.0  # still views after unpickling
    assert float(m2.get_parameter("online_net.body.body.0.weight").detach().reshape(-1)[0]) == 7.0
    c = m.clone_to("cpu")
    assert torch.equal(c.flat, m.flat) and not any(p.requires_grad for p in c.parameters())
    m.sync_target_net()
    assert torch.equal(m.target_flat, m.flat)


# ---------------------------------------------------------------- replay
def _items(n, start=0):
    s = torch.zeros(n, 3, 64, 64, dtype=torch.uint8)
    s[:, 0, 0, 0] = torch.arange(start, start + n).to(torch.uint8)
    return s, torch.arange(start, start + n), torch.arange(start, start + n, dtype=torch.float32)


def test_replay_ring_wraps_and_new_items_get_max_priority():
    from impala_amd.dqn import PrioritizedReplay
    rb = PrioritizedReplay(8, device="cpu", seed=0)
    k = rb.extend(_items(6), priorities=torch.tensor([1., 2, 3, 4, 5, 0.5]))
    assert k.tolist() == [0, 1, 2, 3, 4, 5] and len(rb) == 6
    k = rb.extend(_items(4, start=6))  # wraps: slots 6, 7, 0, 1
    assert k.tolist() == [6, 7, 0, 1] and len(rb) == 8
    assert rb.target.tolist() == [8., 9, 2, 3, 4, 5, 6, 7]
    assert rb.s[0, 0, 0, 0] == 8 and rb.a[1] == 9
    assert rb.priorities.tolist() == [5., 5, 3, 4, 5, 0.5, 5, 5]  # no priority: the current max
    per_item = [(s.unsqueeze(0), a.reshape(1), t.reshape(1)) for s, a, t in zip(*_items(2, start=20))]
    assert rb.extend(per_item).tolist() == [2, 3]
    assert rb.target[2:4].tolist() == [20., 21.]


def test_replay_sample_frequencies_follow_priorities():
    """Frequencies of 40000 draws (seed fixed) against p^alpha / sum p^alpha: chi-square with
    15 degrees of freedom against its critical value at p = 1e-6 (confirmed on the CPU: the
    statistic is far below it)."""
    from scipy.stats import chi2
    from impala_amd.dqn import PrioritizedReplay
    rb = PrioritizedReplay(16, priority_exponent=0.6, device="cpu", seed=5)
    pri = torch.tensor(np.random.default_rng(0).uniform(0.05, 4.0, 16).astype(np.float32))
    rb.extend(_items(16), priorities=pri)
    expect = (pri.double() ** 0.6 / (pri.double() ** 0.6).sum()).numpy()
    np.testing.assert_allclose(rb.probabilities().numpy(), expect, rtol=1e-6)
    n = 40000
    keys, (s, a, t), probs = rb.sample(n)
    assert s.shape == (n, 3, 64, 64) and torch.equal(a, keys) and torch.equal(t, keys.float())
    np.testing.assert_allclose(probs.numpy(), expect[keys.numpy()], rtol=1e-6)
    counts = np.bincount(keys.numpy(), minlength=16)
    stat = float(((counts - n * expect) ** 2 / (n * expect)).sum())
    print("replay chi2 (15 dof)", stat, "critical", chi2.isf(1e-6, 15))
    assert stat < chi2.isf(1e-6, 15)
    # the returned probabilities give the weights the oracle expects, whatever their scale
    w = orc.weights(probs[:64], 0.4, probs[:64])
    w_raw = orc.weights(probs[:64] * 123.0, 0.4, probs[:64])
    np.testing.assert_allclose(w.numpy(), w_raw.numpy(), rtol=1e-5)
    ref = (expect[keys[:64].numpy()] ** -0.4)
    np.testing.assert_allclose(w.numpy(), ref / ref.max(), rtol=1e-5)
    # seeded reset: the same draws again
    rb.reset(5)
    assert torch.equal(rb.sample(100)[0], keys[:100])


def test_replay_update_changes_later_draws():
    from impala_amd.dqn import PrioritizedReplay
    rb = PrioritizedReplay(8, device="cpu", seed=1)
    rb.extend(_items(8), priorities=torch.ones(8))
    before = np.bincount(rb.sample(4000)[0].numpy(), minlength=8)
    assert before.min() > 300
    rb.update(torch.tensor([3]), torch.tensor([1e4]))
    rb.async_update(torch.tensor([0, 1]), torch.tensor([1e-6, 1e-6]))
    after = np.bincount(rb.sample(4000)[0].numpy(), minlength=8)
    assert after[3] > 3800 and after[0] + after[1] == 0
    k = rb.extend(_items(1, start=50))  # new items: the running maximum
    assert float(rb.priorities[k[0]]) == 1e4


def test_replay_extend_takes_item_lists_and_columns_alike():
    """The per-item list form (items with and without a leading dim) and the column form go
    through the same ``_replay_columns`` and leave the same ring, keys and priorities."""
    from impala_amd.dqn import PrioritizedReplay
    cols = _items(5, start=3)
    items = [(s.unsqueeze(0), a.reshape(1), t.reshape(1)) for s, a, t in zip(*cols)]
    items[1] = tuple(x.squeeze(0) for x in items[1])  # s [3,64,64], a and target 0-d
    pri = torch.tensor([1., 2, 3, 4, 5])
    rings = []
    for pick in (lambda lo, hi: tuple(x[lo:hi] for x in cols), lambda lo, hi: items[lo:hi]):
        rb = PrioritizedReplay(4, device="cpu", seed=0)
        keys = [rb.extend(_items(2)), rb.extend(pick(0, 3), priorities=pri[:3]),
                rb.extend(pick(3, 5))]  # wraps; the last two take the running maximum
        rings.append((keys, rb.s, rb.a, rb.target, rb.priorities, len(rb), rb.size, rb._cursor))
    for x, y in zip(*rings):
        if isinstance(x, list):
            assert [k.tolist() for k in x] == [k.tolist() for k in y] == [[0, 1], [2, 3, 0], [1, 2]]
        elif isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
        else:
            assert x == y
    assert rings[0][3].tolist() == [5., 6., 7., 4.] and rings[0][5:] == (4, 4, 3)
    assert rings[0][4].tolist() == [3., 3., 3., 2.]  # no priority: the running maximum


def test_native_replay_shares_the_base_constructor():
    from impala_amd.dqn import NativePrioritizedReplay, PrioritizedReplay
    mro = NativePrioritizedReplay.__mro__
    assert mro.index(PrioritizedReplay) < mro.index(_lib.NativeHandle)
    assert "_alloc_ring" not in vars(NativePrioritizedReplay)  # the ring is the base's
    assert NativePrioritizedReplay._size is PrioritizedReplay._size  # one accessor, _state()
    calls = []
    orig = PrioritizedReplay._alloc_ring
    PrioritizedReplay._alloc_ring = lambda self, shape: calls.append(shape)
    try:
        with pytest.raises(RuntimeError, match="HIP path only"):
            NativePrioritizedReplay(2, device="cpu")
    finally:
        PrioritizedReplay._alloc_ring = orig
    assert calls == []  # refused by the subclass before any allocation


def test_native_replay_runs_the_base_constructor(monkeypatch):
    """The whole constructor path without a GPU: the create entry point and the allocations are
    stubbed, so ``__init__`` runs handle creation, then ``PrioritizedReplay.__init__`` (fields,
    ring, ``reset``), and ends in the library's own refusal of ``dqn_replay_bind`` on the null
    handle the stub left."""
    from impala_amd.dqn import OBS_SHAPE, NativePrioritizedReplay, PrioritizedReplay
    log = []

    def alloc(self, shape):
        log.append(("alloc", tuple(shape), self.capacity, self.alpha, str(self.device)))
        self.s = self.a = self.target = self.priorities = None

    monkeypatch.setattr(_lib.NativeHandle, "_open", lambda self, *a: log.append(("open",) + a))
    monkeypatch.setattr(PrioritizedReplay, "_alloc_ring", alloc)
    monkeypatch.setattr(NativePrioritizedReplay, "_stream", lambda self: 0)
    rb = NativePrioritizedReplay.__new__(NativePrioritizedReplay)
    with pytest.raises(RuntimeError, match=r"dqn_replay_bind failed \(status 1001\)"):
        rb.__init__(6, priority_exponent=0.5, device="cuda:1", seed=9)
    assert log == [("open", "dqn_replay_create", 6, 0.5, 1), ("alloc", OBS_SHAPE, 6, 0.5, "cuda:1")]
    assert (rb._seed, rb._counter) == (9, 0)  # the base constructor's reset(seed), overridden
    assert not hasattr(rb, "_gen")  # the sampler state stays the library's


# ---------------------------------------------------------------- builder
def test_builder_config_surface():
    from impala_amd.config import load_config
    from impala_amd.dqn import ApexDQNBuilder, ConstantEpsFunc, FlexibleEpsFunc, PrioritizedReplay
    cfg = load_config(agent="apex")
    assert cfg.agent.name == "apex" and cfg.agent.batch_size == 512
    cfg.distributed.train_device = cfg.distributed.infer_device = "cpu"
    cfg.agent.replay_buffer_size = 32
    b = ApexDQNBuilder(cfg)
    model = b.make_network()
    assert b._actor_model is model.downstream and b._actor_model is not model
    rb = b.make_replay()
    assert isinstance(rb, PrioritizedReplay) and rb.capacity == 32 and rb.alpha == 0.6
    kw = b.learner_kwargs()
    assert kw["optimizer"].lr == 6.25e-5 and kw["optimizer"].eps == 1e-4
    assert kw["learning_starts"] == cfg.agent.learning_starts  # (the deploy overlay's value)
    with pytest.raises(NotImplementedError):
        b.make_actor(model, rb)
    with pytest.raises(RuntimeError):  # the learner runs on the HIP path only
        b.make_learner(model, rb)
    assert ConstantEpsFunc(0.01)(3) == 0.01
    f = FlexibleEpsFunc(0.4, 8)
    assert f(0) == 0.4 and f(7) == pytest.approx(0.4 ** 8.0) and FlexibleEpsFunc(0.4, 1)(0) == 0.4
