"""Host side of the Ape-X loop on the device (no GPU): the C boundary of
dqn_train_step_replay_rows, ApexActor against a fake model and a fake replay, and the builder's
make_actor."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from impala_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dqn_hip.h")
NAME = "dqn_train_step_replay_rows"
INVALID = 1001
FAKE = 0x1000  # a non-null pointer the entry may not look through before it has refused the call


# ---------------------------------------------------------------- the C boundary
def test_rows_entry_is_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert NAME in set(re.findall(r"\b(dqn_\w+)\s*\(", src))
    assert NAME in _lib.DQN_EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert NAME in set(re.findall(r"\b(dqn_\w+)\b", out))
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == list(lib.dqn_train_step_replay.argtypes)
    # additive: the ABI versions stay
    assert lib.dqn_abi_version() == 2 == _lib.DQN_ABI_VERSION
    assert "#define DQN_ABI_VERSION 2" in src
    assert lib.impala_abi_version() == 3


def test_rows_entry_refuses_null_handles_before_any_hip_call():
    lib = _lib.lib()
    for h, r in ((None, None), (None, FAKE)):
        assert lib.dqn_train_step_replay_rows(h, r, 1, 0, None, None, None) == INVALID
        assert "handle" in lib.dqn_last_error().decode()


# ---------------------------------------------------------------- ApexActor
class FakeModel:
    """act -> (action, q_pi, q_star) [1, 1] each, distinct per call; records (obs, eps)."""

    def __init__(self):
        self.calls = []

    def act(self, obs, eps):
        i = len(self.calls)
        self.calls.append((obs, eps))
        return (torch.tensor([[i % 6]]), torch.tensor([[0.5 + i]]), torch.tensor([[-0.25 - i]]))


class FakeReplay:
    def __init__(self):
        self.rollouts = []

    def extend_rollout(self, s, a, r, done, q_pi, q_star, n_step, gamma):
        self.rollouts.append(dict(s=s, a=a, r=r, done=done, q_pi=q_pi, q_star=q_star,
                                  n_step=n_step, gamma=gamma))


def _frame(i):
    return torch.full((3, 64, 64), i, dtype=torch.uint8)


def _drive(actor, steps, done_at=()):
    """observe_init, then `steps` act / observe pairs; -> the observed (obs id, a, r, done, q, v)."""
    seen = []
    ts = (_frame(0), 0.0, False, {})
    actor.observe_init(ts)
    for i in range(steps):
        action = actor.act(ts)
        nxt = (_frame(i + 1), float(i) / 4, i in done_at, {})
        actor.observe(action, nxt)
        seen.append((i, int(action[0]), nxt[1], nxt[2], float(action[1]["q"]), float(action[1]["v"])))
        ts = nxt
    return seen


def test_actor_hands_whole_rollouts_to_the_replay():
    from impala_amd.dqn import ApexActor
    from impala_amd.core import Actor
    model, rb = FakeModel(), FakeReplay()
    actor = ApexActor(model, rb, eps=0.3, n_step=5, rollout_length=5, gamma=0.97)
    assert isinstance(actor, Actor)
    seen = _drive(actor, 11, done_at=(3, 7))
    assert len(rb.rollouts) == 2
    for k, ro in enumerate(rb.rollouts):
        part = seen[5 * k:5 * k + 5]
        assert ro["s"].shape == (5, 3, 64, 64) and ro["s"].dtype == torch.uint8
        assert ro["s"][:, 0, 0, 0].tolist() == [p[0] for p in part]  # the frame acted on
        assert ro["a"].tolist() == [p[1] for p in part] and ro["a"].dtype == torch.int64
        assert ro["r"].tolist() == [p[2] for p in part] and ro["r"].dtype == torch.float32
        assert ro["done"].reshape(-1).tolist() == [p[3] for p in part]
        assert ro["q_pi"].tolist() == [p[4] for p in part]
        assert ro["q_star"].tolist() == [p[5] for p in part]
        assert all(ro[f].shape == (5,) for f in ("a", "r", "done", "q_pi", "q_star"))
        assert ro["n_step"] == 5 and ro["gamma"] == 0.97
    # one step is pending: a rollout of one step makes no transition, so update() keeps it
    assert len(actor._trajectory) == 1
    actor.update()
    assert len(rb.rollouts) == 2 and len(actor._trajectory) == 1
    # a second pending step: update() flushes the short rollout and clears the trajectory
    actor.observe(actor.act((_frame(50),)), (_frame(51), 1.0, False, {}))
    actor.update()
    assert len(rb.rollouts) == 3 and rb.rollouts[2]["s"].shape[0] == 2 and actor._trajectory == []


def test_act_passes_eps_and_names_q_and_v():
    from impala_amd.dqn import ApexActor
    model = FakeModel()
    actor = ApexActor(model, None, eps=0.125)
    obs = _frame(9)
    action, info = actor.act((obs,))
    assert set(info) == {"q", "v"} and float(info["q"]) == 0.5 and float(info["v"]) == -0.25
    assert int(action) == 0
    got_obs, got_eps = model.calls[0]
    assert got_obs is obs and float(got_eps) == 0.125 and got_eps.dtype == torch.float32


def test_actor_without_a_replay_never_touches_one():
    from impala_amd.dqn import ApexActor
    actor = ApexActor(FakeModel(), None, rollout_length=3)
    _drive(actor, 7)
    actor.update()
    assert actor._trajectory == [] and actor._last_transition is None


def test_async_twins():
    import asyncio
    from impala_amd.dqn import ApexActor
    rb = FakeReplay()
    actor = ApexActor(FakeModel(), rb, rollout_length=2)

    async def run():
        ts = (_frame(0), 0.0, False, {})
        await actor.async_observe_init(ts)
        for i in range(3):
            action = await actor.async_act(ts)
            ts = (_frame(i + 1), 1.0, False, {})
            await actor.async_observe(action, ts)
        await actor.async_update()

    asyncio.run(run())
    assert len(rb.rollouts) == 1 and len(actor._trajectory) == 1


# ---------------------------------------------------------------- builder
def _builder():
    from impala_amd.config import load_config
    from impala_amd.dqn import ApexDQNBuilder
    cfg = load_config(agent="apex")
    cfg.distributed.train_device = cfg.distributed.infer_device = "cpu"
    cfg.agent.replay_buffer_size = 32
    return cfg, ApexDQNBuilder(cfg)


def test_make_actor_returns_a_factory_with_the_configured_exploration():
    from impala_amd.dqn import ApexActor, ApexActorFactory, PrioritizedReplay
    cfg, b = _builder()
    assert cfg.agent.train_eps == 0.4 and cfg.training.num_rollouts > 1
    cfg.agent.n_step, cfg.agent.rollout_length = 4, 17
    model, rb = FakeModel(), FakeReplay()
    f = b.make_actor(model, rb)
    assert isinstance(f, ApexActorFactory)
    first, last = f(0), f(cfg.training.num_rollouts - 1)
    assert isinstance(first, ApexActor) and first._model is model and first._replay_buffer is rb
    assert float(first._eps) == pytest.approx(0.4, rel=1e-7)
    assert float(last._eps) == pytest.approx(0.4 ** 8, rel=1e-6)
    assert (first._n_step, first._rollout_length) == (4, 17)
    g = b.make_actor(model, rb, deterministic=True)
    assert {float(g(i)._eps) for i in (0, 3, cfg.training.num_rollouts - 1)} == {
        float(torch.tensor(cfg.agent.eval_eps, dtype=torch.float32))}
    # evaluation actors come without a replay
    e = b.make_actor(model, None, deterministic=True)(0)
    assert e._replay_buffer is None
    # the plain replay has no n-step ingest: still refused, and the message says why
    with pytest.raises(NotImplementedError, match="extend_rollout"):
        b.make_actor(model, PrioritizedReplay(8, device="cpu", seed=0))


def test_make_replay_in_place_needs_the_native_ring():
    _, b = _builder()
    with pytest.raises(ValueError, match="native"):
        b.make_replay(in_place=True)
    assert not hasattr(b.make_replay(), "in_place")
