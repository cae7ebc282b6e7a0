"""PPO ingest on the CPU: the fp32 restatement of the actor's lambda-return targets
(tests/ppo_rollout_oracle.py) against a float64 transcription of rlax's scan, the torch-CPU
fallback of ``PPOActor`` against that restatement bit for bit, the actor and the builder over a
host replay, and the C boundary (arguments refused before any HIP call)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ppo_rollout_oracle as orc
from impala_amd import _lib

INVALID = 1001
FAKE = 0x1000  # a non-null pointer no entry may look through before it has refused the call
SCALES = (0.1, 1.0, 10.0)
DONE_RATES = (0.0, 0.05, 0.5, 1.0)
GAMMAS = (0.0, 0.99, 1.0)
LAMBDAS = (0.0, 0.95, 1.0)


def _err():
    return _lib.lib().impala_last_error().decode()


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("L", [2, 3, 17, 65, 129])
def test_fp32_restatement_within_the_derived_bound_of_float64(L):
    """|fp32 - float64| <= 6 * 2^-24 * (K - t) * M_t (oracle.error_bound) on every element, for
    every scale x done rate x gamma x lambda.  (Measured on the CPU over 4000 such draws: the
    largest error is 0.30 of the bound.)"""
    rng = np.random.default_rng(100 + L)
    worst = 0.0
    for scale, rate, gamma, lam in itertools.product(SCALES, DONE_RATES, GAMMAS, LAMBDAS):
        r, done, v = orc.draw(rng, L, scale, rate)
        got = orc.lambda_returns_f32(r, done, v, gamma, lam).astype(np.float64)
        ref = orc.reference_f64(r, done, v, gamma, lam)
        bound = orc.error_bound(r, done, v, gamma, lam)
        err = np.abs(got - ref)
        assert got.shape == ref.shape == (L - 1,)
        assert np.all(err <= bound), (scale, rate, gamma, lam, float((err - bound).max()))
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    print(f"L={L}: largest error / bound = {worst:.3f}")


def test_restatement_known_values():
    # L = 3, gamma = 0.5, lambda = 0.5: t1 = r1 + .5 (.5 v2 + .5 v2) = r1 + .5 v2
    r, v = np.array([1.0, 2.0, 99.0]), np.array([7.0, 10.0, 20.0])
    t = orc.lambda_returns_f32(r, np.zeros(3), v, 0.5, 0.5)
    np.testing.assert_array_equal(t, np.float32([1 + .5 * (.5 * 10 + .5 * 12), 2 + .5 * 20]))
    # lambda = 0: one-step targets r + gamma v'; lambda = 1: the discounted return
    np.testing.assert_array_equal(orc.lambda_returns_f32(r, np.zeros(3), v, 0.5, 0.0),
                                  np.float32([1 + 5, 2 + 10]))
    np.testing.assert_array_equal(orc.lambda_returns_f32(r, np.zeros(3), v, 0.5, 1.0),
                                  np.float32([1 + .5 * (2 + 10), 2 + 10]))
    # a done at step 0 cuts its bootstrap; the last step's done is never read
    np.testing.assert_array_equal(orc.lambda_returns_f32(r, np.array([1, 0, 1]), v, 0.5, 0.5),
                                  np.float32([1.0, 12.0]))


@pytest.mark.parametrize("L", [2, 3, 17, 129])
def test_host_fallback_equals_the_restatement_bitwise(L):
    from impala_amd.ppo import lambda_returns
    rng = np.random.default_rng(7 * L)
    for scale, rate, gamma, lam in itertools.product((0.1, 10.0), DONE_RATES, GAMMAS, LAMBDAS):
        r, done, v = orc.draw(rng, L, scale, rate)
        got = lambda_returns(torch.from_numpy(r).reshape(L, 1), torch.from_numpy(done),
                             torch.from_numpy(v).reshape(L, 1), gamma, lam)
        exp = orc.lambda_returns_f32(r, done, v, gamma, lam)
        assert got.dtype == torch.float32 and got.shape == (L - 1,)
        assert np.array_equal(got.numpy().view(np.uint32), exp.view(np.uint32)), (scale, rate, gamma, lam)
    with pytest.raises(ValueError):
        lambda_returns(torch.zeros(1), torch.zeros(1), torch.zeros(1), 0.99, 0.95)


# ---------------------------------------------------------------- actor and builder, host replay
class _FakeModel:
    """act -> (action, logits, value) derived from the frame, as AtariPPOModel.act returns."""
    A = 6

    def act(self, obs, deterministic):
        x = torch.as_tensor(obs).float().mean()
        logits = torch.arange(self.A, dtype=torch.float32).reshape(1, self.A) * 0.1 + x / 255
        return (torch.tensor([[int(x) % self.A]]), logits, (x / 100).reshape(1, 1))


def _stream(n, seed):
    rng = np.random.default_rng(seed)
    return [(torch.from_numpy(rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)),
             float(rng.standard_normal()), bool(rng.random() < 0.2)) for _ in range(n)]


def test_actor_fills_a_host_replay_with_the_reference_items():
    from impala_amd.ppo import PPOActor
    from impala_amd.replay import ReplayBuffer
    L = 5
    rb = ReplayBuffer(64, seed=0)
    actor = PPOActor(_FakeModel(), rb, rollout_length=L)
    assert (actor._gamma, actor._lambda) == (0.99, 0.95)
    assert PPOActor(_FakeModel(), rb)._rollout_length == 128
    steps = _stream(2 * L + 1, seed=3)
    actor.observe_init(steps[0])
    rec = []
    for i in range(2 * L):
        action = actor.act(steps[i])
        rec.append((steps[i][0], action[0], steps[i + 1][1], steps[i + 1][2], action[1]["logpi"],
                    action[1]["v"]))
        actor.observe(action, steps[i + 1])
    assert len(rb) == 2 * (L - 1)  # two rollouts of L steps, L - 1 transitions each
    slot = 0
    for k in range(2):
        part = rec[k * L:(k + 1) * L]
        tgt = orc.lambda_returns_f32([p[2] for p in part], [p[3] for p in part],
                                     [float(p[5]) for p in part], 0.99, 0.95)
        for t in range(L - 1):
            s, a, target, pi = rb._data[slot]
            assert s.shape == (1, 3, 64, 64) and torch.equal(s[0], part[t][0])
            assert a.dtype == torch.int64 and int(a) == int(part[t][1])
            assert target.dtype == torch.float32 and target.numpy().view(np.uint32)[0] == \
                tgt[t:t + 1].view(np.uint32)[0]
            assert torch.equal(pi, part[t][4].reshape(1, -1))
            slot += 1
    actor.update()  # an empty trajectory: nothing to add
    assert len(rb) == 2 * (L - 1)
    assert PPOActor(_FakeModel(), None).observe(None, None) is None  # no replay: a pure policy


def test_builder_makes_actors_and_a_host_replay_without_a_device():
    from impala_amd.builder import PPOBuilder
    from impala_amd.config import load_config
    from impala_amd.ppo import PPOActor
    from impala_amd.replay import ReplayBuffer
    cfg = load_config(agent="ppo")
    cfg.distributed.train_device = cfg.distributed.infer_device = "cpu"
    cfg.agent.replay_buffer_size = 32
    cfg.learner = {"replay": "host"}
    b = PPOBuilder(cfg)
    rb = b.make_replay()
    assert type(rb) is ReplayBuffer and rb.capacity == 32
    factory = b.make_actor(_FakeModel(), rb, deterministic=True)
    actor = factory(0)
    assert isinstance(actor, PPOActor) and actor._replay_buffer is rb
    assert not bool(actor._deterministic_policy)  # `deterministic` is ignored, as in the reference
    assert (actor._gamma, actor._lambda, actor._rollout_length) == (0.99, 0.95, 128)


# ---------------------------------------------------------------- boundary
def _ring(cap=16, A=15, **null):
    f = {k: (None if null.get(k) else FAKE) for k in ("obs", "actions", "targets", "behaviour_logits")}
    return _lib.ImpalaPpoRing(f["obs"], f["actions"], f["targets"], f["behaviour_logits"], cap, A)


def _extend(ring=None, cursor=0, ptrs=(FAKE,) * 6, L=9, gamma=0.99, lam=0.95):
    ring = _ring() if ring is None else ring
    return _lib.lib().impala_ppo_extend_rollout(C.byref(ring), cursor, *ptrs, L, gamma, lam, None)


def test_new_entries_are_bound_and_the_abi_numbers_stay():
    lib = _lib.lib()
    for name in ("impala_ppo_extend_rollout", "impala_ppo_train_step_rows"):
        assert name in _lib.EXPORTS and getattr(lib, name).restype is C.c_int
    assert lib.impala_abi_version() == 3 == _lib.ABI_VERSION and _lib.DQN_ABI_VERSION == 2


def test_extend_rollout_refuses_bad_arguments_before_any_launch():
    """Every pointer here is null or fake, so a call that got past its checks would fault."""
    lib = _lib.lib()
    assert lib.impala_ppo_extend_rollout(None, 0, *(FAKE,) * 6, 9, 0.99, 0.95, None) == INVALID
    assert "null pointer" in _err()
    for k in ("obs", "actions", "targets", "behaviour_logits"):
        assert _extend(_ring(**{k: True})) == INVALID and "null pointer" in _err(), k
    for i in range(6):
        ptrs = tuple(None if j == i else FAKE for j in range(6))
        assert _extend(ptrs=ptrs) == INVALID and "null pointer" in _err(), i
    for L in (1, 0, -4, 1026):
        assert _extend(_ring(cap=4096), L=L) == INVALID and "L must be in [2, 1025]" in _err(), L
    assert _extend(_ring(cap=7), L=9) == INVALID and "capacity" in _err()  # K = 8 > 7
    assert _extend(_ring(cap=0), L=2) == INVALID and "capacity" in _err()
    for lam in (1.5, -0.1, float("nan")):
        assert _extend(lam=lam) == INVALID and "lambda" in _err(), lam
    for gamma in (1.01, -1.0, float("nan")):
        assert _extend(gamma=gamma) == INVALID and "gamma" in _err(), gamma
    for A in (0, 16):
        assert _extend(_ring(A=A)) == INVALID and "num_actions" in _err(), A
    for cursor in (-1, 16):
        assert _extend(cursor=cursor) == INVALID and "cursor" in _err(), cursor


def test_train_step_rows_refuses_bad_arguments_before_the_handle_is_looked_at():
    """Null pointers, n and the row range need no handle and are checked first; with those
    valid, the null handle is what refuses the call."""
    lib = _lib.lib()
    ring = _lib.ImpalaPpoBatch(FAKE, FAKE, FAKE, FAKE)
    rows = np.arange(8, dtype=np.int64)

    def call(ring_=ring, rows_=rows, n=8, cap=16):
        return lib.impala_ppo_train_step_rows(None, C.byref(ring_) if ring_ is not None else None,
                                              rows_.ctypes.data if rows_ is not None else None,
                                              n, cap, None)
    assert call(ring_=None) == INVALID and "null argument" in _err()
    assert call(rows_=None) == INVALID and "null argument" in _err()
    for n in (0, -1, 257):
        assert call(n=n) == INVALID and "n must equal batch_size" in _err(), n
    assert call(cap=0) == INVALID and "capacity" in _err()
    for bad in (16, -1, 1 << 40):
        r = rows.copy()
        r[5] = bad
        assert call(rows_=r) == INVALID and "row index out of range" in _err(), bad
    assert call() == INVALID and "null handle" in _err()
    # the IMPALA entry shares the checks
    b = _lib.ImpalaBatch(FAKE, FAKE, FAKE, FAKE, FAKE)
    r = rows.copy()
    r[0] = 16
    assert lib.impala_train_step_rows(None, C.byref(b), r.ctypes.data, 8, 16, None) == INVALID
    assert "impala_train_step_rows: row index out of range" in _err()
