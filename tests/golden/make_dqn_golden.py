"""Generate the Ape-X DQN golden fixtures in tests/golden/ FROM THE REFERENCE ITSELF.  Runs only
where a checkout of the reference is present (``make_golden.REF``), never in the test suite:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dqn_golden.py

The reference is imported read-only with make_golden.py's import-boundary stubs;
``AtariDQNModel`` (models/distributed_models.py:72-104) and ``ApexLearner``
(agents/dqn/learning.py:97-191) are the reference's own code.  Data only (float32 unless stated):

* ``dqn_head.npz``        N=256, A=15: random adv / v / targets / actions, probabilities spread
  over two decades, through the reference's own ``DuelingHead.forward`` and
  ``ApexLearner._train_step`` (a no-op optimizer, so the raw gradients stay); the 4
  metrics (q, target, priorities, loss), d loss / d adv, d loss / d v, the priorities.
* ``dqn_train_step.npz`` + ``dqn_train_step_vec{0..11}.npz``  ApexLearner with Adam(6.25e-5, eps
  1e-4) on the seed-0 model, three ``train_step`` calls on three N=16 batches with
  prioritised-style probabilities through a fake replay that records ``async_update``: the 5
  metrics and the priorities of each step, the state_dict key list, and (the long vectors, cut
  into equal chunks so that no file passes 1 MiB) the initial flat online params, the post-clip
  grads of step 1, captured before zero_grad, and the flat online params after steps 1 and 3.
  ``impala_amd.dqn.AtariDQNModel(seed=0)`` restates the seed-0 init bit for bit on the machine
  that runs this script (checked here; trunc_normal_ is not bit-portable across CPUs).
* ``dqn_act.npz``         q_online / q_target of 128 frames and the greedy action, on the same
  seed-0 model with the target net nudged (deltas and frames from the seeds it stores).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (stubs, flat helpers)

METRICS = ("train_step/q", "train_step/target", "train_step/priorities", "train_step/loss",
           "train_step/grad_norm")
VEC_FILES = 12


def _import_reference():
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    import models.distributed_models as dm  # noqa: E402  (reference)
    import agents.dqn.learning as dl  # noqa: E402  (reference)
    return dm, dl


class _Future:
    def wait(self):
        pass


class _RecordingReplay:
    """sample -> (keys, batch, probabilities); async_update records (keys, priorities)."""

    def __init__(self, batches):
        self.batches = list(batches)
        self.updates = []

    def warm_up(self, n):
        pass

    def sample(self, b):
        keys, batch, probs = self.batches.pop(0)
        return keys, batch, probs

    def async_update(self, keys, priorities):
        self.updates.append((keys, priorities.numpy().copy()))
        return _Future()


class _GradSnapAdam(torch.optim.Adam):
    """Adam that records the (post-clip) grads it is stepped with (the online net's: the target
    net's parameters have none)."""
    snaps: list

    def step(self, closure=None):
        self.snaps.append(torch.cat([p.grad.detach().reshape(-1) for g in self.param_groups
                                     for p in g["params"] if p.grad is not None]).numpy().copy())
        return super().step(closure)


class _Model:
    """What ApexLearner needs of rlmeta's model wrapper around the reference AtariDQNModel."""

    def __init__(self, m):
        self.m = m

    def __call__(self, x):
        return self.m.forward(x)

    def parameters(self):
        return self.m.parameters()

    def push(self):
        pass

    def sync_target_net(self):
        self.m.sync_target_net()


class _NoOptimizer:
    """ApexLearner's optimizer calls, doing nothing: the head fixture keeps the raw gradients."""

    def zero_grad(self):
        pass

    def step(self):
        pass


def gen_head(out, dm, dl):
    """The reference's own ``ApexLearner._train_step`` on given head outputs: the model handed to
    it is the reference ``DuelingHead`` with its three sub-modules replaced by constants (identity
    body, adv and v leaves), so q is the reference's dueling combination and the gradients of the
    reference's loss arrive in ``adv.grad`` / ``v.grad``.  The learner's only parameter is a dummy
    with a zero gradient, so its clip_grad_norm_ touches nothing."""
    import models.models as mm  # noqa: E402  (reference)
    rng = np.random.default_rng(23)
    N, A, beta = 256, 15, 0.4
    adv = (1.5 * rng.standard_normal((N, A))).astype(np.float32)
    v = rng.standard_normal((N, 1)).astype(np.float32)
    act = rng.integers(0, A, size=(N,), dtype=np.int64)
    tgt = (2.0 * rng.standard_normal(N)).astype(np.float32)
    prob = (10.0 ** rng.uniform(-4, -2, N)).astype(np.float32)
    a_t, v_t = torch.tensor(adv, requires_grad=True), torch.tensor(v, requires_grad=True)

    class _GivenHead(mm.DuelingHead):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.body = lambda x: x
            self.q = lambda h: a_t
            self.v = lambda h: v_t
            self.dummy = torch.nn.Parameter(torch.zeros(1))
            self.dummy.grad = torch.zeros(1)

    head = _GivenHead()
    rb = _RecordingReplay([])
    learner = dl.ApexLearner(head, rb, _NoOptimizer(), batch_size=N, importance_sampling_exponent=beta)
    keys = torch.arange(N)
    m = learner._train_step(keys, [torch.zeros(N, 1), torch.from_numpy(act), torch.from_numpy(tgt)],
                            torch.from_numpy(prob))
    assert float(m["train_step/grad_norm"]) == 0.0 and len(rb.updates) == 1
    np.savez_compressed(os.path.join(out, "dqn_head.npz"), adv=adv, v=v.reshape(-1), act=act,
                        target=tgt, prob=prob, beta=np.float32(beta),
                        scalars=np.array([m[k] for k in METRICS[:4]], np.float32),
                        dadv=a_t.grad.numpy(), dv=v_t.grad.numpy().reshape(-1), priorities=rb.updates[0][1])


def _batch(N, A, seed):
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 256, size=(N, 3, 64, 64), dtype=np.uint8)
    act = rng.integers(0, A, size=(N,), dtype=np.int64)
    tgt = rng.standard_normal(N).astype(np.float32)
    pri = rng.uniform(0.05, 3.0, 4 * N) ** 0.6  # prioritised-style: p^alpha / sum over a larger ring
    prob = (pri[:N] / pri.sum()).astype(np.float32)
    keys = rng.integers(0, 1000, size=(N,), dtype=np.int64)
    return keys, obs, act, tgt, prob


def gen_train_step(out, dm, dl):
    A, N = 15, 16
    torch.manual_seed(0)
    model = dm.AtariDQNModel((3, 64, 64), A)
    online = list(model.online_net.parameters())
    params0 = mg._flat(online)
    from impala_amd.dqn import AtariDQNModel  # the init restatement must be the reference's
    ours = AtariDQNModel((3, 64, 64), A, device="cpu", seed=0)
    assert np.array_equal(ours.flat.numpy(), params0), "seed-0 init differs from the reference's"
    assert [k for k, _ in ours.state_dict().items()] == list(model.state_dict().keys())
    batches = [_batch(N, A, 3030 + i) for i in range(3)]
    opt = _GradSnapAdam(model.parameters(), lr=6.25e-5, eps=1e-4)  # agents/dqn/builder.py:100-101
    opt.snaps = []
    rb = _RecordingReplay([(torch.from_numpy(k), [torch.from_numpy(o), torch.from_numpy(a),
                                                   torch.from_numpy(t)], torch.from_numpy(p))
                           for k, o, a, t, p in batches])
    learner = dl.ApexLearner(_Model(model), rb, opt, batch_size=N)
    res = {k.split("/")[1]: [] for k in METRICS}
    vec = []
    for i in range(3):
        m = learner.train_step()
        for k in METRICS:
            res[k.split("/")[1]].append(float(m[k]))
        if i == 0:
            vec = [params0, opt.snaps[0][:params0.size], mg._flat(online)]
    vec.append(mg._flat(online))
    arrays = {}
    for i, (k, o, a, t, p) in enumerate(batches):
        arrays[f"keys{i}"], arrays[f"obs{i}"], arrays[f"act{i}"], arrays[f"tgt{i}"], arrays[f"prob{i}"] = k, o, a, t, p
        assert np.array_equal(rb.updates[i][0].numpy(), k)
        arrays[f"prio{i}"] = rb.updates[i][1]
    np.savez_compressed(os.path.join(out, "dqn_train_step.npz"), n_params=np.int64(params0.size),
                        state_dict_keys=np.array(list(model.state_dict().keys())),
                        state_dict_shapes=np.array([",".join(map(str, v.shape)) for v in model.state_dict().values()]),
                        **arrays, **{k: np.asarray(v, dtype=np.float32) for k, v in res.items()})
    long = np.concatenate(vec).astype(np.float32)
    assert long.size == 4 * params0.size and long.size % VEC_FILES == 0
    for i, x in enumerate(np.split(long, VEC_FILES)):
        np.savez_compressed(os.path.join(out, f"dqn_train_step_vec{i}.npz"), x=x)


def gen_act(out, dm):
    A, n = 15, 128
    torch.manual_seed(0)
    model = dm.AtariDQNModel((3, 64, 64), A)
    rng = np.random.default_rng(77)
    with torch.no_grad():  # a target net that differs from the online net: a deterministic nudge
        for p in model.target_net.parameters():
            p.add_(torch.from_numpy((0.01 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    target_delta_seed = 77
    obs = rng.integers(0, 256, size=(n, 3, 64, 64), dtype=np.uint8)
    with torch.no_grad():
        q_on = model.online_net(torch.from_numpy(obs))
        q_tg = model.target_net(torch.from_numpy(obs))
    np.savez_compressed(os.path.join(out, "dqn_act.npz"), obs_seed=np.int64(77),
                        target_delta_seed=np.int64(target_delta_seed),
                        q_online=q_on.numpy(), q_target=q_tg.numpy(),
                        greedy=q_on.argmax(-1).numpy())


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    dm, dl = _import_reference()
    gen_head(HERE, dm, dl)
    gen_train_step(HERE, dm, dl)
    gen_act(HERE, dm)
    print("DQN golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
