"""Generate the IQN fixtures in tests/golden/ FROM THE REFERENCE ITSELF (data only).

Run where the reference checkout is (see make_golden.py, whose stubs this goes through):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_iqn_golden.py

The reference's own ``DistributionalAtariDQN`` (models/distributed_models.py:35-69),
``ImplicitQuantileHead`` (models/quantile_layers.py:7-54) and ``quantile_regression_loss``
(:83-93) run on parameters from tests/iqn_oracle.py's portable stream (``fixture_params``), so
no fixture holds a parameter vector and every file stays small:

* ``iqn_forward.npz``  A = 6, W = 8, n = 4 frames: the taus the reference drew, q of the online
  net and of a nudged target net (``DistributionalAtariNetwork.forward``); the state_dict keys,
  shapes and dtypes of the whole model.
* ``iqn_act.npz``      the same model at n = 16 frames with explicit taus (the reference's body
  and head called with them): q of both nets, qbar, greedy, q_star per greedy action.  The frames
  are the first 16 of 64 candidates whose top-two gap of qbar exceeds 1e-3.
* ``iqn_head.npz``     N = 16, Ws = 8, Wt = 8, probabilities over two decades, kappa = 1 and 0:
  DistributionalApex._train_step's loss lines (agents/dqn/learning.py:203-216) with the reference's
  loss function; the four scalars, dadv, dv (autograd), priorities.

Checked here, on the generating host: tests/iqn_oracle.py's ``act_like_reference`` against the
reference's ``act`` under one torch seed (same order of RNG calls), and
``impala_amd.iqn.iqn_init_flat`` against the reference's seed-0 construction, bit for bit.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (the stubs and the reference import)
import iqn_oracle as orc  # noqa: E402

A, W = 6, 8
PARAM_SEED, TARGET_SEED, OBS_SEED = 2024, 2025, 77


def _load(net, flat):
    orc.load_flat(net, flat)


def gen_forward_and_act(out, dm):
    model = dm.DistributionalAtariDQN((3, 64, 64), A, n_tau_samples=W)
    online, target = orc.fixture_params(A, PARAM_SEED), orc.fixture_params(A, TARGET_SEED)
    target = online + 0.05 * (target - online)  # a nudged copy
    _load(model.online_net, online)
    _load(model.target_net, target.astype(np.float32))
    sd = model.state_dict()
    cand = orc.fixture_obs(OBS_SEED, 64)
    obs = torch.from_numpy(cand)
    # ---- forward: the reference draws its own taus
    torch.manual_seed(11)
    with torch.no_grad():
        q_on, taus_on = model.online_net(obs[:4])
        q_tg, taus_tg = model.target_net(obs[:4])
    np.savez_compressed(
        os.path.join(out, "iqn_forward.npz"), A=A, W=W, param_seed=PARAM_SEED, target_seed=TARGET_SEED,
        obs_seed=OBS_SEED, taus_online=taus_on.numpy(), taus_target=taus_tg.numpy(),
        q_online=q_on.numpy(), q_target=q_tg.numpy(), state_dict_keys=np.array(list(sd.keys())),
        state_dict_shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]),
        state_dict_dtypes=np.array([str(v.dtype) for v in sd.values()]))
    # ---- act pieces with explicit taus, through the reference's body and head
    rng = np.random.default_rng(OBS_SEED + 1)
    t_on = rng.random((64, W)).astype(np.float32)
    t_tg = rng.random((64, W)).astype(np.float32)
    with torch.no_grad():
        def run(net, taus):
            return net.q(net.body(obs / 255.), torch.from_numpy(taus)).numpy()
        q_on, q_tg = run(model.online_net, t_on), run(model.target_net, t_tg)
        qbar_ref = torch.from_numpy(q_on).mean(1).numpy()
    gap = orc.top2_gap(qbar_ref)
    idx = np.nonzero(gap > 1e-3)[0][:16]
    assert idx.size == 16, "too few candidate frames with a clear greedy action"
    parts = orc.act_parts(q_on[idx], q_tg[idx])
    np.testing.assert_allclose(parts["qbar"], qbar_ref[idx], rtol=1e-6, atol=1e-6)
    greedy = torch.from_numpy(qbar_ref[idx]).argmax(-1).numpy()
    assert np.array_equal(parts["greedy"], greedy)
    np.savez_compressed(os.path.join(out, "iqn_act.npz"), frame_idx=idx, taus_online=t_on[idx],
                        taus_target=t_tg[idx], q_online=q_on[idx], q_target=q_tg[idx],
                        qbar=qbar_ref[idx], greedy=greedy,
                        q_star=q_tg[idx][np.arange(16), :, greedy])
    # ---- the restatement's act against the reference's, same RNG call order
    on, tg = orc.make_net(online, A), orc.make_net(target.astype(np.float32), A)
    eps = torch.full((16, 1), 0.4)
    torch.manual_seed(5)
    ref = model.act(obs[idx], eps)
    torch.manual_seed(5)
    mine = orc.act_like_reference(on, tg, obs[idx], eps, W)
    assert torch.equal(ref[0], mine[0])
    for a, b in zip(ref[1:], mine[1:]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)
    print("act restatement matches the reference's act under one seed")


def gen_init_check(dm):
    from impala_amd.iqn import iqn_init_flat
    torch.manual_seed(0)
    ref = dm.DistributionalAtariDQN((3, 64, 64), 15, n_tau_samples=8)
    flat_ref = torch.cat([p.detach().reshape(-1) for p in ref.online_net.parameters()])
    torch.manual_seed(0)
    mine = iqn_init_flat(15)
    assert torch.equal(flat_ref, mine), "seed-0 init differs from the reference"
    print("seed-0 init: bit for bit the reference's,", mine.numel(), "parameters")


def gen_head(out, ql):
    N, Ws, Wt = 16, 8, 8
    res = {}
    for tag, kappa in (("k1", 1.0), ("k0", 0.0)):
        adv, v, act, taus, tgt, p = orc.head_inputs(N, Ws, Wt, A, kappa, seed=5)
        ta = torch.tensor(adv, requires_grad=True)
        tv = torch.tensor(v, requires_grad=True)
        action = torch.from_numpy(act)
        q = tv.unsqueeze(-1) + ta - ta.mean(-1, keepdim=True)  # ImplicitQuantileHead.forward's last line
        # agents/dqn/learning.py:204-216
        q = q.gather(-1, action.reshape(-1, 1, 1).repeat(1, Ws, 1)).squeeze(-1)
        probabilities = torch.from_numpy(p)
        weight = probabilities.pow(-0.4)
        weight.div_(weight.max())
        target = torch.from_numpy(tgt)
        loss = ql.quantile_regression_loss(q, torch.from_numpy(taus), target, huber_param=kappa).mul(weight).mean()
        loss.backward()
        with torch.no_grad():
            priorities = (target.mean(dim=-1) - q.mean(dim=-1)).abs()
        res.update({f"adv_{tag}": adv, f"v_{tag}": v, f"act_{tag}": act, f"taus_{tag}": taus,
                    f"target_{tag}": tgt, f"prob_{tag}": p,
                    f"scalars_{tag}": np.array([q.mean().item(), target.mean().item(),
                                                priorities.mean().item(), loss.item()], np.float32),
                    f"dadv_{tag}": ta.grad.numpy(), f"dv_{tag}": tv.grad.numpy(),
                    f"priorities_{tag}": priorities.numpy()})
    np.savez_compressed(os.path.join(out, "iqn_head.npz"), beta=np.float32(0.4), **res)


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    dm, _ = mg._import_reference()
    import models.quantile_layers as ql  # (reference)
    gen_init_check(dm)
    gen_forward_and_act(HERE, dm)
    gen_head(HERE, ql)
    print("IQN fixtures written to", HERE)


if __name__ == "__main__":
    main()
