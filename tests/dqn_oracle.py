"""Test helper: torch-CPU restatement of the Ape-X DQN learner, written from the formulas
(DESIGN.md §13), never on the product path.

* net   : AtariBody -> LayerNorm(1024) -> Linear(1024, 512) -> GELU -> adv Linear(512, A) and
  v Linear(512, 1);  q = v + adv - mean_A(adv)
* step  : err = target - q[a];  w = p^-beta / max(p^-beta) (1 without probabilities);
  loss = 1/2 mean(err^2 w);  clip_grad_norm_(40);  Adam(6.25e-5, eps 1e-4);  priorities |err|
* act   : pi = eps / (A - 1) everywhere, 1 - eps on argmax q

Pinned against the reference's own outputs by tests/golden/make_dqn_golden.py ->
tests/golden/dqn_*.npz -> tests/test_dqn_host.py.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

HIDDEN = 512
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAIN_VEC_FILES = 12  # dqn_train_step_vec{i}.npz: params0 | grads1 | params1 | params3, equal chunks


class DuelingNet(nn.Module):
    """state_dict keys = impala_amd.dqn.net_specs (one DuellingAtariNetwork)."""

    def __init__(self, A: int = 15):
        super().__init__()
        self.body = nn.Module()
        self.body.body = nn.Sequential(nn.Conv2d(3, 32, 8, stride=4), nn.ReLU(),
                                       nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                                       nn.Conv2d(64, 64, 3, stride=1), nn.ReLU(), nn.Flatten())
        self.q = nn.Module()
        self.q.body = nn.Sequential(nn.LayerNorm(1024), nn.Linear(1024, HIDDEN), nn.GELU())
        self.q.q = nn.Linear(HIDDEN, A)
        self.q.v = nn.Linear(HIDDEN, 1)

    def heads(self, obs_u8: torch.Tensor):
        x = obs_u8.to(self.q.v.weight.dtype) / 255.
        h = self.q.body(self.body.body(x))
        return self.q.q(h), self.q.v(h)

    def forward(self, obs_u8: torch.Tensor) -> torch.Tensor:
        adv, v = self.heads(obs_u8)
        return v + adv - adv.mean(dim=-1, keepdim=True)


def make_net(flat: np.ndarray, A: int = 15, dtype=torch.float32) -> DuelingNet:
    net = DuelingNet(A).to(dtype)
    load_flat(net, flat)
    return net


def load_flat(net: nn.Module, flat: np.ndarray) -> None:
    off = 0
    with torch.no_grad():
        for p in net.parameters():
            n = p.numel()
            p.copy_(torch.as_tensor(np.asarray(flat[off:off + n])).to(p.dtype).view_as(p))
            off += n
    assert off == len(flat)


def flat_params(net: nn.Module) -> np.ndarray:
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy().copy()


def flat_grads(net: nn.Module) -> np.ndarray:
    return torch.cat([p.grad.detach().reshape(-1) for p in net.parameters()]).numpy().copy()


def weights(probabilities: Optional[torch.Tensor], beta: float, like: torch.Tensor) -> torch.Tensor:
    if probabilities is None:
        return torch.ones_like(like)
    w = probabilities.to(like.dtype).pow(-beta)
    return w / w.max()


def loss_from_heads(adv, v, act, target, probabilities=None, beta: float = 0.4) -> Dict[str, np.ndarray]:
    """The loss head alone on adv [N, A], v [N]: metrics (q, target, priorities, loss), dadv, dv,
    priorities."""
    adv = torch.as_tensor(adv).clone().requires_grad_(True)
    v = torch.as_tensor(v).reshape(-1).clone().requires_grad_(True)
    act, target = torch.as_tensor(act).long(), torch.as_tensor(target).to(adv.dtype)
    q = v.unsqueeze(-1) + adv - adv.mean(dim=-1, keepdim=True)
    qa = q.gather(1, act.unsqueeze(-1)).squeeze(-1)
    w = weights(None if probabilities is None else torch.as_tensor(probabilities), beta, qa)
    err = target - qa
    loss = 0.5 * (err.pow(2) * w).mean()
    loss.backward()
    prio = err.detach().abs()
    return dict(metrics=np.array([qa.mean().item(), target.mean().item(), prio.mean().item(),
                                  loss.item()]),
                dadv=adv.grad.numpy(), dv=v.grad.numpy(), priorities=prio.numpy())


def make_optimizer(net: nn.Module, lr: float = 6.25e-5, eps: float = 1e-4):
    return torch.optim.Adam(net.parameters(), lr=lr, eps=eps)


def train_step(net: DuelingNet, opt, obs, act, target, probabilities=None, beta: float = 0.4,
               max_grad_norm: float = 40.0) -> Dict[str, np.ndarray]:
    """One learner step; returns the 5 metrics, the post-clip grads and the priorities."""
    dt = net.q.v.weight.dtype
    opt.zero_grad()
    obs, act = torch.as_tensor(obs), torch.as_tensor(act).long()
    target = torch.as_tensor(target).to(dt)
    qa = net(obs).gather(1, act.unsqueeze(-1)).squeeze(-1)
    w = weights(None if probabilities is None else torch.as_tensor(probabilities), beta, qa)
    err = target - qa
    loss = 0.5 * (err.pow(2) * w).mean()
    loss.backward()
    gn = torch.nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm)
    grads = flat_grads(net)
    opt.step()
    prio = err.detach().abs()
    return dict(q=qa.mean().item(), target=target.mean().item(), priorities=prio.mean().item(),
                loss=loss.item(), grad_norm=gn.item(), grads=grads, prio=prio.numpy())


def act_pi(q: np.ndarray, eps) -> np.ndarray:
    """pi [n, A] of AtariDQNModel.act: 1 - eps on argmax q (lowest index on ties), eps / (A - 1)
    elsewhere."""
    q = np.asarray(q)
    n, A = q.shape
    eps = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1, 1), (n, 1))
    pi = np.ones((n, A)) * (eps / (A - 1))
    pi[np.arange(n), q.argmax(-1)] = 1.0 - eps[:, 0]
    return pi


def synthetic_batch(N: int, A: int = 15, seed: int = 99, probs: bool = True):
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 256, size=(N, 3, 64, 64), dtype=np.uint8)
    act = rng.integers(0, A, size=(N,), dtype=np.int64)
    tgt = rng.standard_normal(N).astype(np.float32)
    p = (10.0 ** rng.uniform(-4, -2, N)).astype(np.float32) if probs else None
    return obs, act, tgt, p


def load_train_fixture() -> Dict[str, np.ndarray]:
    """dqn_train_step.npz plus the chunked long vectors (params0, grads1, params1, params3)."""
    d = dict(np.load(os.path.join(GOLDEN, "dqn_train_step.npz"), allow_pickle=False))
    vec = np.concatenate([np.load(os.path.join(GOLDEN, f"dqn_train_step_vec{i}.npz"))["x"]
                          for i in range(TRAIN_VEC_FILES)])
    n = int(d["n_params"])
    assert vec.size == 4 * n
    d["params0"], d["grads1"], d["params1"], d["params3"] = np.split(vec, 4)
    return d
