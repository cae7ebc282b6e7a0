"""Test helper: torch-CPU restatement of the distributional (IQN) Ape-X pieces, written from the
formulas, never on the product path.

* net    : x = AtariBody(obs / 255); e = cos(pi * i * tau), i = 1..64 (torch's order: (pi * i) * tau);
  phi = GELU(Wq e + bq); y = LayerNorm(x * phi); h = GELU(Wfc y + bfc); q = v + adv - mean_A(adv)
* act    : qbar = mean_k q_online; greedy = argmax qbar; pi = eps / (A - 1) everywhere, 1 - eps on
  greedy; q_pi = qbar[action]; q_star[k] = q_target[k][greedy]
* ingest : per quantile column the n-step return of tests/dqn_replay_oracle.py; priority
  |mean_k target - q_pi|
* loss   : quantile regression (Huber kappa, or |delta| at kappa = 0), importance weights
  p^-beta / max; gradients by autograd

``dtype=torch.float64`` runs the same code in double.  Pinned against the reference's own outputs
by tests/golden/make_iqn_golden.py -> tests/golden/iqn_*.npz -> tests/test_iqn_host.py.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

import dqn_replay_oracle as rorc

HIDDEN = 512
N_COS = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class IqnNet(nn.Module):
    """state_dict keys = one DistributionalAtariNetwork's (impala_amd.iqn.net_specs plus the
    ``embedding_range`` buffer)."""

    def __init__(self, A: int = 15):
        super().__init__()
        self.body = nn.Module()
        self.body.body = nn.Sequential(nn.Conv2d(3, 32, 8, stride=4), nn.ReLU(),
                                       nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                                       nn.Conv2d(64, 64, 3, stride=1), nn.ReLU(), nn.Flatten())
        self.q = nn.Module()
        self.q.quantile_layer = nn.Module()
        self.q.quantile_layer.register_buffer("embedding_range",
                                              torch.arange(1, N_COS + 1).reshape(1, 1, N_COS))
        self.q.quantile_layer.output_layer = nn.Sequential(nn.Linear(N_COS, 1024), nn.GELU())
        self.q.project = nn.Sequential(nn.LayerNorm(1024), nn.Linear(1024, HIDDEN), nn.GELU())
        self.q.q = nn.Linear(HIDDEN, A)
        self.q.v = nn.Linear(HIDDEN, 1)

    def heads(self, obs_u8: torch.Tensor, taus: torch.Tensor, arg32: bool = False):
        """-> adv [n, W, A], v [n, W, 1].  ``arg32``: the cosine's argument formed in float32 (as
        the reference's own float32 run and the kernel form it), whatever the net's dtype."""
        dt = self.q.v.weight.dtype
        x = self.body.body(obs_u8.to(dt) / 255.)
        tau = torch.as_tensor(taus).to(torch.float32 if arg32 else dt)
        e = torch.cos((torch.pi * self.q.quantile_layer.embedding_range * tau.unsqueeze(-1)).to(dt))
        phi = self.q.quantile_layer.output_layer(e)
        h = self.q.project(x.unsqueeze(1) * phi)
        return self.q.q(h), self.q.v(h)

    def forward(self, obs_u8: torch.Tensor, taus: torch.Tensor, arg32: bool = False) -> torch.Tensor:
        adv, v = self.heads(obs_u8, taus, arg32)
        return v + adv - adv.mean(dim=-1, keepdim=True)


def load_flat(net: nn.Module, flat: np.ndarray) -> None:
    off = 0
    with torch.no_grad():
        for p in net.parameters():
            n = p.numel()
            p.copy_(torch.as_tensor(np.asarray(flat[off:off + n])).to(p.dtype).view_as(p))
            off += n
    assert off == len(flat)


def make_net(flat: np.ndarray, A: int = 15, dtype=torch.float32) -> IqnNet:
    net = IqnNet(A).to(dtype)
    load_flat(net, flat)
    return net


def flat_params(net: nn.Module) -> np.ndarray:
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy().copy()


def fixture_params(A: int, seed: int) -> np.ndarray:
    """One net's flat fp32 parameters from numpy's PCG64 stream (the same on every host): weights
    uniform in +-sqrt(3 / fan_in) (unit output variance for unit inputs), biases in +-0.1, the
    LayerNorm weight in 1 +- 0.2.  What the fixtures' generator loads into the reference and the
    tests regenerate, so no fixture holds a parameter vector."""
    from impala_amd.iqn import net_specs
    rng = np.random.default_rng(seed)
    out = []
    for name, shape in net_specs(A):
        n = int(np.prod(shape))
        u = rng.random(n) * 2.0 - 1.0
        if name == "q.project.0.weight":
            x = 1.0 + 0.2 * u
        elif name.endswith(".bias"):
            x = 0.1 * u
        else:
            x = np.sqrt(3.0 / int(np.prod(shape[1:]))) * u
        out.append(x.astype(np.float32))
    return np.concatenate(out)


def fixture_obs(seed: int, n: int = 64) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3, 64, 64), dtype=np.uint8)


def edge_taus(n: int, W: int, seed: int = 0) -> np.ndarray:
    """taus [n, W] in [0, 1) holding 0 and (where there is room) the two largest float32 below 1."""
    top = np.nextafter(np.float32(1), np.float32(0))
    t = np.minimum(np.random.default_rng(seed).random((n, W)).astype(np.float32), top)
    flat = t.reshape(-1)
    flat[0] = 0.0
    if flat.size > 1:
        flat[-1] = top
    if flat.size > 2:
        flat[flat.size // 2] = np.nextafter(top, np.float32(0))
    return t


# ---------------------------------------------------------------- taus drawn by the library
def draw_taus(seed: int, counter: int, which: int, R: int) -> np.ndarray:
    """u_r = (mix(mix(seed ^ mix(counter)) + ((1 + which) << 32) + r) >> 40) * 2^-24."""
    base = rorc.mix((seed & rorc.M64) ^ rorc.mix(counter & rorc.M64))
    return np.array([(rorc.mix((base + ((1 + which) << 32) + r) & rorc.M64) >> 40) * 2.0 ** -24
                     for r in range(R)], dtype=np.float32)


# ---------------------------------------------------------------- act
def act_parts(q_on, q_tg) -> Dict[str, np.ndarray]:
    """qbar [n, A] (k-ordered sum over W, then / W, in q's dtype), greedy [n], q_star [n, W]."""
    q_on, q_tg = np.asarray(q_on), np.asarray(q_tg)
    n, W, A = q_on.shape
    s = np.zeros((n, A), dtype=q_on.dtype)
    for k in range(W):
        s = s + q_on[:, k, :]
    qbar = s / q_on.dtype.type(W)
    g = qbar.argmax(-1)
    return dict(qbar=qbar, greedy=g, q_star=q_tg[np.arange(n), :, g])


def top2_gap(qbar: np.ndarray) -> np.ndarray:
    s = np.sort(np.asarray(qbar, dtype=np.float64), axis=-1)
    return s[:, -1] - s[:, -2]


def act_like_reference(net_on: IqnNet, net_tg: IqnNet, obs: torch.Tensor, eps: torch.Tensor, W: int):
    """DistributionalAtariDQN.act with the reference's order of global-RNG calls: rand (online
    taus), multinomial, rand (target taus)."""
    with torch.no_grad():
        n = obs.shape[0]
        q = net_on(obs, torch.rand(size=(n, W))).mean(1)
        A = q.shape[1]
        greedy = q.argmax(-1, keepdim=True)
        pi = torch.ones_like(q) * (eps / (A - 1))
        pi.scatter_(dim=-1, index=greedy, src=1.0 - eps)
        action = pi.multinomial(1, replacement=True)
        q_pi = q.gather(dim=-1, index=action)
        q_tg = net_tg(obs, torch.rand(size=(n, W)))
        q_star = q_tg.gather(dim=-1, index=greedy.unsqueeze(1).repeat(1, W, 1)).squeeze(-1)
    return action, q_pi, q_star


# ---------------------------------------------------------------- actor ingest
def nstep_targets(rewards, done, q_pi, q_star, n_step: int, gamma: float):
    """float64: targets [L-1, W] (column k: dqn_replay_oracle.nstep_targets on q_star[:, k]) and
    priorities [L-1] = |mean_k target - q_pi|."""
    q_star = np.asarray(q_star, dtype=np.float64)
    L, W = q_star.shape
    tg = np.stack([rorc.nstep_targets(rewards, done, q_star[:, k], n_step, gamma) for k in range(W)], 1)
    prio = np.abs(tg.mean(1) - np.asarray(q_pi, dtype=np.float64)[:L - 1])
    return tg, prio


# ---------------------------------------------------------------- loss head
def quantile_regression_loss(q, taus, target, kappa: float = 1.0):
    """models/quantile_layers.py:83-93 restated: q [N, Ws], taus [N, Ws], target [N, Wt] -> [N]."""
    delta = target.unsqueeze(1) - q.unsqueeze(2)
    weight = torch.abs(taus.unsqueeze(2) - (delta < 0.).to(q.dtype)).detach()
    a = torch.abs(delta)
    if kappa == 0:
        hub = a
    else:
        m = torch.clamp_max(a, kappa)
        hub = 0.5 * m.pow(2) + kappa * (a - m)
    return (weight * hub).sum(1).mean(-1)


def loss_from_heads(adv, v, act, taus, targets, probabilities=None, kappa: float = 1.0,
                    beta: float = 0.4, dtype=torch.float32) -> Dict[str, np.ndarray]:
    """The loss head alone on adv [N, Ws, A], v [N, Ws]: metrics (q, target, priorities, loss),
    dadv, dv, priorities."""
    adv = torch.as_tensor(adv).to(dtype).clone().requires_grad_(True)
    N, Ws, A = adv.shape
    v = torch.as_tensor(v).to(dtype).reshape(N, Ws).clone().requires_grad_(True)
    act = torch.as_tensor(act).long()
    taus = torch.as_tensor(taus).to(dtype).reshape(N, Ws)
    targets = torch.as_tensor(targets).to(dtype)
    q = v.unsqueeze(-1) + adv - adv.mean(dim=-1, keepdim=True)
    qa = q.gather(-1, act.reshape(-1, 1, 1).repeat(1, Ws, 1)).squeeze(-1)
    if probabilities is None:
        w = torch.ones(N, dtype=dtype)
    else:
        w = torch.as_tensor(probabilities).to(dtype).pow(-beta)
        w = w / w.max()
    loss = quantile_regression_loss(qa, taus, targets, kappa).mul(w).mean()
    loss.backward()
    prio = (targets.mean(-1) - qa.mean(-1)).detach().abs()
    return dict(metrics=np.array([qa.mean().item(), targets.mean().item(), prio.mean().item(),
                                  loss.item()]),
                dadv=adv.grad.numpy(), dv=v.grad.numpy(), priorities=prio.numpy())


def head_inputs(N: int, Ws: int, Wt: int, A: int, kappa: float, seed: int = 5, probs: bool = True):
    """Random heads inputs holding exact ties: transition 0's first target equals its first q
    (delta = 0) and its second target is q + kappa (|delta| = kappa), in float32."""
    rng = np.random.default_rng(seed)
    adv = rng.standard_normal((N, Ws, A)).astype(np.float32)
    v = rng.standard_normal((N, Ws)).astype(np.float32)
    act = rng.integers(0, A, size=(N,), dtype=np.int64)
    taus = rng.random((N, Ws)).astype(np.float32)
    tgt = (0.5 * rng.standard_normal((N, Wt))).astype(np.float32)
    # q of (0, 0) is exact in float32 in any summation order: dyadic advantages in +- pairs (their
    # sum, and so the mean, is exactly 0) and a dyadic v
    a0 = np.zeros(A, dtype=np.float32)
    for k in range(0, A - 1, 2):
        a0[k], a0[k + 1] = 0.25 * (k + 1), -0.25 * (k + 1)
    adv[0, 0] = a0
    v[0, 0] = 0.75
    q00 = np.float32(v[0, 0] + a0[act[0]])
    tgt[0, 0] = q00
    if Wt > 1:
        tgt[0, 1] = np.float32(q00 + np.float32(kappa))
    p = (10.0 ** rng.uniform(-4, -2, N)).astype(np.float32) if probs else None
    return adv, v, act, taus, tgt, p
