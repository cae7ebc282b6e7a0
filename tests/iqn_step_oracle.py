"""Test helper: the reference of the distributional (IQN) Ape-X training step
(``DistributionalApex._train_step``, agents/dqn/learning.py:197-237), never on the product path.

``tests/iqn_oracle.IqnNet`` under torch autograd with ``iqn_oracle.quantile_regression_loss``
(pinned to the reference's own fixture by tests/test_iqn_host.py), the importance weights of
learning.py:206-210, ``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.Adam``; the cosine's
argument is formed in float32, whatever the net's dtype.  ``dtype=torch.float64``
is the reference the GPU tests hold the step to; ``dtype=torch.float32`` the evaluation whose own
distance from it shows whether a bound is a float32 computation's to meet.

Also the shapes and inputs of the step's tests, shared by the host and the GPU files.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

import iqn_oracle as orc

# the library's defaults (iqn_optim_default)
OPT = dict(lr=6.25e-5, betas=(0.9, 0.999), eps=1e-4, max_grad_norm=40.0, beta=0.4, kappa=1.0)

# the project's bounds (tests/test_gpu_dqn.py)
MET_RTOL, MET_ATOL = 1e-4, 1e-7
PRIO_RTOL, PRIO_ATOL = 1e-4, 1e-6
GRAD_RL2 = 1e-3
PARAM_ABS = 2e-6
BF16_MET_RTOL, BF16_MET_ATOL = 5e-2, 1e-3
BF16_COS = 0.99
MET_NAMES = ("q", "target", "priorities", "loss", "grad_norm")

# (N, W, A, probabilities): the smallest shapes at which each kernel can go wrong --
#   (1, 1)    R = 1: 15 clamped rows in every row tile, a frame sum of one term
#   (3, 8)    a tile spanning two frames and a ragged last tile
#   (2, 5)    W not a power of two
#   (1, 32), (5, 32)  one frame over two tiles: the sum over k crosses the tile boundary
#   (63, 31)  R = 1953 rows: past the FC's persistent grid cap (its second pass) and a split-K
#             remainder in the two weight-gradient GEMMs over R
CASES = [(1, 1, 2, False), (3, 8, 6, True), (2, 5, 15, True), (1, 32, 15, False), (5, 32, 6, True),
         (63, 31, 15, True)]
MULTI = (3, 8, 6, True)  # three consecutive steps
# The input seed of a case: the first k >= 0 at which the float32 evaluation of the reference keeps
# every figure within a quarter of its bound (tests/test_iqn_step_host.py asserts it).  At k = 0 the
# (1, 1) case's single q is 0.006 after cancelling v against the advantages, and 1e-4 of it is below
# float32's own error; no other case needed another seed.
SEEDS = {(1, 1, 2, False): 1}


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def tensor_slices(A: int):
    """name -> slice of the flat vector, in ``parameters()`` order."""
    from impala_amd.iqn import net_specs
    out, off = {}, 0
    for name, shape in net_specs(A):
        n = int(np.prod(shape))
        out[name] = slice(off, off + n)
        off += n
    return out


class Step:
    """The net, its optimizer and one batch's step; ``step`` may be called again (Adam state)."""

    def __init__(self, flat: np.ndarray, A: int, dtype=torch.float64, opt: Optional[dict] = None):
        self.o = dict(OPT, **(opt or {}))
        self.dtype = dtype
        self.net = orc.make_net(flat, A, dtype)
        self.optim = torch.optim.Adam(self.net.parameters(), lr=self.o["lr"], betas=self.o["betas"],
                                      eps=self.o["eps"])

    def loss_parts(self, obs, act, taus, targets, prob):
        """-> (loss, q at the actions [N, W], adv, v, weights): adv and v keep their gradients."""
        dt = self.dtype
        obs = torch.as_tensor(obs)
        taus32 = torch.as_tensor(np.asarray(taus, np.float32))
        adv, v = self.net.heads(obs, taus32, arg32=True)
        adv.retain_grad()
        v.retain_grad()
        q = v + adv - adv.mean(dim=-1, keepdim=True)
        W = taus32.shape[-1]
        act = torch.as_tensor(act).long()
        qa = q.gather(-1, act.reshape(-1, 1, 1).repeat(1, W, 1)).squeeze(-1)
        targets = torch.as_tensor(targets).to(dt)
        if prob is None:
            w = torch.ones(obs.shape[0], dtype=dt)
        else:  # learning.py:206-208
            w = torch.as_tensor(prob).to(dt).pow(-self.o["beta"])
            w = w / w.max()
        loss = orc.quantile_regression_loss(qa, taus32.to(dt), targets, self.o["kappa"]).mul(w).mean()
        return loss, qa, adv, v, w

    def step(self, obs, act, taus, targets, prob=None, update: bool = True) -> Dict[str, np.ndarray]:
        self.optim.zero_grad()
        loss, qa, adv, v, _ = self.loss_parts(obs, act, taus, targets, prob)
        loss.backward()
        grad = torch.cat([p.grad.reshape(-1) for p in self.net.parameters()]).numpy().copy()
        targets = torch.as_tensor(targets).to(self.dtype)
        prio = (targets.mean(-1) - qa.detach().mean(-1)).abs()
        norm = torch.nn.utils.clip_grad_norm_(self.net.parameters(), self.o["max_grad_norm"])
        if update:
            self.optim.step()
        return dict(met=dict(q=qa.mean().item(), target=targets.mean().item(),
                             priorities=prio.mean().item(), loss=loss.item(), grad_norm=norm.item()),
                    prio=prio.numpy().copy(), grad=grad, params=orc.flat_params(self.net),
                    dadv=adv.grad.numpy().copy(), dv=v.grad.squeeze(-1).numpy().copy(),
                    qa=qa.detach().numpy().copy())


# ---------------------------------------------------------------- the tests' inputs
_FLAT, _BATCH, _REF = {}, {}, {}


def flat0(A: int) -> np.ndarray:
    if A not in _FLAT:
        _FLAT[A] = orc.fixture_params(A, 31 + A)
    return _FLAT[A]


def batch(case, step: int = 0):
    """(obs u8 [N,3,64,64], act i64 [N], taus f32 [N,W], targets f32 [N,W], prob f32 [N] or None).
    Targets lie around the net's own q (so both Huber branches occur); with probabilities the
    smallest one -- the largest weight -- sits on the last frame; where W > 1, target (0, 0) is the
    float32 neighbour of the float64 reference's q of row 0 (delta ~ 0: rho jumps, H' ~ 0)."""
    key = (case, step)
    if key in _BATCH:
        return _BATCH[key]
    N, W, A, probs = case
    k = SEEDS.get(case, 0)
    rng = np.random.default_rng(1000 * N + 10 * W + A + 7919 * step + 104729 * k)
    obs = orc.fixture_obs(300 + N + step + 1000 * k, N)
    act = rng.integers(0, A, size=(N,), dtype=np.int64)
    taus = orc.edge_taus(N, W, seed=N + step)
    with torch.no_grad():
        net = orc.make_net(flat0(A), A, torch.float64)
        q = net(torch.as_tensor(obs), torch.as_tensor(taus), arg32=True).numpy()
    qa = q[np.arange(N), :, act]
    tgt = (qa.mean(1, keepdims=True) + 1.5 * rng.standard_normal((N, W))).astype(np.float32)
    if W > 1:  # (alone, it would be a batch of zero loss and zero gradient)
        tgt[0, 0] = np.nextafter(np.float32(qa[0, 0]), np.float32(np.inf))
    else:  # edge_taus puts tau = 0 on row 0, and rho = |0 - 1{delta < 0}| is 0 above q: targets below it
        tgt = (qa - 0.25 - np.abs(tgt - qa)).astype(np.float32)
    prob = None
    if probs:
        prob = (10.0 ** rng.uniform(-4, -2, N)).astype(np.float32)
        prob[-1] = np.float32(0.5 * prob.min())
    _BATCH[key] = (obs, act, taus, tgt, prob)
    return _BATCH[key]


def reference(case, dtype=torch.float64):
    """One step from flat0 on batch(case): computed once, shared, left unchanged."""
    key = (case, dtype)
    if key not in _REF:
        _REF[key] = Step(flat0(case[2]), case[2], dtype).step(*batch(case))
    return _REF[key]


def reference_steps(case, n: int, dtype=torch.float64):
    """n consecutive steps on batch(case, 0..n-1) -> the list of their outputs."""
    key = (case, dtype, n)
    if key not in _REF:
        s = Step(flat0(case[2]), case[2], dtype)
        _REF[key] = [s.step(*batch(case, i)) for i in range(n)]
    return _REF[key]
