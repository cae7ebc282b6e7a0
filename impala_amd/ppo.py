"""PPOLearner — drop-in for ``agents/ppo/learning.py:78-143`` on MI355X.

Same constructor (``model, replay_buffer, optimizer, batch_size=256, max_grad_norm=0.5,
entropy_coeff=0.01, learning_starts=None, model_push_period=8``), ``prepare`` /
``train_step`` behaviour and metric keys (``train/{loss,entropy,td,pg,target,kl,ratio}``,
``train_step/grad_norm``, ``debug/*``).  ``_train_step`` is one HIP call on a PPO handle
(``impala_ppo_train_step``: the shared CNN forward, the fused PPO head -- clipped surrogate,
½·td², entropy, KL -- the shared backward, clip and Adam), or for data-parallel replicas the
data-parallel gradient path of ``distributed.compute_grads_allreduced``.

The batch is flat transitions ``(s u8 [N,3,64,64], a i64 [N], v_target f32 [N], pi_ref
logits f32 [N,A])`` -- the order ``_train_step`` unpacks (learning.py:132).  Over a
``DeviceTransitionBuffer`` the learner draws slots and the step reads them in place
(``impala_ppo_train_step_rows``); over a host ``ReplayBuffer`` it collates and copies the
sampled items, as the reference does.

``PPOActor`` mirrors ``PPOActorRemote`` (learning.py:22-72).  The reference's target line
(``rlego.lambda_returns(r[:-1], discount_t[:-1], values[1:], lambda)``, learning.py:68) cannot
run as shipped -- ``values`` is undefined and rlego is absent -- so it is restated here as rlax's
``lambda_returns`` on the actor's ``v``, with a fixed fp32 operation order (include/impala_hip.h,
impala_ppo_extend_rollout; parity unpinned).
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import torch

from impala_amd import _lib
from impala_amd.core import Actor, Learner
from impala_amd.engine import Engine
from impala_amd.learner import ImpalaAdam


def collate_transitions(batch, device):
    """CircularBuffer(collate_fn=torch.cat) semantics (agents/ppo/builder.py:30-35): a list of
    transition items ``[s, a, target, pi_ref]`` (each with a leading dim, or without one) ->
    4 contiguous device tensors; an already-collated 4-tuple is moved as is."""
    if isinstance(batch, (tuple, list)) and len(batch) == 4 and isinstance(batch[0], torch.Tensor) \
            and batch[0].dim() == 4:
        fields = list(batch)
    else:
        fields = []
        for j in range(4):
            xs = [item[j] for item in batch]
            xs = [x if x.dim() > (3 if j == 0 else (1 if j == 3 else 0)) else x.unsqueeze(0)
                  for x in xs]
            fields.append(torch.cat(xs))
    out = []
    for j, t in enumerate(fields):
        if t.device != device:
            if t.device.type == "cpu" and torch.cuda.is_available():
                t = t.pin_memory()
            t = t.to(device, non_blocking=True)
        out.append(t.contiguous())
    s, a, tgt, mu = out
    return (s, a.reshape(-1).to(torch.int64), tgt.reshape(-1).float(),
            mu.reshape(s.shape[0], -1).float())


class PPOLearner(Learner):
    def __init__(self, model, replay_buffer, optimizer=None, batch_size: int = 256,
                 max_grad_norm: float = 0.5, entropy_coeff: float = 0.01,
                 learning_starts: Optional[int] = None, model_push_period: int = 8,
                 clip_coeff: float = 0.1, dtype: Optional[str] = None, process_group=None,
                 world_size: Optional[int] = None):
        self._model = model
        self._replay_buffer = replay_buffer
        self._optimizer = optimizer = ImpalaAdam.of(optimizer)
        self._batch_size = batch_size
        self._max_grad_norm = max_grad_norm
        self._entropy_coeff = entropy_coeff
        self._learning_starts = learning_starts
        self._model_push_period = model_push_period
        self._pg = process_group
        self._native_dp = None  # decided at the first data-parallel step (distributed.py)
        if world_size is None:
            world_size = 1
            if process_group is not None:
                import torch.distributed as dist
                world_size = dist.get_world_size(process_group)
        self._world_size = int(world_size)
        self._device = None
        self._step_counter = 0
        self.can_train = False
        self._rows = True    # read a device ring in place until the handle refuses it
        self._ring = None    # (replay, Engine.ppo_ring_batch of its arrays)
        # losses.ppo_loss's clip_coeff default (losses.py:131): the learner never overrides it
        self._engine = Engine(model, batch_size=batch_size, algo="ppo", ppo_clip=clip_coeff,
                              dtype=dtype, lr=optimizer.lr, eps=optimizer.eps,
                              betas=optimizer.betas, max_grad_norm=max_grad_norm,
                              entropy_coeff=entropy_coeff, world_size=self._world_size)
        model._train_engine = self._engine

    @property
    def engine(self) -> Engine:
        return self._engine

    def device(self) -> torch.device:
        if self._device is None:
            self._device = self._model.flat.device
        return self._device

    @property
    def samples_per_step(self) -> int:
        """Environment frames one train_step consumes (DistributedAgent.train's total without
        a controller)."""
        return self._batch_size

    def prepare(self):  # learning.py:105-108
        if not self.can_train:
            self._replay_buffer.warm_up(self._learning_starts)
        self.can_train = True

    def train_step(self):  # learning.py:110-128
        t0 = time.perf_counter()
        rb = self._replay_buffer
        metrics = None
        if self._rows and self._world_size == 1 and self._batch_size <= _lib.MAX_ROWS and \
                hasattr(rb, "sample_rows"):
            # a device ring: draw slots, the step reads them in place (no gather, no copy)
            _, rs, _ = rb.sample_rows(self._batch_size)
            t1 = time.perf_counter()
            try:
                metrics = self._train_step(None, rows=rs)
            except _lib.Unsupported:  # refused before anything was enqueued: gather from now on
                self._rows = False
                batch = rs.gather()
        else:
            _, batch, _ = rb.sample(self._batch_size)
            batch = collate_transitions(batch, self.device())
        if metrics is None:
            t1 = time.perf_counter()
            metrics = self._train_step(batch)
        t2 = time.perf_counter()
        self._step_counter += 1
        update_time = 0
        if self._step_counter % self._model_push_period == 0:
            start = time.perf_counter()
            self._model.push()
            update_time = (time.perf_counter() - start) * 1000
        metrics["debug/replay_sample_per_second"] = (self._batch_size / ((t1 - t0) * 1000))
        metrics["debug/gradient_per_second"] = (self._batch_size / ((t2 - t1) * 1000))
        metrics["debug/total_time"] = (time.perf_counter() - t0) * 1000
        metrics["debug/forward_dt"] = (t2 - t1) * 1000
        metrics["debug/update_time"] = update_time
        return metrics

    def _train_step(self, batch, rows=None) -> Dict[str, torch.Tensor]:  # learning.py:130-143
        """The step on a collated device batch, or (``rows``: a RowSample of a device ring) on
        the ring's slots read in place."""
        e = self._engine
        # this step's metrics vector (impala_set_metrics), which the returned values are views of
        m = torch.empty(_lib.NUM_METRICS, dtype=torch.float32, device=e.device)
        e.bind_metrics(m)
        if rows is not None:
            if self._ring is None or self._ring[0] is not rows.replay:
                self._ring = (rows.replay, e.ppo_ring_batch(rows.replay.fields))
            e.ppo_train_step_rows(self._ring[1], rows.idx)
        elif self._world_size == 1:
            e.train_step(*batch)
        else:
            from .distributed import (compute_grads_allreduced, native_dp_buckets,
                                      native_dp_enabled)
            if self._native_dp is None:
                native = native_dp_enabled(self._pg)
                if native:
                    e.dp_init(self._pg)  # raises before the path is chosen if RCCL fails
                self._native_dp = native
            if self._native_dp:
                e.dp_train_step(*batch, buckets=native_dp_buckets())
            else:
                compute_grads_allreduced(e, batch, self._model.flat_grad, group=self._pg)
                e.apply_update()
        v = m.unbind(0)  # device scalars; float(v) synchronises lazily
        return {name: v[i] for name, i in _lib.PPO_METRIC_SLOTS}


def lambda_returns(rewards, done, values, gamma: float, lambda_: float) -> torch.Tensor:
    """rlax ``lambda_returns(r[:-1], discount[:-1], v[1:], lambda)`` for one rollout of L steps
    (rewards, done, values [L]) -> targets [L-1], on the CPU in fp32 with the operation order of
    include/impala_hip.h (impala_ppo_extend_rollout): every product and sum a separate fp32
    operation, so it equals the ingest kernel bit for bit."""
    f32 = torch.float32
    r = torch.as_tensor(rewards).reshape(-1).to("cpu", f32)
    v = torch.as_tensor(values).reshape(-1).to("cpu", f32)
    d = torch.as_tensor(done).reshape(-1).to("cpu").to(torch.bool)
    L = r.numel()
    if L < 2 or v.numel() != L or d.numel() != L:
        raise ValueError("lambda_returns: rewards, done and values of one length L >= 2")
    lam = torch.tensor(lambda_, dtype=f32)
    disc = torch.where(d, torch.zeros((), dtype=f32), torch.tensor(gamma, dtype=f32))
    oml = torch.ones((), dtype=f32) - lam
    K = L - 1
    out = torch.empty(K, dtype=f32)
    acc = v[K]
    for t in range(K - 1, -1, -1):
        p = oml * v[t + 1]
        q = lam * acc
        s = p + q
        m = disc[t] * s
        acc = r[t] + m
        out[t] = acc
    return out


class PPOActor(Actor):
    """``PPOActorRemote`` (agents/ppo/learning.py:22-72) for in-process actors: it collects
    ``(obs, action, reward, done, logpi, v)`` per step and turns every ``rollout_length`` steps
    into ``rollout_length - 1`` transitions ``[s, a, target, pi_ref]`` in the replay."""

    def __init__(self, model, replay_buffer=None, deterministic_policy: bool = False,
                 gamma: float = 0.99, lambda_: float = 0.95, rollout_length: int = 128):
        self._gamma = gamma
        self._lambda = lambda_
        self._deterministic_policy = torch.tensor([deterministic_policy])
        self._model = model
        self._replay_buffer = replay_buffer
        self._rollout_length = rollout_length
        self._trajectory = []
        self._last_transition = None

    def act(self, timestep):
        obs = timestep.observation if hasattr(timestep, "observation") else timestep[0]
        action, logpi, v = self._model.act(obs, self._deterministic_policy)
        return action, {"logpi": logpi, "v": v}

    async def async_act(self, timestep):
        return self.act(timestep)

    def observe_init(self, timestep) -> None:
        if self._replay_buffer is None:
            return
        self._last_transition = timestep

    async def async_observe_init(self, timestep) -> None:
        self.observe_init(timestep)

    def observe(self, action, next_timestep) -> None:  # learning.py:49-57
        if self._replay_buffer is None:
            return
        lt = self._last_transition
        obs = lt.observation if hasattr(lt, "observation") else lt[0]
        act, info = action
        reward, done = next_timestep[1], next_timestep[2]
        self._trajectory.append((torch.as_tensor(obs).reshape(3, 64, 64),
                                 torch.as_tensor(act).reshape(()),
                                 torch.as_tensor(reward, dtype=torch.float32).reshape(()),
                                 torch.as_tensor(done).reshape(()),
                                 torch.as_tensor(info["logpi"]).reshape(-1),
                                 torch.as_tensor(info["v"], dtype=torch.float32).reshape(())))
        self._last_transition = next_timestep
        if len(self._trajectory) == self._rollout_length:
            self.update()

    async def async_observe(self, action, next_timestep) -> None:
        self.observe(action, next_timestep)

    def update(self) -> None:  # learning.py:59-63
        if self._replay_buffer is None or len(self._trajectory) < 2:
            return
        self._make_replay()

    async def async_update(self) -> None:
        self.update()

    def _make_replay(self):  # learning.py:65-69
        """The rollout's transitions into the replay: natively (``extend_rollout``) when the
        replay offers it, else targets from ``lambda_returns`` and one item per transition."""
        s, a, r, d, pi_ref, v = (torch.stack(x) for x in zip(*self._trajectory))
        self._trajectory = []
        rb = self._replay_buffer
        if hasattr(rb, "extend_rollout"):
            return rb.extend_rollout(s, a, r, d, pi_ref, v, self._gamma, self._lambda)
        tgt = lambda_returns(r, d, v, self._gamma, self._lambda)
        a, pi_ref = a.to(torch.int64), pi_ref.to(torch.float32)
        return rb.extend([[s[t:t + 1], a[t:t + 1], tgt[t:t + 1], pi_ref[t:t + 1]]
                          for t in range(tgt.numel())])


class PPOActorFactory:
    def __init__(self, model, rb, rollout_length: int = 128):
        self._args = (model, rb, rollout_length)

    def __call__(self, index: int) -> Actor:
        m, rb, L = self._args
        return PPOActor(m, rb, False, rollout_length=L)
