"""Ape-X DQN on the HIP learner: ``AtariDQNModel``
(models/distributed_models.py:72-104), ``ApexLearner`` (agents/dqn/learning.py:97-191),
``PrioritizedReplay`` (rlmeta ReplayBuffer + PrioritizedSampler as agents/dqn/builder.py:82-89
builds them), ``NativePrioritizedReplay`` (the same ring on the library's ``dqn_replay``) and
``ApexDQNBuilder`` (agents/dqn/builder.py:76-120).

The network is IMPALA's trunk with a 512-wide projection and a dueling head; the step is one
``dqn_train_step`` call (include/dqn_hip.h) or, over a ``NativePrioritizedReplay``, one
``dqn_train_step_replay`` call: sample, step and priority update
(``dqn_train_step_replay_rows`` with ``in_place=True``: the step reads the sampled ring rows where
they lie).  ``ApexActor`` (agents/dqn/learning.py:17-65) feeds that replay one rollout at a time.
The compute path is the HIP library only.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from impala_amd import _lib
from impala_amd._lib import check, lib
from impala_amd.core import Actor, Builder, Learner
from impala_amd.flat import FlatModule, spec_count, trunk_init_flat
from impala_amd.learner import ImpalaAdam
from impala_amd.model import OBS_SHAPE

HIDDEN = 512
_ERR = "dqn_last_error"  # the DQN ABI reports through its own accessor (_lib.check)
# calls of dqn_train_step_replay made through DqnEngine.train_step_replay (this process)
REPLAY_STEP_CALLS = 0
# calls of dqn_train_step_replay_rows made through DqnEngine.train_step_replay_rows (this process)
REPLAY_ROWS_STEP_CALLS = 0


def net_specs(num_actions: int = 15) -> List[Tuple[str, Tuple[int, ...]]]:
    """state_dict keys / shapes of one DuellingAtariNetwork (models/models.py:44-87)."""
    return [
        ("body.body.0.weight", (32, 3, 8, 8)), ("body.body.0.bias", (32,)),
        ("body.body.2.weight", (64, 32, 4, 4)), ("body.body.2.bias", (64,)),
        ("body.body.4.weight", (64, 64, 3, 3)), ("body.body.4.bias", (64,)),
        ("q.body.0.weight", (1024,)), ("q.body.0.bias", (1024,)),
        ("q.body.1.weight", (HIDDEN, 1024)), ("q.body.1.bias", (HIDDEN,)),
        ("q.q.weight", (num_actions, HIDDEN)), ("q.q.bias", (num_actions,)),
        ("q.v.weight", (1, HIDDEN)), ("q.v.bias", (1,)),
    ]


def param_specs(num_actions: int = 15):
    """AtariDQNModel.state_dict(): the online net, then the target net."""
    s = net_specs(num_actions)
    return [("online_net." + k, v) for k, v in s] + [("target_net." + k, v) for k, v in s]


def param_count(num_actions: int = 15) -> int:
    """Parameters of one net (the online net alone): dqn_param_count."""
    return spec_count(net_specs(num_actions))


def default_config() -> _lib.DqnConfig:
    cfg = _lib.DqnConfig()
    check(lib().dqn_config_default(C.byref(cfg)), "dqn_config_default", _ERR)
    return cfg


def dqn_loss_head(adv, v, actions, targets, probabilities=None,
                  importance_sampling_exponent: float = 0.4) -> Dict[str, torch.Tensor]:
    """The DQN loss alone on given heads (``dqn_loss_head``): adv [N,A], v [N] fp32 on the GPU."""
    adv = adv.contiguous().float()
    N, A = adv.shape
    dev = adv.device
    out = dict(dadv=torch.empty_like(adv), dv=torch.empty(N, device=dev),
               priorities=torch.empty(N, device=dev), metrics=torch.empty(4, device=dev))
    v, targets = v.reshape(-1).contiguous().float(), targets.reshape(-1).contiguous().float()
    actions = actions.reshape(-1).contiguous().to(torch.int64)
    if probabilities is not None:
        probabilities = probabilities.reshape(-1).contiguous().float()
    check(lib().dqn_loss_head(_lib.ptr(adv), _lib.ptr(v), _lib.ptr(actions), _lib.ptr(targets),
                              _lib.ptr(probabilities), N, A, importance_sampling_exponent,
                              _lib.ptr(out["dadv"]), _lib.ptr(out["dv"]),
                              _lib.ptr(out["priorities"]), _lib.ptr(out["metrics"]),
                              _lib.stream_ptr(None)), "dqn_loss_head", _ERR)
    return out


class QEngine(_lib.NativeHandle):
    """What the handles of the two Q-learners share, ``DqnEngine`` and ``IqnEngine``
    (impala_amd/iqn.py): a subclass names its C-symbol prefix ``_abi`` and its error accessor;
    their entry points ``<abi>_refresh_weights``, ``_set_metrics``, ``_set_step`` and
    ``_sync_target`` take the same arguments."""
    _abi: str

    def _call(self, entry: str, *args) -> None:
        """``<abi>_<entry>(handle, *args)``, checked."""
        name = f"{self._abi}_{entry}"
        check(getattr(lib(), name)(self._h, *args), name, self._last_error)

    def _begin(self, model, batch_size: int, dtype: Optional[str], default_config):
        """The start of ``__init__``: the model, its device and the compute type; -> the ABI's
        default configuration with batch size, action count and dtype filled in."""
        self.model = model
        self.device = model.flat.device
        if self.device.type != "cuda":
            raise RuntimeError(f"the {self._abi.upper()} engine runs on the HIP path only (cuda device)")
        self.N, self.A = int(batch_size), model.action_dim
        cfg = default_config()
        cfg.batch_size, cfg.num_actions = self.N, self.A
        self.bf16 = (dtype or model.compute_dtype) == "bf16"
        cfg.dtype = _lib.IMPALA_DTYPE_BF16 if self.bf16 else _lib.IMPALA_DTYPE_F32
        return cfg

    def _fresh(self):
        if self._version != self.model._version:  # the flat buffers were written from outside
            self._call("refresh_weights", _lib.stream_ptr(None))
            self._version = self.model._version

    def bind_metrics(self, m: torch.Tensor) -> None:
        self.metrics = m
        self._call("set_metrics", _lib.ptr(m))

    def set_step(self, step: int) -> None:
        self._call("set_step", int(step), _lib.stream_ptr(None))

    def sync_target(self) -> None:
        self._fresh()
        self._call("sync_target", _lib.stream_ptr(None))

    def _eps_args(self, eps, n: int):
        """``act``'s exploration rate -> (eps_t [n] on the device or None, eps_all)."""
        if isinstance(eps, torch.Tensor) and eps.numel() > 1:
            eps_t = eps.reshape(-1).to(self.device, torch.float32).contiguous()
            if eps_t.numel() != n:
                raise ValueError("eps: one value, or one per frame")
            return eps_t, 0.0
        return None, float(eps.reshape(-1)[0]) if isinstance(eps, torch.Tensor) else float(eps)


class DqnEngine(QEngine):
    """One ``dqn_learner`` handle bound to an ``AtariDQNModel``'s flat buffers."""
    _abi, _destroy, _last_error = "dqn", "dqn_destroy", _ERR

    def __init__(self, model: "AtariDQNModel", batch_size: int = 512, dtype: Optional[str] = None,
                 lr: float = 6.25e-5, eps: float = 1e-4, betas=(0.9, 0.999),
                 max_grad_norm: float = 40.0, importance_sampling_exponent: float = 0.4,
                 inference_only: bool = False):
        cfg = self._begin(model, batch_size, dtype, default_config)
        cfg.lr, cfg.adam_eps = lr, eps
        cfg.adam_beta1, cfg.adam_beta2 = betas
        cfg.max_grad_norm = max_grad_norm
        cfg.importance_sampling_exponent = importance_sampling_exponent
        self._open("dqn_create", C.byref(cfg), self.device_index(self.device))
        n = model.flat.numel()
        self.inference_only = inference_only
        self.exp_avg = None if inference_only else torch.zeros(n, device=self.device)
        self.exp_avg_sq = None if inference_only else torch.zeros(n, device=self.device)
        self.metrics = torch.zeros(_lib.DQN_NUM_METRICS, device=self.device)
        sp = _lib.stream_ptr(None)
        check(lib().dqn_bind_state(self._h, _lib.ptr(model.flat),
                                   0 if inference_only else _lib.ptr(model.flat_grad),
                                   _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                   _lib.ptr(self.metrics), sp), "dqn_bind_state", _ERR)
        check(lib().dqn_bind_target(self._h, _lib.ptr(model.target_flat), sp), "dqn_bind_target", _ERR)
        self._version = model._version

    def forward(self, obs: torch.Tensor, target: bool = False) -> torch.Tensor:
        self._fresh()
        obs = obs.contiguous()
        n = obs.shape[0]
        q = torch.empty(n, self.A, device=self.device)
        check(lib().dqn_forward(self._h, _lib.ptr(obs), n, 1 if target else 0, _lib.ptr(q),
                                _lib.stream_ptr(None)), "dqn_forward", _ERR)
        return q

    def act(self, obs: torch.Tensor, eps, seed: int, counter: int):
        """-> (action [n] i64, q_pi [n], q_star [n], greedy [n] i64) on the device."""
        self._fresh()
        obs = obs.contiguous()
        n = obs.shape[0]
        eps_t, eps_all = self._eps_args(eps, n)
        a = torch.empty(n, dtype=torch.int64, device=self.device)
        g = torch.empty(n, dtype=torch.int64, device=self.device)
        q_pi, q_star = torch.empty(n, device=self.device), torch.empty(n, device=self.device)
        check(lib().dqn_act(self._h, _lib.ptr(obs), n, _lib.ptr(eps_t), eps_all, int(seed),
                            int(counter), _lib.ptr(a), _lib.ptr(q_pi), _lib.ptr(q_star),
                            _lib.ptr(g), _lib.stream_ptr(None)), "dqn_act", _ERR)
        return a, q_pi, q_star, g

    def train_step(self, obs, actions, targets, probabilities=None) -> torch.Tensor:
        """One learner step; returns the new priorities |err| [N] (device)."""
        return self._step("dqn_train_step", obs, actions, targets, probabilities)

    def compute_grads(self, obs, actions, targets, probabilities=None) -> torch.Tensor:
        """``train_step`` without clip and Adam (``dqn_compute_grads``): the pre-clip gradient in
        ``model.flat_grad`` and metrics q / target / priorities / loss; returns the priorities."""
        return self._step("dqn_compute_grads", obs, actions, targets, probabilities)

    # name -> (IMPALA_DBG_* id, element kind, shape of one frame): Engine.DEBUG_TENSORS with the
    # projection HIDDEN wide
    DEBUG_TENSORS = {
        "act1": (0, "T", (15, 15, 32)), "act2": (1, "T", (6, 6, 64)), "act3": (2, "T", (1024,)),
        "y": (3, "T", (1024,)), "h": (4, "T", (HIDDEN,)), "dz": (5, "T", (HIDDEN,)),
        "dact3": (6, "T", (1024,)), "dact2": (7, "T", (6, 6, 64)), "mask1": (8, "u32", (225,)),
        "lnstat": (9, "f32", (2,)), "zg": (10, "f32", (HIDDEN,)), "heads": (11, "f32", (16,)),
        "dy": (12, "f32", (1024,)),
    }

    def debug_tensor(self, name: str, frames: Optional[int] = None, target: bool = False):
        """``Engine.debug_tensor`` on this handle (``dqn_debug_read``; a host sync): the workspace
        tensor ``name`` as the last forward, act or step left it, a numpy array [frames, ...] in
        ``Engine.debug_tensor``'s layouts with h / dz / zg 512 wide.  The one workspace holds the
        net that ran last; ``target`` matters for "heads" alone, which then reads the target
        net's own buffer.  The step keeps its heads in LDS: "heads" is a forward's or act's."""
        if name not in self.DEBUG_TENSORS:
            raise ValueError(f"unknown debug tensor {name!r}: one of {sorted(self.DEBUG_TENSORS)}")
        which, kind, shape = self.DEBUG_TENSORS[name]
        n = self.N if frames is None else int(frames)
        if not 1 <= n <= self.N:
            raise ValueError(f"frames must be in [1, {self.N}]")
        return _lib.read_debug(
            lambda dst, nbytes, sp: check(lib().dqn_debug_read(self._h, 1 if target else 0, which, dst,
                                                               nbytes, sp), "dqn_debug_read", _ERR),
            kind, shape, n, self.bf16, self.device)

    def _step(self, entry: str, obs, actions, targets, probabilities) -> torch.Tensor:
        self._fresh()
        if obs.shape[0] != self.N:
            raise ValueError(f"batch of {obs.shape[0]} transitions on a handle of {self.N}")
        prio = torch.empty(self.N, device=self.device)
        keep = [obs.contiguous(), actions.reshape(-1).contiguous().to(torch.int64),
                targets.reshape(-1).contiguous().float(),
                None if probabilities is None else probabilities.reshape(-1).contiguous().to(
                    self.device, torch.float32)]
        b = _lib.DqnBatch(_lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]), _lib.ptr(keep[3]),
                          _lib.ptr(prio))
        check(getattr(lib(), entry)(self._h, C.byref(b), _lib.stream_ptr(None)), entry, _ERR)
        return prio

    @staticmethod
    def _own_replay(replay) -> None:
        """A ``dqn_replay`` handle and no other (a ``NativeQuantileReplay``'s is an ``iqn_replay``)."""
        if getattr(replay, "_abi", None) != "dqn_replay":
            raise TypeError("the DQN step samples a NativePrioritizedReplay (scalar targets)")

    def train_step_replay(self, replay: "NativePrioritizedReplay", seed: int, counter: int):
        """Sample ``batch_size`` rows of ``replay`` keyed by (seed, counter), one learner step on
        them and the priority update, as one ``dqn_train_step_replay`` call; returns the sampled
        keys [N] i64 and the new priorities [N] (device)."""
        global REPLAY_STEP_CALLS
        self._own_replay(replay)
        self._fresh()
        keys = torch.empty(self.N, dtype=torch.int64, device=self.device)
        prio = torch.empty(self.N, device=self.device)
        REPLAY_STEP_CALLS += 1
        check(lib().dqn_train_step_replay(self._h, replay._h, int(seed), int(counter),
                                          _lib.ptr(keys), _lib.ptr(prio),
                                          _lib.stream_ptr(None)), "dqn_train_step_replay", _ERR)
        return keys, prio

    def train_step_replay_rows(self, replay: "NativePrioritizedReplay", seed: int, counter: int):
        """``train_step_replay`` without the batch copy: one ``dqn_train_step_replay_rows`` call,
        the step reading the sampled rows of ``replay``'s ring in place.  Same outputs, bit for
        bit.  Until the current stream reaches the call's end, do not write ``replay``'s rows
        from another stream.  Raises ``_lib.Unsupported`` off the default kernel path."""
        global REPLAY_ROWS_STEP_CALLS
        self._own_replay(replay)
        self._fresh()
        keys = torch.empty(self.N, dtype=torch.int64, device=self.device)
        prio = torch.empty(self.N, device=self.device)
        REPLAY_ROWS_STEP_CALLS += 1
        check(lib().dqn_train_step_replay_rows(self._h, replay._h, int(seed), int(counter),
                                               _lib.ptr(keys), _lib.ptr(prio),
                                               _lib.stream_ptr(None)),
              "dqn_train_step_replay_rows", _ERR)
        return keys, prio


class QModel(FlatModule):
    """What ``AtariDQNModel`` and ``DistributionalAtariDQN`` (impala_amd/iqn.py) share: an online
    and a target net of the same ``specs``, one flat fp32 buffer each, and the lazily made
    inference engine.  A subclass gives ``_init_flat`` and ``_make_infer_engine``, and ends its
    ``__init__`` with ``reset_parameters(seed)``."""

    def __init__(self, observation_space, action_dim: int, specs, device, dtype: str):
        super().__init__()
        if tuple(observation_space) != OBS_SHAPE:
            raise ValueError(f"AtariBody requires observations of shape {OBS_SHAPE}")
        if not 1 <= action_dim <= 15:
            raise ValueError("action_dim must be in [1, 15]")
        self.action_dim = action_dim
        self.compute_dtype = dtype
        self._specs = specs
        self._attach_segments(torch.device(device))
        self._train_engine = None
        self._infer_engine = None
        self._act_seed = int.from_bytes(os.urandom(8), "little") >> 2
        self._act_calls = 0

    def _segment_table(self):
        return [("online_net", self._specs, "flat", "flat_grad"),
                ("target_net", self._specs, "target_flat", None)]

    def _init_flat(self) -> torch.Tensor:
        """Hook: the reference init of one net as a flat CPU tensor (consumes the global RNG)."""
        raise NotImplementedError

    def _make_infer_engine(self):
        """Hook: the engine ``forward`` / ``act`` run on while no learner has attached its own."""
        raise NotImplementedError

    # ---------------------------------------------------------------- parameters
    def reset_parameters(self, seed: Optional[int] = None) -> None:
        """Reference init (``_init_flat``, after seeding the global torch RNG with ``seed``); the
        target net is a copy of the online net."""
        if seed is not None:
            torch.manual_seed(int(seed))
        with torch.no_grad():
            self.flat.copy_(self._init_flat().to(self.flat.device))
            self.target_flat.copy_(self.flat)
        self.params_changed()

    def load_flat(self, flat, target=None) -> None:
        with torch.no_grad():
            self.flat.copy_(torch.as_tensor(np.asarray(flat, dtype=np.float32)).to(self.flat.device))
            if target is not None:
                self.target_flat.copy_(torch.as_tensor(np.asarray(target, dtype=np.float32)).to(
                    self.flat.device))
        self.params_changed()

    # ---------------------------------------------------------------- compute
    def _engine(self):
        if self._train_engine is not None:
            return self._train_engine
        if self._infer_engine is None:
            self._infer_engine = self._make_infer_engine()
        return self._infer_engine

    def sync_target_net(self) -> None:
        if self.flat.device.type == "cuda":
            self._engine().sync_target()
        else:
            with torch.no_grad():
                self.target_flat.copy_(self.flat)


class AtariDQNModel(QModel):
    """Drop-in for ``models.distributed_models.AtariDQNModel`` on an MI355X: the online and the
    target net are one flat fp32 buffer each, exposed as ``nn.Parameter`` views under the
    reference's ``state_dict`` names (``target_net.*`` with ``requires_grad=False``)."""

    def __init__(self, observation_space: Tuple[int, ...] = OBS_SHAPE, action_dim: int = 15,
                 device="cuda", seed: Optional[int] = None, dtype: str = "fp32"):
        super().__init__(observation_space, action_dim, net_specs(action_dim), device, dtype)
        self.reset_parameters(seed)

    def _init_flat(self) -> torch.Tensor:  # (the target a copy: distributed_models.py:77)
        return trunk_init_flat(HIDDEN, self.action_dim)

    def _make_infer_engine(self) -> DqnEngine:
        # the reference serves act() in batches of <= 128 (distributed_models.py:84)
        return DqnEngine(self, batch_size=128, inference_only=True)

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        """distributed_models.py:81-82 -> q [N, A] of the online net."""
        if obs.device.type != "cuda" or self.flat.device.type != "cuda":
            raise RuntimeError("AtariDQNModel.forward runs on the HIP path only (cuda device)")
        return self._engine().forward(obs)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, eps: torch.Tensor):
        """distributed_models.py:84-101 -> (action [N,1], q_pi [N,1], q_star [N,1]) on the CPU."""
        if self.flat.device.type != "cuda":
            raise RuntimeError("AtariDQNModel.act runs on the HIP path only (cuda device)")
        x = obs.to(self.flat.device)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        self._act_calls += 1
        a, q_pi, q_star, _ = self._engine().act(x, eps, seed=self._act_seed, counter=self._act_calls)
        return a.unsqueeze(-1).cpu(), q_pi.unsqueeze(-1).cpu(), q_star.unsqueeze(-1).cpu()

    def clone_to(self, device) -> "AtariDQNModel":
        return self._frozen_clone(AtariDQNModel(OBS_SHAPE, self.action_dim, device=device,
                                                dtype=self.compute_dtype))


def _replay_columns(items, width: int = 1):
    """``(s [n,3,64,64], a [n], target [n])`` from either form ``PrioritizedReplay.extend`` takes
    (``target [n, width]`` for a ring of ``width`` targets per transition)."""
    if isinstance(items, (list,)) and items and isinstance(items[0], (tuple, list)):
        cols = list(zip(*items))
        s = torch.cat([x if x.dim() == 4 else x.unsqueeze(0) for x in cols[0]])
        a = torch.cat([x.reshape(-1) for x in cols[1]])
        t = torch.cat([x.reshape(-1) if width == 1 else x.reshape(-1, width) for x in cols[2]])
        return s, a, t
    return items


class PrioritizedReplay:
    """A ring of flat transitions ``(s u8 [3,64,64], a i64, target f32)`` with a priority vector,
    on one device: ``P(i) ∝ priority_i ** priority_exponent`` (rlmeta's PrioritizedSampler as
    agents/dqn/builder.py:82-89 configures it).  ``sample`` is cumsum + searchsorted in torch.

    The returned ``probabilities`` are normalised (``p^α / Σ p^α``); whether rlmeta returns these
    or the raw ``p^α`` is not pinned, and the learner's weights ``w / max w`` do not depend on
    that scale.

    ``target_width=W > 1`` makes ``target`` a ``[capacity, W]`` array: one row of W quantile targets
    per transition (the distributional actor's, impala_amd/iqn.py); ``extend`` then takes
    ``target [n, W]`` and ``sample`` returns ``target [n, W]``.
    """

    def __init__(self, capacity: int, priority_exponent: float = 0.6, device="cuda",
                 seed: Optional[int] = None, obs_shape=OBS_SHAPE, target_width: int = 1):
        self.capacity = int(capacity)
        self.target_width = int(target_width)
        if self.target_width < 1:
            raise ValueError("target_width must be >= 1")
        self.alpha = float(priority_exponent)
        self.device = torch.device(device)
        self._alloc_ring(obs_shape)
        self._init_sampler()
        self.reset(seed)

    def _alloc_ring(self, obs_shape) -> None:
        cap, dev = self.capacity, self.device
        self.s = torch.zeros((cap,) + tuple(obs_shape), dtype=torch.uint8, device=dev)
        self.a = torch.zeros(cap, dtype=torch.int64, device=dev)
        shape = (cap,) if self.target_width == 1 else (cap, self.target_width)
        self.target = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.priorities = torch.zeros(cap, dtype=torch.float32, device=dev)

    def _init_sampler(self) -> None:
        self._ring_state = (0, 0)
        self._max_priority = torch.ones((), dtype=torch.float32, device=self.device)
        self._gen = torch.Generator(device=self.device)

    def reset(self, seed: Optional[int] = None) -> None:
        self._gen.manual_seed(0 if seed is None else int(seed))

    def _state(self) -> Tuple[int, int]:
        """-> (transitions stored, next slot written)."""
        return self._ring_state

    _size = property(lambda self: self._state()[0])
    _cursor = property(lambda self: self._state()[1])
    size = _size

    def __len__(self) -> int:
        return self._size

    def extend(self, items, priorities=None) -> torch.Tensor:
        """items: ``(s [n,3,64,64], a [n], target [n])`` or a list of per-transition triples (each
        with or without a leading dim).  Items without a priority get the current maximum.
        Returns the ring keys written."""
        s, a, t = _replay_columns(items, self.target_width)
        n = s.shape[0]
        if n > self.capacity:
            raise ValueError("more items than the ring holds")
        size, cursor = self._ring_state
        keys = (torch.arange(n, device=self.device) + cursor) % self.capacity
        self.s[keys] = s.to(self.device)
        self.a[keys] = a.reshape(-1).to(self.device, torch.int64)
        self.target[keys] = t.reshape((n,) + self.target.shape[1:]).to(self.device, torch.float32)
        if priorities is None:
            self.priorities[keys] = self._max_priority
        else:
            p = torch.as_tensor(priorities, dtype=torch.float32).reshape(-1).to(self.device)
            self.priorities[keys] = p
            self._max_priority = torch.maximum(self._max_priority, p.max())
        self._ring_state = (min(self.capacity, size + n), (cursor + n) % self.capacity)
        return keys

    async def async_extend(self, items, priorities=None):
        return self.extend(items, priorities)

    def probabilities(self) -> torch.Tensor:
        w = self.priorities[:self._size].double().pow(self.alpha)
        return (w / w.sum()).float()

    def sample(self, n: int):
        """-> (keys [n] i64, (s, a, target), probabilities [n]), drawn with replacement."""
        if self._size == 0:
            raise RuntimeError("sample from an empty replay")
        w = self.priorities[:self._size].double().pow(self.alpha)
        cdf = torch.cumsum(w, 0)
        u = torch.rand(n, generator=self._gen, device=self.device, dtype=torch.float64) * cdf[-1]
        keys = torch.searchsorted(cdf, u, right=True).clamp_(max=self._size - 1)
        probs = (w[keys] / cdf[-1]).float()
        return keys, (self.s[keys], self.a[keys], self.target[keys]), probs

    def update(self, keys, priorities) -> None:
        p = torch.as_tensor(priorities, dtype=torch.float32).reshape(-1).to(self.device)
        self.priorities[torch.as_tensor(keys).to(self.device)] = p
        # (a device-side running maximum: no host synchronisation in the step)
        self._max_priority = torch.maximum(self._max_priority, p.max())

    def async_update(self, keys, priorities):
        self.update(keys, priorities)
        return None

    def warm_up(self, learning_starts: Optional[int] = None, timeout: float = 240.0) -> None:
        """Block until ``learning_starts`` transitions are stored (rlmeta ReplayBuffer.warm_up);
        another thread's ``extend`` fills the ring meanwhile."""
        if not learning_starts:
            return
        need = min(int(learning_starts), self.capacity)
        deadline = time.monotonic() + timeout
        while self._size < need:
            if time.monotonic() > deadline:
                raise TimeoutError(f"replay warm_up: {self._size}/{need} after {timeout}s")
            time.sleep(0.01)


class NativePrioritizedReplay(PrioritizedReplay, _lib.NativeHandle):
    """``PrioritizedReplay`` on the library's ``dqn_replay`` (include/dqn_hip.h): the same
    constructor, attributes and methods, every one through a ``dqn_replay_*`` entry point.  The
    tensors ``s``, ``a``, ``target``, ``priorities`` are the bound ring arrays; the float64
    weights, their block sums and the running maximum priority belong to the library.

    ``sample`` draws by the header's contract from ``(seed, counter)``; the counter advances once
    per call (``reset(seed)`` rewinds it), so a seeded replay repeats its draws.
    ``extend_rollout`` is the actor's ``_async_make_replay`` (agents/dqn/learning.py:56-65).
    ``in_place=True`` asks ``ApexLearner`` to step on the sampled rows where they lie
    (``dqn_train_step_replay_rows``) instead of on a gathered copy.
    """
    _destroy, _last_error = "dqn_replay_destroy", _ERR
    _abi = "dqn_replay"  # the C-symbol prefix of the entry points shared with NativeQuantileReplay

    def _call(self, entry: str, *args) -> None:
        """``<abi>_<entry>(handle, *args)``, checked."""
        name = f"{self._abi}_{entry}"
        check(getattr(lib(), name)(self._h, *args), name, self._last_error)

    def __init__(self, capacity: int, priority_exponent: float = 0.6, device="cuda",
                 seed: Optional[int] = None, obs_shape=OBS_SHAPE, in_place: bool = False,
                 target_width: int = 1):
        if target_width != 1:
            raise NotImplementedError("NativePrioritizedReplay holds scalar targets only "
                                      "(target_width 1); PrioritizedReplay takes target_width > 1")
        self.in_place = bool(in_place)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("NativePrioritizedReplay lives on the HIP path only (cuda device)")
        if tuple(obs_shape) != OBS_SHAPE:
            raise ValueError(f"NativePrioritizedReplay stores observations of shape {OBS_SHAPE}")
        idx = self.device_index(device)
        self._open("dqn_replay_create", int(capacity), float(priority_exponent), idx)
        super().__init__(capacity, priority_exponent, torch.device("cuda", idx), seed)
        check(lib().dqn_replay_bind(self._h, _lib.ptr(self.s), _lib.ptr(self.a),
                                    _lib.ptr(self.target), _lib.ptr(self.priorities),
                                    self._stream()), "dqn_replay_bind", _ERR)

    def _init_sampler(self) -> None:
        """The weights, the running maximum priority, size and cursor belong to the library."""

    def _stream(self) -> int:
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, seed: Optional[int] = None) -> None:
        self._seed = (0 if seed is None else int(seed)) & (2 ** 64 - 1)
        self._counter = 0

    def _state(self) -> Tuple[int, int]:
        size, cursor = C.c_int64(), C.c_int64()
        self._call("state", C.byref(size), C.byref(cursor))
        return size.value, cursor.value

    def next_draw(self) -> Tuple[int, int]:
        """The (seed, counter) of the next sample; the counter advances."""
        c = self._counter
        self._counter += 1
        return self._seed, c

    def extend(self, items, priorities=None) -> torch.Tensor:
        s, a, t = _replay_columns(items)
        n = s.shape[0]
        if n > self.capacity:
            raise ValueError("more items than the ring holds")
        s = s.to(self.device, torch.uint8).contiguous()
        a = a.reshape(-1).to(self.device, torch.int64).contiguous()
        t = t.reshape(-1).to(self.device, torch.float32).contiguous()
        p = None
        if priorities is not None:
            p = torch.as_tensor(priorities, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if p.numel() != n:
                raise ValueError("one priority per item")
        if a.numel() != n or t.numel() != n:
            raise ValueError("s, a, target: one row per item")
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        check(lib().dqn_replay_extend(self._h, _lib.ptr(s), _lib.ptr(a), _lib.ptr(t), _lib.ptr(p),
                                      n, _lib.ptr(keys), self._stream()), "dqn_replay_extend", _ERR)
        return keys

    def extend_rollout(self, s, a, r, done, q_pi, q_star, n_step: int = 3,
                       gamma: float = 0.99) -> torch.Tensor:
        """One actor rollout of L steps -> L - 1 transitions with their n-step targets and initial
        priorities ``|target - q_pi|`` (``dqn_replay_extend_rollout``).  Returns the keys written."""
        L = s.shape[0]
        f32 = lambda x: x.reshape(-1).to(self.device, torch.float32).contiguous()
        s = s.to(self.device, torch.uint8).contiguous()
        a = a.reshape(-1).to(self.device, torch.int64).contiguous()
        d = done.reshape(-1).to(self.device).ne(0).to(torch.uint8).contiguous()
        r, q_pi, q_star = f32(r), f32(q_pi), f32(q_star)
        if not all(x.numel() == L for x in (a, r, d, q_pi, q_star)):
            raise ValueError("extend_rollout: every field has one entry per step")
        keys = torch.empty(max(L - 1, 0), dtype=torch.int64, device=self.device)
        check(lib().dqn_replay_extend_rollout(
            self._h, _lib.ptr(s), _lib.ptr(a), _lib.ptr(r), _lib.ptr(d), _lib.ptr(q_pi),
            _lib.ptr(q_star), L, int(n_step), float(gamma), _lib.ptr(keys), self._stream()),
            "dqn_replay_extend_rollout", _ERR)
        return keys

    def weights(self) -> torch.Tensor:
        """A copy of the library's float64 weights [capacity] (``priorities ** alpha``)."""
        return self._weights_and_max()[0]

    def max_priority(self) -> torch.Tensor:
        return self._weights_and_max()[1]

    def _weights_and_max(self):
        w = torch.empty(self.capacity, dtype=torch.float64, device=self.device)
        m = torch.empty(1, dtype=torch.float32, device=self.device)
        self._call("weights", _lib.ptr(w), _lib.ptr(m), self._stream())
        return w, m

    def probabilities(self) -> torch.Tensor:
        w = self.weights()[:self._size]
        return (w / w.sum()).float()

    def sample(self, n: int, gather: bool = True):
        """-> (keys [n] i64, (s, a, target), probabilities [n]); with ``gather=False`` the middle
        element is None and only keys and probabilities are produced."""
        if self._size == 0:
            raise RuntimeError("sample from an empty replay")
        n = int(n)
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        probs = torch.empty(n, dtype=torch.float32, device=self.device)
        rows = None
        if gather:
            rows = (torch.empty((n,) + OBS_SHAPE, dtype=torch.uint8, device=self.device),
                    torch.empty(n, dtype=torch.int64, device=self.device),
                    torch.empty(n, dtype=torch.float32, device=self.device))
        seed, counter = self.next_draw()
        out = rows or (None, None, None)
        check(lib().dqn_replay_sample(self._h, seed, counter, n, _lib.ptr(keys), _lib.ptr(probs),
                                      _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                      self._stream()), "dqn_replay_sample", _ERR)
        return keys, rows, probs

    def update(self, keys, priorities) -> None:
        p = torch.as_tensor(priorities, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        k = torch.as_tensor(keys).reshape(-1).to(self.device, torch.int64).contiguous()
        if k.numel() != p.numel():
            raise ValueError("one priority per key")
        for i in range(0, k.numel(), _lib.DQN_MAX_BATCH):  # one workgroup per call: <= 4096 keys
            kc, pc = k[i:i + _lib.DQN_MAX_BATCH], p[i:i + _lib.DQN_MAX_BATCH]
            self._call("update", _lib.ptr(kc), _lib.ptr(pc), kc.numel(), self._stream())


class ApexLearner(Learner):
    """agents/dqn/learning.py:97-191 with ``_train_step`` as one ``dqn_train_step`` call, or --
    over a ``NativePrioritizedReplay`` -- sample, step and priority update as one
    ``dqn_train_step_replay`` call (``last_keys`` / ``last_priorities`` then hold its outputs)."""

    def __init__(self, model, replay_buffer, optimizer=None, batch_size: int = 512,
                 max_grad_norm: float = 40.0, importance_sampling_exponent: float = 0.4,
                 target_sync_period: int = 2500, learning_starts: Optional[int] = None,
                 model_push_period: int = 10, dtype: Optional[str] = None) -> None:
        self._model = model
        self._replay_buffer = replay_buffer
        self._optimizer = optimizer = ImpalaAdam.of(optimizer, lr=6.25e-5, eps=1e-4)
        self._batch_size = batch_size
        self._max_grad_norm = max_grad_norm
        self._importance_sampling_exponent = importance_sampling_exponent
        self._target_sync_period = target_sync_period
        self._learning_starts = learning_starts
        self._model_push_period = model_push_period
        self._step_counter = 0
        self._update_priorities_future = None
        self._device = model.flat.device
        self.can_train = False
        self._engine = self._make_engine(model, batch_size, dtype)
        model._train_engine = self._engine

    def _make_engine(self, model, batch_size, dtype):
        """The training engine bound to ``model`` (``DistributionalApexLearner`` makes an IQN one)."""
        o = self._optimizer
        return DqnEngine(model, batch_size=batch_size, dtype=dtype, lr=o.lr, eps=o.eps, betas=o.betas,
                         max_grad_norm=self._max_grad_norm,
                         importance_sampling_exponent=self._importance_sampling_exponent)

    @property
    def engine(self) -> DqnEngine:
        return self._engine

    @property
    def samples_per_step(self) -> int:
        return self._batch_size

    def prepare(self):  # learning.py:154-157
        if not self.can_train:
            self._replay_buffer.warm_up(self._learning_starts)
        self.can_train = True

    def train_step(self):
        """Sample, one device step, then the periodic target sync and weight push.  The ``debug/*``
        keys are the reference learner's; the times are host wall-clock milliseconds and the two
        rates are transitions per second.  Over a ``NativePrioritizedReplay`` the sample is part
        of the one call, and ``debug/replay_sample_per_second`` and ``debug/forward_dt`` are
        reported over the whole call."""
        clock = time.perf_counter
        begin = clock()
        if isinstance(self._replay_buffer, NativePrioritizedReplay):
            metrics = self._train_step_replay()
            sampled = stepped = clock()
            forward_begin = begin
        else:
            keys, batch, probabilities = self._replay_buffer.sample(self._batch_size)
            batch = tuple(x.to(self._device) for x in batch)
            sampled = forward_begin = clock()
            metrics = self._train_step(keys, batch, probabilities)
            stepped = clock()
        self._step_counter += 1

        def every(period, action):  # -> ms spent in `action` when this step is a multiple of period
            if self._step_counter % period:
                return 0.0
            t = clock()
            action()
            return (clock() - t) * 1e3

        sync_ms = every(self._target_sync_period, self._model.sync_target_net)
        push_ms = every(self._model_push_period, self._model.push)
        metrics.update({
            "debug/replay_sample_per_second": self._batch_size / max(sampled - begin, 1e-9),
            "debug/gradient_per_second": self._batch_size / max(stepped - begin, 1e-9),
            "debug/forward_dt": (stepped - forward_begin) * 1e3,
            "debug/target_sync_time": sync_ms,
            "debug/update_time": push_ms,
            "debug/total_time": (clock() - begin) * 1e3,
        })
        return metrics

    def _train_step_replay(self) -> Dict[str, torch.Tensor]:
        e = self._engine
        m = torch.empty(_lib.DQN_NUM_METRICS, dtype=torch.float32, device=e.device)
        e.bind_metrics(m)
        rb = self._replay_buffer
        seed, counter = rb.next_draw()
        out = None
        if rb.in_place:
            try:
                out = e.train_step_replay_rows(rb, seed, counter)
            except _lib.Unsupported:  # refused before any launch: the gather path, from now on
                rb.in_place = False
        self.last_keys, self.last_priorities = out or e.train_step_replay(rb, seed, counter)
        v = m.unbind(0)
        out = {name: v[i] for name, i in _lib.DQN_METRIC_SLOTS}
        out["debug/priority_update_time"] = 0
        return out

    def _train_step(self, keys, batch, probabilities) -> Dict[str, torch.Tensor]:  # :159-191
        e = self._engine
        m = torch.empty(_lib.DQN_NUM_METRICS, dtype=torch.float32, device=e.device)
        e.bind_metrics(m)
        obs, action, target = batch
        priorities = e.train_step(obs, action, target, probabilities)
        priority_update_time = 0
        if isinstance(self._replay_buffer, PrioritizedReplay):
            self._replay_buffer.update(keys, priorities)  # stays on the device
        else:
            if self._update_priorities_future is not None:
                t0 = time.perf_counter()
                self._update_priorities_future.wait()
                priority_update_time = (time.perf_counter() - t0) * 1000
            self._update_priorities_future = self._replay_buffer.async_update(keys, priorities.cpu())
        v = m.unbind(0)  # device scalars; float(v) synchronises lazily
        out = {name: v[i] for name, i in _lib.DQN_METRIC_SLOTS}
        out["debug/priority_update_time"] = priority_update_time
        return out


class ApexActor(Actor):
    """``ApexActor`` (agents/dqn/learning.py:17-65) for in-process actors: it collects
    ``(obs, action, reward, done, q_pi, q_star)`` per step and hands every ``rollout_length`` steps
    to the replay's ``extend_rollout``, whose kernel computes the n-step targets and the initial
    priorities of the rollout's ``rollout_length - 1`` transitions.  Each rollout stands alone."""

    def __init__(self, model, replay_buffer=None, eps: float = 0.4, n_step: int = 3,
                 rollout_length: int = 100, gamma: float = 0.99):
        self._model = model
        self._replay_buffer = replay_buffer
        self._eps = torch.tensor((eps,), dtype=torch.float32)
        self._n_step = n_step
        self._rollout_length = rollout_length
        self._gamma = gamma
        self._trajectory = []
        self._last_transition = None

    @staticmethod
    def _star(v) -> torch.Tensor:
        """One step's bootstrap value as it is stacked (a scalar; the distributional actor's: a row)."""
        return torch.as_tensor(v, dtype=torch.float32).reshape(())

    def act(self, timestep):  # learning.py:31-33
        obs = timestep.observation if hasattr(timestep, "observation") else timestep[0]
        action, q, v = self._model.act(obs, self._eps)
        return action, {"q": q, "v": v}

    async def async_act(self, timestep):
        return self.act(timestep)

    def observe_init(self, timestep) -> None:
        if self._replay_buffer is None:
            return
        self._last_transition = timestep

    async def async_observe_init(self, timestep) -> None:
        self.observe_init(timestep)

    def observe(self, action, next_timestep) -> None:  # learning.py:40-48
        if self._replay_buffer is None:
            return
        lt = self._last_transition
        obs = lt.observation if hasattr(lt, "observation") else lt[0]
        act, info = action
        reward, done = next_timestep[1], next_timestep[2]
        f32 = lambda x: torch.as_tensor(x, dtype=torch.float32).reshape(())
        self._trajectory.append((torch.as_tensor(obs).reshape(OBS_SHAPE),
                                 torch.as_tensor(act).reshape(()), f32(reward),
                                 torch.as_tensor(done).reshape(()), f32(info["q"]),
                                 self._star(info["v"])))
        self._last_transition = next_timestep
        if len(self._trajectory) == self._rollout_length:
            self.update()

    async def async_observe(self, action, next_timestep) -> None:
        self.observe(action, next_timestep)

    def update(self) -> None:  # learning.py:50-65
        """The stacked steps into the replay (a rollout of L steps makes L - 1 transitions, so
        fewer than 2 steps make none and stay pending)."""
        if self._replay_buffer is None or len(self._trajectory) < 2:
            return
        s, a, r, d, q_pi, q_star = (torch.stack(x) for x in zip(*self._trajectory))
        self._trajectory = []
        self._replay_buffer.extend_rollout(s, a.to(torch.int64), r, d, q_pi, q_star, self._n_step,
                                           self._gamma)

    async def async_update(self) -> None:
        self.update()


class ApexActorFactory:
    """Actor index -> an ``ApexActor`` exploring at ``eps_func(index)`` (the reference's
    ApexDQNAgentFactory)."""

    def __init__(self, model, eps_func, rb=None, **kwargs):
        self._model, self._eps_func, self._rb, self._kwargs = model, eps_func, rb, kwargs

    def __call__(self, index: int) -> Actor:
        return ApexActor(self._model, self._rb, eps=self._eps_func(index), **self._kwargs)


class ConstantEpsFunc:
    """Actor index -> the same exploration rate for every actor (the evaluation actors)."""

    def __init__(self, eps: float) -> None:
        self.eps = float(eps)

    def __call__(self, index: int) -> float:
        return self.eps


class FlexibleEpsFunc:
    """Actor index -> Ape-X's per-actor exploration rate: ``eps ** (1 + alpha * i / (num - 1))`` for
    actor i of ``num``, so actor 0 explores at ``eps`` and the last at ``eps ** (1 + alpha)``; one
    actor alone gets ``eps``.  Signature as the reference's helper of the same name."""

    def __init__(self, eps: float, num: int, alpha: float = 7.0) -> None:
        self.eps, self.num, self.alpha = float(eps), int(num), float(alpha)

    def __call__(self, index: int) -> float:
        frac = index / (self.num - 1) if self.num > 1 else 0.0
        return self.eps ** (1.0 + self.alpha * frac)


class ApexDQNBuilder(Builder):
    """agents/dqn/builder.py:76-120 on the HIP learner."""

    def make_replay(self, native: bool = False, in_place: bool = False):  # builder.py:82-89
        """``native=True``: the ring on the library's ``dqn_replay`` (NativePrioritizedReplay);
        ``in_place=True`` (native only): the learner steps on the sampled rows where they lie."""
        if in_place and not native:
            raise ValueError("in_place needs the native replay (native=True)")
        kw = dict(priority_exponent=float(self.cfg.agent.priority_exponent),
                  device=self.cfg.distributed.train_device, seed=self.cfg.training.seed)
        if native:
            return NativePrioritizedReplay(self.cfg.agent.replay_buffer_size, in_place=in_place, **kw)
        return PrioritizedReplay(self.cfg.agent.replay_buffer_size, **kw)

    def make_actor(self, model, rb=None, deterministic: bool = False):  # builder.py:91-97
        if deterministic:
            eps_func = ConstantEpsFunc(self.cfg.agent.eval_eps)
        else:
            eps_func = FlexibleEpsFunc(self.cfg.agent.train_eps, self.cfg.training.num_rollouts)
        if rb is not None and not hasattr(rb, "extend_rollout"):
            # ApexActor's n-step targets and initial priorities are the native replay's ingest
            # (dqn_replay_extend_rollout); the plain PrioritizedReplay has no such entry
            raise NotImplementedError(
                "ApexActor hands whole rollouts to the replay's extend_rollout, the n-step ingest "
                "of NativePrioritizedReplay (make_replay(native=True)); this replay has none")
        return ApexActorFactory(model, eps_func, rb, n_step=int(self.cfg.agent.n_step),
                                rollout_length=int(self.cfg.agent.rollout_length))

    def learner_kwargs(self) -> dict:
        """make_learner's constructor arguments (builder.py:99-110): Adam from
        cfg.agent.optimizer and learning_starts; every other argument keeps its default."""
        return dict(optimizer=ImpalaAdam(lr=float(self.cfg.agent.optimizer.lr),
                                         eps=float(self.cfg.agent.optimizer.eps)),
                    learning_starts=self.cfg.agent.learning_starts)

    def make_learner(self, model, rb):
        return ApexLearner(self._learner_model if model is None else model, replay_buffer=rb,
                           **self.learner_kwargs())

    def make_network(self, env_spec=None):  # builder.py:112-120
        obs_shape, n_act = OBS_SHAPE, 15
        if env_spec is not None:
            obs_shape = tuple(env_spec.observation_space.shape)
            n_act = int(env_spec.action_space.n)
        model = AtariDQNModel(obs_shape, n_act, device=self.cfg.distributed.train_device)
        self._learner_model = model
        self._actor_model = model.clone_to(self.cfg.distributed.infer_device)
        model.downstream = self._actor_model
        return model
