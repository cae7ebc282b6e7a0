"""Actor-critic model whose parameters live in ONE flat fp32 buffer (state_dict order).

Mirrors ``models/distributed_models.py:12-32`` (``AtariPPOModel``: ``forward`` and the batched
``act``) over ``models/models.py:61-76`` / ``models/common.py:108-126`` (NatureCNN actor-critic).
Every parameter is a ``torch.nn.Parameter`` VIEW into ``self.flat`` (and every ``.grad`` a view
into ``self.flat_grad``) so that ``state_dict()`` / ``load_state_dict()`` / ``torch.save`` keep
the reference's key names, while the HIP library reads and updates the whole model through one
pointer.  The compute path is the HIP library only: ``forward`` on a non-GPU tensor raises.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np
import torch

# (the helpers lived here before flat.py: re-exported for code that imports them from here)
from impala_amd.flat import (ENGINE_ATTRS, FlatModule, _Node, layer_init_truncated,  # noqa: F401
                             picklable_state, rebind_views, trunk_init_flat)

OBS_SHAPE = (3, 64, 64)


def param_specs(num_actions: int = 15) -> List[Tuple[str, Tuple[int, ...]]]:
    """state_dict keys/shapes of the reference AtariPPOModel."""
    return [
        ("model.body.body.0.weight", (32, 3, 8, 8)),
        ("model.body.body.0.bias", (32,)),
        ("model.body.body.2.weight", (64, 32, 4, 4)),
        ("model.body.body.2.bias", (64,)),
        ("model.body.body.4.weight", (64, 64, 3, 3)),
        ("model.body.body.4.bias", (64,)),
        ("model.projection.0.weight", (1024,)),
        ("model.projection.0.bias", (1024,)),
        ("model.projection.1.weight", (256, 1024)),
        ("model.projection.1.bias", (256,)),
        ("model.actor.weight", (num_actions, 256)),
        ("model.actor.bias", (num_actions,)),
        ("model.critic.weight", (1, 256)),
        ("model.critic.bias", (1,)),
    ]


def param_count(num_actions: int = 15) -> int:
    return sum(int(np.prod(s)) for _, s in param_specs(num_actions))


class AtariPPOModel(FlatModule):
    """Drop-in for ``models.distributed_models.AtariPPOModel`` on an MI355X.

    ``forward(obs_u8[N,3,64,64]) -> (logits[N,A], v[N,1])`` through ``impala_forward``;
    ``act(obs, deterministic)`` as the reference's remote batched act (``:21-32``).
    """

    def __init__(self, observation_space: Tuple[int, ...] = OBS_SHAPE, action_dim: int = 15,
                 device="cuda", seed: Optional[int] = None, dtype: str = "fp32"):
        super().__init__()
        if tuple(observation_space) != OBS_SHAPE:
            # models/common.py:124-126 hard-codes output_dim 1024 => 64x64x3 only
            raise ValueError(f"AtariBody requires observations of shape {OBS_SHAPE}")
        if not 1 <= action_dim <= 15:
            raise ValueError("action_dim must be in [1, 15]")
        self.action_dim = action_dim
        self.compute_dtype = dtype
        self._specs = param_specs(action_dim)
        self._views, = self._attach_segments(torch.device(device))
        self._train_engine = None  # Engine whose kernel-layout weights track every update
        self._infer_engine = None  # lazily created inference-only Engine
        # act() sampling stream; drawn outside torch's generator so seeded inits are unchanged
        self._act_seed = int.from_bytes(os.urandom(8), "little") >> 2
        self.reset_parameters(seed)

    def _segment_table(self):
        return [(None, self._specs, "flat", "flat_grad")]

    # ---------------------------------------------------------------- parameters
    def reset_parameters(self, seed: Optional[int] = None) -> None:
        """Reference init, bit for bit (``trunk_init_flat``).  ``seed`` seeds the global torch RNG
        first, as main.py:57-58 does before ``make_network``."""
        if seed is not None:
            torch.manual_seed(int(seed))
        with torch.no_grad():
            self.flat.copy_(trunk_init_flat(256, self.action_dim).to(self.flat.device))
        self.params_changed()

    def load_flat(self, flat) -> None:
        with torch.no_grad():
            self.flat.copy_(torch.as_tensor(np.asarray(flat, dtype=np.float32)).to(self.flat.device))
        self.params_changed()

    # ---------------------------------------------------------------- compute
    def _engine(self):
        if self._train_engine is not None:
            return self._train_engine
        if self._infer_engine is None:
            from impala_amd.engine import Engine
            # the reference serves act() in batches of <= 128 (distributed_models.py:21)
            self._infer_engine = Engine(self, batch_size=2, rollout_length=64, inference_only=True)
        return self._infer_engine

    def forward(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """models/distributed_models.py:17-19 -> (logits [N,A], v [N,1])."""
        if obs.device.type != "cuda" or self.flat.device.type != "cuda":
            raise RuntimeError("AtariPPOModel.forward runs on the HIP path only (cuda device)")
        return self._engine().forward(obs)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, deterministic_policy: torch.Tensor):
        """models/distributed_models.py:21-32: sample a ~ softmax(logits) (or argmax when
        deterministic); returns (action [N,1], logits [N,A], v [N,1]) on the CPU."""
        if self.flat.device.type != "cuda":
            raise RuntimeError("AtariPPOModel.act runs on the HIP path only (cuda device)")
        x = obs.to(self.flat.device)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        # forward + argmax / softmax draw in one HIP call (impala_act); each call draws fresh
        self._act_calls = getattr(self, "_act_calls", 0) + 1
        action, logits, v = self._engine().act(x, deterministic_policy, seed=self._act_seed,
                                               counter=self._act_calls)
        # the three results to the host with one wait: asynchronous copies into page-locked
        # tensors (torch's caching host allocator), then a single stream synchronize -- instead
        # of three synchronous .cpu() round trips
        out = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (action, logits, v)]
        for h, t in zip(out, (action, logits, v)):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.flat.device).synchronize()
        return tuple(out)

    def clone_to(self, device) -> "AtariPPOModel":
        return self._frozen_clone(AtariPPOModel(OBS_SHAPE, self.action_dim, device=device,
                                                dtype=self.compute_dtype))
