"""The IMPALA ResNet actor-critic on the HIP library: the reference's
``AtariActorCritic`` (models/models.py:61-76) with ``ImpalaCNNLarge`` (models/common.py:11-83) as
its body -- the actor path, ``forward`` and ``act``, and the backward pass:
``forward_train`` returns outputs attached to the autograd graph, and ``loss.backward()`` runs
``resnet_backward`` into ``model.flat_grad``, in fp32 or (``train_dtype="bf16"``) in bf16.  Every compute entry is one call of
include/resnet_hip.h; the compute path is the HIP library only.  ``ImpalaResNetLearner`` is the
learner: one ``resnet_train_step`` a step (``conf/agent/impala_resnet.yaml``).
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from impala_amd import _lib
from impala_amd._lib import check, lib
from impala_amd.core import Learner
from impala_amd.flat import FlatModule, layer_init_truncated, spec_count
from impala_amd.model import OBS_SHAPE

FEATURES, HIDDEN = 2048, 256
_ERR = "resnet_last_error"
# (in channels, out channels) of the three ImpalaCNNBlocks
STAGES = ((3, 16), (16, 32), (32, 32))
_CONVS = ("conv", "res_block0.conv0", "res_block0.conv1", "res_block1.conv0", "res_block1.conv1")


def param_specs(num_actions: int = 15) -> List[Tuple[str, Tuple[int, ...]]]:
    """state_dict keys / shapes of AtariActorCritic over ImpalaCNNLarge, in order."""
    specs = []
    for s, (cin, c) in enumerate(STAGES):
        for j, name in enumerate(_CONVS):
            k = f"model.body.body.{s}.{name}"
            specs += [(k + ".weight", (c, cin if j == 0 else c, 3, 3)), (k + ".bias", (c,))]
    return specs + [
        ("model.projection.0.weight", (FEATURES,)), ("model.projection.0.bias", (FEATURES,)),
        ("model.projection.1.weight", (HIDDEN, FEATURES)), ("model.projection.1.bias", (HIDDEN,)),
        ("model.actor.weight", (num_actions, HIDDEN)), ("model.actor.bias", (num_actions,)),
        ("model.critic.weight", (1, HIDDEN)), ("model.critic.bias", (1,)),
    ]


def param_count(num_actions: int = 15) -> int:
    return spec_count(param_specs(num_actions))


def resnet_init_flat(action_dim: int) -> torch.Tensor:
    """Reference init as one flat CPU tensor: the layers are constructed in the reference's order,
    each consuming the global RNG as there.  The body's convolutions keep torch's default
    ``Conv2d`` init (the reference's ``scale`` argument is unused); the projection and the heads
    take ``layer_init_truncated``; LayerNorm stays (1, 0)."""
    trunc = layer_init_truncated
    layers = [nn.Conv2d(cin if j == 0 else c, c, 3, padding=1)
              for cin, c in STAGES for j in range(len(_CONVS))]
    layers += [nn.LayerNorm(FEATURES), trunc(nn.Linear(FEATURES, HIDDEN), FEATURES),
               trunc(nn.Linear(HIDDEN, action_dim), HIDDEN), trunc(nn.Linear(HIDDEN, 1), HIDDEN)]
    return torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])


def _stage_shape(i: int) -> Tuple[int, int, int]:
    return (32, 32, 16) if i < 5 else (16, 16, 32) if i < 10 else (8, 8, 32)


def default_config() -> _lib.ResnetConfig:
    cfg = _lib.ResnetConfig()
    check(lib().resnet_config_default(C.byref(cfg)), "resnet_config_default", _ERR)
    return cfg


class ResnetEngine(_lib.NativeHandle):
    """One ``resnet_actor`` handle bound to an ``ImpalaResNetModel``'s flat buffer."""
    _destroy, _last_error = "resnet_destroy", _ERR
    # name -> (debug tensor id, element kind, shape of one frame); the body's stage tensors are
    # channels-last [H, H, C], "y" in the kernel order p*32 + c
    DEBUG_TENSORS = dict(
        [(f"s{i}", (i, "T", _stage_shape(i))) for i in range(15)],
        y=(_lib.RESNET_DBG_Y, "T", (FEATURES,)), h=(_lib.RESNET_DBG_H, "T", (HIDDEN,)),
        heads=(_lib.RESNET_DBG_HEADS, "f32", (16,)))
    # a ``train=True`` engine after a ``backward``: the gradient at every convolution's output (at its
    # pool's output for 0, 5, 10), at y and at the pre-GELU z, the pools' winning taps, the LayerNorm's
    # (mean, rstd); "part" is not per frame: the whole [8, batch_size, 256] (``frames=None``)
    TRAIN_TENSORS = dict(
        [(f"g{i}", (_lib.RESNET_DBG_GRAD0 + i, "T", _stage_shape(i))) for i in range(15)],
        gy=(_lib.RESNET_DBG_GY, "f32", (FEATURES,)), gz=(_lib.RESNET_DBG_GZ, "f32", (HIDDEN,)),
        amax=(_lib.RESNET_DBG_AMAX, "u32", ((16384 + 8192 + 2048) // 4,)),
        lnstat=(_lib.RESNET_DBG_LNSTAT, "f32", (2,)), part=(_lib.RESNET_DBG_PART, "f32", (8 * HIDDEN,)))

    def __init__(self, model: "ImpalaResNetModel", batch_size: int = 128,
                 dtype: Optional[str] = None, debug: bool = False, train: bool = False):
        dtype = dtype or model.compute_dtype
        if dtype not in ("fp32", "bf16"):
            raise ValueError("dtype: 'fp32' or 'bf16'")
        self.model, self.device = model, model.flat.device
        if self.device.type != "cuda":
            raise RuntimeError("ResnetEngine runs on the HIP path only (cuda device)")
        if lib().resnet_abi_version() != _lib.RESNET_ABI_VERSION:
            raise RuntimeError("resnet ABI version mismatch (rebuild: python -m impala_amd.build)")
        cfg = default_config()
        cfg.batch_size, cfg.num_actions = int(batch_size), model.action_dim
        cfg.dtype, cfg.debug, cfg.train = (1 if dtype == "bf16" else 0), int(bool(debug)), int(bool(train))
        cfg.train_dtype = cfg.dtype if train else 0  # forward_train is forward, the same bits
        self.N, self.A, self.bf16 = cfg.batch_size, cfg.num_actions, dtype == "bf16"
        self._open("resnet_create", C.byref(cfg), self.device_index(self.device))
        check(lib().resnet_bind_params(self._h, _lib.ptr(model.flat)), "resnet_bind_params", _ERR)
        self._version = None

    def _fresh(self) -> None:
        """Re-pack the kernel-layout weights if the flat parameters were written."""
        if self._version != self.model._version:
            check(lib().resnet_refresh_weights(self._h, _lib.stream_ptr(None)),
                  "resnet_refresh_weights", _ERR)
            self._version = self.model._version

    def _outputs(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return torch.empty(n, self.A, device=self.device), torch.empty(n, 1, device=self.device)

    def forward(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (logits [n, A], values [n, 1]) on the device."""
        self._fresh()
        obs = obs.contiguous()
        n = obs.shape[0]
        logits, values = self._outputs(n)
        check(lib().resnet_forward(self._h, _lib.ptr(obs), n, _lib.ptr(logits), _lib.ptr(values),
                                   _lib.stream_ptr(None)), "resnet_forward", _ERR)
        return logits, values

    def forward_train(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``forward``'s outputs, the same bits, with what ``backward`` needs left in the handle
        (an engine created with ``train=True``)."""
        self._fresh()
        self._obs = obs.contiguous()  # the backward reads the frames again (the stem's gradient)
        n = self._obs.shape[0]
        logits, values = self._outputs(n)
        check(lib().resnet_forward_train(self._h, _lib.ptr(self._obs), n, _lib.ptr(logits),
                                         _lib.ptr(values), _lib.stream_ptr(None)),
              "resnet_forward_train", _ERR)
        return logits, values

    def backward(self, dlogits: torch.Tensor, dvalues: torch.Tensor,
                 out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
        """The gradient of ``sum(dlogits * logits) + sum(dvalues * values)`` of the last
        ``forward_train`` with respect to the flat parameters, written (or, with ``accumulate``,
        added) to ``out`` [param_count] fp32 (a new buffer without one)."""
        if self._version != self.model._version:
            raise RuntimeError("the parameters changed since forward_train")
        obs = getattr(self, "_obs", None)
        if obs is None:
            raise RuntimeError("backward needs a forward_train first")
        n = obs.shape[0]
        dl = dlogits.to(self.device, torch.float32).reshape(n, self.A).contiguous()
        dv = dvalues.to(self.device, torch.float32).reshape(n).contiguous()
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs the buffer to add to")
            out = torch.empty(self.model.flat.numel(), device=self.device)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != self.model.flat.numel():
            raise ValueError("out: a contiguous fp32 tensor of param_count elements")
        check(lib().resnet_backward(self._h, _lib.ptr(obs), n, _lib.ptr(dl), _lib.ptr(dv), _lib.ptr(out),
                                    int(bool(accumulate)), _lib.stream_ptr(None)), "resnet_backward", _ERR)
        return out

    def act(self, obs: torch.Tensor, deterministic, seed: int, counter: int):
        """-> (action [n, 1] i64, logits [n, A], values [n, 1]) on the device; ``deterministic``
        a bool for every frame or a tensor of one flag per frame."""
        self._fresh()
        obs = obs.contiguous()
        n = obs.shape[0]
        det, det_all = None, 0
        if torch.is_tensor(deterministic) and deterministic.numel() > 1:
            det = deterministic.reshape(-1).to(self.device).ne(0).to(torch.uint8).contiguous()
            if det.numel() != n:
                raise ValueError("deterministic: one flag per frame")
        else:
            det_all = int(bool(deterministic.item() if torch.is_tensor(deterministic) else deterministic))
        action = torch.empty(n, 1, dtype=torch.int64, device=self.device)
        logits, values = self._outputs(n)
        check(lib().resnet_act(self._h, _lib.ptr(obs), n, _lib.ptr(det), det_all, int(seed),
                               int(counter), _lib.ptr(action), _lib.ptr(logits), _lib.ptr(values),
                               _lib.stream_ptr(None)), "resnet_act", _ERR)
        return action, logits, values

    # ------------------------------------------------------------------ the learner step
    def step_init(self, batch_size: int, rollout_length: int, *, lr: float = 1e-4, eps: float = 1e-5,
                  betas: Tuple[float, float] = (0.9, 0.999), max_grad_norm: float = 0.5,
                  entropy_coeff: float = 0.01, vtrace_lambda: float = 1.0, clip_rho: float = 1.0,
                  clip_pg_rho: float = 1.0, vtrace_grad_mode=None) -> None:
        """Set the engine (``train=True``) up for steps on ``batch_size`` trajectories of
        ``rollout_length`` frames (``resnet_step_init``) and bind the state the steps update: the
        model's ``flat`` and ``flat_grad``, and ``exp_avg`` / ``exp_avg_sq`` / ``metrics`` made here."""
        cfg = _lib.ResnetStepConfig()
        check(lib().resnet_step_config_default(C.byref(cfg)), "resnet_step_config_default", _ERR)
        cfg.batch_size, cfg.rollout_length = int(batch_size), int(rollout_length)
        cfg.lr, cfg.adam_eps, (cfg.adam_beta1, cfg.adam_beta2) = lr, eps, betas
        cfg.max_grad_norm, cfg.entropy_coeff, cfg.vtrace_lambda = max_grad_norm, entropy_coeff, vtrace_lambda
        cfg.clip_rho_threshold, cfg.clip_pg_rho_threshold = clip_rho, clip_pg_rho
        cfg.vtrace_grad_mode = _lib.vtrace_grad_mode(vtrace_grad_mode)
        check(lib().resnet_step_init(self._h, C.byref(cfg)), "resnet_step_init", _ERR)
        self.B, self.T = cfg.batch_size, cfg.rollout_length
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.model.flat), torch.zeros_like(self.model.flat)
        self.bind_metrics(torch.zeros(_lib.NUM_METRICS, device=self.device))

    def bind_metrics(self, metrics: torch.Tensor) -> None:
        """The vector [NUM_METRICS] the following steps write (host-side only: ``resnet_bind_state``)."""
        self.metrics = metrics
        check(lib().resnet_bind_state(self._h, _lib.ptr(self.model.flat), _lib.ptr(self.model.flat_grad),
                                      _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(metrics),
                                      _lib.stream_ptr(None)), "resnet_bind_state", _ERR)

    def set_step(self, step: int) -> None:
        check(lib().resnet_set_step(self._h, int(step), _lib.stream_ptr(None)), "resnet_set_step", _ERR)

    def debug_vtrace(self, on: bool = True) -> Optional[torch.Tensor]:
        """With ``on``, every following ``loss_head`` also writes its adv, err, q [3, B, T-1] and rho
        [B, T] into the returned flat tensor (``resnet_set_debug_vtrace``)."""
        self._vt = torch.zeros(3 * self.B * (self.T - 1) + self.B * self.T, device=self.device) if on else None
        check(lib().resnet_set_debug_vtrace(self._h, _lib.ptr(self._vt)), "resnet_set_debug_vtrace", _ERR)
        return self._vt

    def _batch(self, obs, actions, rewards, discounts, behaviour_logits) -> _lib.ImpalaBatch:
        """The library's batch struct of a collated device batch, shapes and types checked; the
        tensors it points at stay referenced by the engine until the next batch."""
        B, T, A = self.B, self.T, self.A
        want = ((obs, torch.uint8, (B, T) + OBS_SHAPE), (actions, torch.int64, (B, T)),
                (rewards, torch.float32, (B, T)), (discounts, torch.float32, (B, T)),
                (behaviour_logits, torch.float32, (B, T, A)))
        keep = []
        for t, dt, shape in want:
            if t.dtype != dt or t.device != self.device or t.numel() != int(np.prod(shape)):
                raise ValueError(f"batch field: expected {dt} {shape} on {self.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
            keep.append(t.contiguous())
        self._obs = keep[0].view((B * T,) + OBS_SHAPE)  # (what ``backward`` reads after a ``forward_train``)
        self._kept = keep
        return _lib.ImpalaBatch(*[_lib.ptr(t) for t in keep])

    def _step_call(self, name: str, *batch) -> None:
        self._fresh()
        args = (C.byref(self._batch(*batch)),) if batch else ()
        check(getattr(lib(), name)(self._h, *args, _lib.stream_ptr(None)), name, _ERR)

    def loss_head(self, *batch) -> None:
        """``resnet_loss_head`` on the heads of the last ``forward_train`` (of the batch's B T frames): the
        cotangents ("dlogits", "dvalues") and the metric sums ("tpart") stay in the handle."""
        self._step_call("resnet_loss_head", *batch)

    def compute_grads(self, *batch) -> None:
        """forward_train, loss head and backward into ``model.flat_grad`` (``resnet_compute_grads``)."""
        self._step_call("resnet_compute_grads", *batch)

    def _updated(self) -> None:
        """The library updated ``model.flat`` and re-packed this engine's weights: the model's other
        engines re-pack before their next use."""
        self.model.params_changed()
        self._version = self.model._version

    def apply_update(self) -> None:
        """Clip, Adam and the re-pack (``resnet_apply_update``); ``metrics`` is written."""
        self._step_call("resnet_apply_update")
        self._updated()

    def train_step(self, *batch) -> None:
        """One learner step on (obs, actions, rewards, discounts, behaviour_logits), collated on the
        device: ``resnet_train_step``."""
        self._step_call("resnet_train_step", *batch)
        self._updated()

    def debug_tensor(self, name: str, frames: Optional[int] = None):
        """The tensor ``name`` of the last forward / act or, the g* and the names after them, of the
        last ``backward`` (``resnet_debug_read``; a host sync; a handle created with ``debug=True``
        or ``train=True``) as a float32 numpy array [frames, ...]; "amax" as uint32 words of four
        bytes each (``.view(np.uint8)``)."""
        # after a ``loss_head``: its cotangents (``frames`` = B T) and a row of metric sums per trajectory (B)
        step = dict(dlogits=(_lib.RESNET_DBG_DLOGITS, "f32", (self.A,)), dvalues=(_lib.RESNET_DBG_DVALUES, "f32", ()),
                    tpart=(_lib.RESNET_DBG_TPART, "f32", (8,)))
        known = {**self.DEBUG_TENSORS, **self.TRAIN_TENSORS, **step}
        if name not in known:
            raise ValueError(f"unknown debug tensor {name!r}: one of {sorted(known)}")
        which, kind, shape = known[name]
        n = self.N if frames is None else int(frames)
        if not 1 <= n <= self.N:
            raise ValueError(f"frames must be in [1, {self.N}]")
        return _lib.read_debug(
            lambda dst, nbytes, sp: check(lib().resnet_debug_read(self._h, which, dst, nbytes, sp),
                                          "resnet_debug_read", _ERR),
            kind, shape, n, self.bf16, self.device)


class _ResnetGrad(torch.autograd.Function):
    """``ImpalaResNetModel.forward_train`` on the autograd graph, in chunks of the training
    engine's batch.  An engine holds the activations of one chunk at a time, so a chunk's forward
    runs again at the head of its backward; the chunks' gradients are summed in a staging buffer
    (``resnet_backward``'s ``accumulate``) and added to ``model.flat_grad`` once."""

    @staticmethod
    def forward(ctx, anchor, model, obs):
        ctx.model, ctx.obs, ctx.version = model, obs, model._version
        eng = model.train_engine()
        outs = [eng.forward_train(c) for c in model._chunks(obs, eng.N)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    @staticmethod
    def backward(ctx, dlogits, dvalues):
        model, eng = ctx.model, ctx.model.train_engine()
        if ctx.version != model._version:
            raise RuntimeError("the parameters changed between forward_train and backward")
        if model._grad_stage is None:
            model._grad_stage = torch.empty_like(model.flat_grad)
        for i in range(0, ctx.obs.shape[0], eng.N):
            eng.forward_train(ctx.obs[i:i + eng.N])
            eng.backward(dlogits[i:i + eng.N], dvalues[i:i + eng.N], out=model._grad_stage, accumulate=i > 0)
        model._bind_grads()
        model.flat_grad.add_(model._grad_stage)
        return None, None, None


class ImpalaResNetModel(FlatModule):
    """``AtariPPOModel``'s surface over the IMPALA ResNet body on an MI355X:
    ``forward(obs_u8 [N,3,64,64]) -> (logits [N,A], v [N,1])`` through ``resnet_forward`` and
    ``act(obs, deterministic)`` as the reference's remote batched act
    (models/distributed_models.py:21-32) through ``resnet_act``."""

    def __init__(self, obs_shape: Tuple[int, ...] = OBS_SHAPE, n_act: int = 15, device="cuda",
                 dtype: Optional[str] = None, seed: Optional[int] = None, train_batch: int = 160,
                 train_dtype: str = "fp32"):
        super().__init__()
        if tuple(obs_shape) != OBS_SHAPE:
            # models/common.py:81-83 hard-codes output_dim 2048 => 64x64x3 only
            raise ValueError(f"ImpalaCNNLarge requires observations of shape {OBS_SHAPE}")
        if not 1 <= n_act <= 15:
            raise ValueError("n_act must be in [1, 15]")
        self.action_dim = int(n_act)
        self.compute_dtype = dtype or "fp32"
        if train_dtype not in ("fp32", "bf16"):
            raise ValueError("train_dtype: 'fp32' or 'bf16'")
        self.train_dtype = train_dtype  # of forward_train / loss.backward(), whatever forward and act run in
        self._specs = param_specs(self.action_dim)
        self._views, = self._attach_segments(torch.device(device))
        self._infer_engine = None
        self._train_engine, self._train_batch = None, int(train_batch)  # 160: IMPALA's 8 x 20 frames
        self._anchor = self._grad_stage = None
        self._act_seed = int.from_bytes(os.urandom(8), "little") >> 2
        self._act_calls = 0
        self.reset_parameters(seed)

    def _segment_table(self):
        return [(None, self._specs, "flat", "flat_grad")]

    def reset_parameters(self, seed: Optional[int] = None) -> None:
        """Reference init (``resnet_init_flat``); ``seed`` seeds the global torch RNG first."""
        if seed is not None:
            torch.manual_seed(int(seed))
        with torch.no_grad():
            self.flat.copy_(resnet_init_flat(self.action_dim).to(self.flat.device))
        self.params_changed()

    def _engine(self) -> ResnetEngine:
        if self._infer_engine is None:
            # the reference serves act() in batches of <= 128 (distributed_models.py:21)
            self._infer_engine = ResnetEngine(self, batch_size=128)
        return self._infer_engine

    def _chunks(self, x: torch.Tensor, N: Optional[int] = None):
        N = N or self._engine().N
        return [x[i:i + N] for i in range(0, x.shape[0], N)]

    def train_engine(self, batch_size: Optional[int] = None, dtype: Optional[str] = None) -> ResnetEngine:
        """The training engine, of ``train_dtype``; with ``batch_size`` or ``dtype``, one of that
        many frames a chunk or of that type from here on."""
        if dtype is not None and dtype != self.train_dtype:
            if dtype not in ("fp32", "bf16"):
                raise ValueError("dtype: 'fp32' or 'bf16'")
            self.train_dtype, self._train_engine = dtype, None
        if batch_size is not None and int(batch_size) != self._train_batch:
            self._train_batch, self._train_engine = int(batch_size), None
        if self._train_engine is None:
            self._train_engine = ResnetEngine(self, self._train_batch, self.train_dtype, train=True)
        return self._train_engine

    def _bind_grads(self) -> None:
        """Every parameter's ``.grad`` is its view of ``flat_grad``: zeroed where an optimizer's
        ``zero_grad`` had set it to None, taking over a gradient held elsewhere."""
        with torch.no_grad():
            for p, g in self._grad_pairs():
                if p.grad is None:
                    g.zero_()
                elif p.grad.data_ptr() != g.data_ptr():
                    g.copy_(p.grad)
                else:
                    continue
                p.grad = g

    def _grad_pairs(self):
        named = dict(self.named_parameters())
        for k, (off, n, shape) in self._views.items():
            yield named[k], self.flat_grad[off:off + n].view(shape)

    def forward_train(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (logits [N, A], values [N, 1]) attached to the autograd graph: ``loss.backward()``
        adds the gradient into ``flat_grad`` -- every parameter's ``.grad`` is a view of it -- as
        torch accumulates.  N above the training engine's batch runs in chunks, each chunk's
        backward accumulating."""
        if obs.device.type != "cuda" or self.flat.device.type != "cuda":
            raise RuntimeError("ImpalaResNetModel.forward_train runs on the HIP path only (cuda device)")
        if self._anchor is None:
            self._anchor = torch.zeros((), device=self.flat.device, requires_grad=True)
        return _ResnetGrad.apply(self._anchor, self, obs.contiguous())

    def forward(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if obs.device.type != "cuda" or self.flat.device.type != "cuda":
            raise RuntimeError("ImpalaResNetModel.forward runs on the HIP path only (cuda device)")
        outs = [self._engine().forward(c) for c in self._chunks(obs)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    @torch.no_grad()
    def act(self, obs: torch.Tensor, deterministic_policy):
        """-> (action [N,1], logits [N,A], v [N,1]) on the CPU."""
        if self.flat.device.type != "cuda":
            raise RuntimeError("ImpalaResNetModel.act runs on the HIP path only (cuda device)")
        x = obs.to(self.flat.device)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.shape[0] > self._engine().N:
            raise ValueError(f"act serves at most {self._engine().N} frames a call")
        self._act_calls += 1
        res = self._engine().act(x, deterministic_policy, seed=self._act_seed, counter=self._act_calls)
        out = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in res]
        for h, t in zip(out, res):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.flat.device).synchronize()
        return tuple(out)

    def clone_to(self, device) -> "ImpalaResNetModel":
        return self._frozen_clone(ImpalaResNetModel(OBS_SHAPE, self.action_dim, device=device,
                                                    dtype=self.compute_dtype, train_dtype=self.train_dtype))


class ImpalaResNetLearner(Learner):
    """``ImpalaLearner``'s surface (agents/impala/learning.py:86-177) over the IMPALA ResNet: one
    ``resnet_train_step`` per ``train_step`` -- forward, V-trace loss, backward, clip, Adam and the
    re-pack.  The batch is the reference's list of trajectories (collated on the
    device with torch) or a collated device batch; one replica, no staging ring, no prefetch."""

    def __init__(self, model: ImpalaResNetModel, replay_buffer, optimizer=None, batch_size: int = 8,
                 max_grad_norm: float = 0.5, entropy_coeff: float = 0.01,
                 learning_starts: Optional[int] = None, model_push_period: int = 4,
                 rollout_length: int = 20, dtype: Optional[str] = None, vtrace_grad_mode=None):
        from impala_amd.learner import ImpalaAdam
        self._model, self._replay_buffer = model, replay_buffer
        self._optimizer = opt = ImpalaAdam.of(optimizer)
        self._batch_size, self._rollout_length = int(batch_size), int(rollout_length)
        self._learning_starts, self._model_push_period = learning_starts, model_push_period
        self._step_count = self._step_counter = 0
        self._adam_step = 0  # torch's state['step'], as the handle counts it on the device
        self.can_train = True
        self._engine = model.train_engine(self._batch_size * self._rollout_length, dtype)
        self._engine.step_init(self._batch_size, self._rollout_length, lr=opt.lr, eps=opt.eps,
                               betas=opt.betas, max_grad_norm=max_grad_norm, entropy_coeff=entropy_coeff,
                               vtrace_grad_mode=vtrace_grad_mode)

    @property
    def engine(self) -> ResnetEngine:
        return self._engine

    @property
    def samples_per_step(self) -> int:
        return self._batch_size * self._rollout_length

    def prepare(self):  # learning.py:116-117
        self._replay_buffer.warm_up(self._learning_starts)

    def train_step(self):  # learning.py:119-138
        from impala_amd.learner import _collate
        t0 = time.perf_counter()
        _, batch, _ = self._replay_buffer.sample(self._batch_size)
        tensors = _collate(batch, self._engine.device)
        t1 = time.perf_counter()
        metrics = self._train_step(tensors)
        t2 = time.perf_counter()
        update_time = 0
        self._step_count += 1
        self._step_counter = self._step_count
        if self._step_count % self._model_push_period == 0:
            start = time.perf_counter()
            self._model.push()
            update_time = time.perf_counter() - start
        n_samples = self.samples_per_step
        metrics["debug/replay_sample_per_second"] = n_samples / (max(t1 - t0, 1e-9) * 1000)
        metrics["debug/gradient_per_second"] = n_samples / ((t2 - t1) * 1000)
        metrics["debug/total_time"] = (time.perf_counter() - t0) * 1000
        metrics["debug/forward_dt"] = (t2 - t1) * 1000 / self._batch_size
        metrics["debug/update_time"] = update_time
        return metrics

    def _train_step(self, batch):  # learning.py:140-177
        """-> the reference's metric keys as device scalars, views of this step's own vector."""
        m = torch.empty(_lib.NUM_METRICS, dtype=torch.float32, device=self._engine.device)
        self._engine.bind_metrics(m)
        self._engine.train_step(*batch)
        self._adam_step += 1
        return dict(zip(_lib.METRIC_NAMES, m.unbind(0)))

    # ---------------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        e = self._engine
        return {"model": {k: v.detach().clone() for k, v in self._model.state_dict().items()},
                "optimizer": {"step": self._adam_step, "exp_avg": e.exp_avg.clone(),
                              "exp_avg_sq": e.exp_avg_sq.clone()}}

    def load_state_dict(self, sd: dict) -> None:
        e, opt = self._engine, sd["optimizer"]
        self._model.load_state_dict(sd["model"])
        e._fresh()  # resnet_refresh_weights: the kernel-layout weights of the loaded parameters
        e.exp_avg.copy_(opt["exp_avg"])
        e.exp_avg_sq.copy_(opt["exp_avg_sq"])
        self._adam_step = int(opt["step"])
        e.set_step(self._adam_step)
