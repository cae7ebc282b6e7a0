"""The IMPALA ResNet actor-critic on the HIP library: the reference's
``AtariActorCritic`` (models/models.py:61-76) with ``ImpalaCNNLarge`` (models/common.py:11-83) as
its body -- the actor path, ``forward`` and ``act``, and the backward pass:
``forward_train`` returns outputs attached to the autograd graph, and ``loss.backward()`` runs
``resnet_backward`` into ``model.flat_grad``, in fp32 or (``train_dtype="bf16"``) in bf16.  Every compute entry is one call of
include/resnet_hip.h; the compute path is the HIP library only.  The one-call learner step (loss
head, clip and Adam fused) is not built, so there is no ``conf/`` entry for this network yet.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from impala_amd import _lib
from impala_amd._lib import check, lib
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

    def debug_tensor(self, name: str, frames: Optional[int] = None):
        """The tensor ``name`` of the last forward / act or, the g* and the names after them, of the
        last ``backward`` (``resnet_debug_read``; a host sync; a handle created with ``debug=True``
        or ``train=True``) as a float32 numpy array [frames, ...]; "amax" as uint32 words of four
        bytes each (``.view(np.uint8)``)."""
        known = {**self.DEBUG_TENSORS, **self.TRAIN_TENSORS}
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
