"""Modules whose parameters are views of flat fp32 buffers -- the one copy of that machinery.

The HIP library reads and updates a whole network through one pointer, while ``state_dict()`` /
``load_state_dict()`` / ``torch.save`` keep the reference's key names: every parameter is a
``torch.nn.Parameter`` VIEW into a flat buffer (and every ``.grad`` a view into a grad buffer),
laid out in the order of a spec table ``[(state_dict name, shape), ...]``.  ``FlatModule`` owns
the buffers, the views and what keeps them views (pickling, deepcopy, cloning); a model declares
its segments and adds its compute methods.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn


class _Node(nn.Module):
    pass


def spec_count(specs) -> int:
    return sum(int(np.prod(s)) for _, s in specs)


def attach_views(root: nn.Module, specs, flat: torch.Tensor, grad: Optional[torch.Tensor],
                 requires_grad: bool = True) -> Dict[str, Tuple[int, int, Tuple[int, ...]]]:
    """Register every ``(name, shape)`` of ``specs`` under ``root`` as a parameter viewing its
    slice of ``flat`` (its ``.grad`` the same slice of ``grad``), creating the modules the dotted
    names pass through.  -> ``{name: (offset, count, shape)}``."""
    views, off = {}, 0
    for name, shape in specs:
        cnt = int(np.prod(shape))
        parts = name.split(".")
        mod = root
        for p in parts[:-1]:
            if not isinstance(getattr(mod, p, None), nn.Module):
                mod.add_module(p, _Node())
            mod = getattr(mod, p)
        param = nn.Parameter(flat[off:off + cnt].view(shape), requires_grad=requires_grad)
        if grad is not None:
            param.grad = grad[off:off + cnt].view(shape)
        mod.register_parameter(parts[-1], param)
        views[name] = (off, cnt, tuple(shape))
        off += cnt
    assert off == flat.numel()
    return views


def rebind_views(root: nn.Module, specs, flat: torch.Tensor, grad: Optional[torch.Tensor]) -> None:
    """Point every registered parameter of ``root`` (``specs`` order) back at its view of
    ``flat`` (and its ``.grad`` at the view of ``grad``).  Unpickling (``torch.load`` of a
    whole model) and ``copy.deepcopy`` rebuild each ``nn.Parameter`` on its own storage and
    drop ``.grad``; the HIP library reads and writes the model through the flat buffers only."""
    off = 0
    for name, shape in specs:
        cnt = int(np.prod(shape))
        param = root.get_parameter(name)
        param.data = flat[off:off + cnt].view(shape)
        param.grad = None if grad is None else grad[off:off + cnt].view(shape)
        off += cnt
    assert off == flat.numel()


def layer_init_truncated(layer: nn.Module, fan_in: int) -> nn.Module:
    """The reference's ``layer_init_truncated`` (models/common.py:151-158) restated:
    trunc_normal weights of std sqrt(1 / fan_in) / 0.8796..., zero bias."""
    std_div = np.asarray(.87962566103423978, dtype=np.float32)
    with torch.no_grad():
        std = np.sqrt(1.0 / max(1, fan_in)) / std_div
        torch.nn.init.trunc_normal_(layer.weight, std=std)
        torch.nn.init.constant_(layer.bias, 0.)
    return layer


def trunk_init_flat(hidden: int, action_dim: int) -> torch.Tensor:
    """Reference init of the NatureCNN trunk and two heads as one flat CPU tensor, bit for bit:
    the layers are constructed in the reference's order (each torch default init consumes the
    global RNG exactly as there) and ``layer_init_truncated`` is applied to the 3 convs and the
    3 Linears; LayerNorm stays (1, 0) (models/models.py:61-70, models/common.py:108-126)."""
    trunc = layer_init_truncated
    layers = [trunc(nn.Conv2d(3, 32, 8, stride=4), 3 * 64),
              trunc(nn.Conv2d(32, 64, 4, stride=2), 32 * 16),
              trunc(nn.Conv2d(64, 64, 3, stride=1), 64 * 9),
              nn.LayerNorm(1024), trunc(nn.Linear(1024, hidden), 1024),
              trunc(nn.Linear(hidden, action_dim), hidden), trunc(nn.Linear(hidden, 1), hidden)]
    return torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])


# attributes holding native handles (ctypes pointers): never pickled, recreated lazily
ENGINE_ATTRS = ("_train_engine", "_infer_engine", "_engine")


def picklable_state(module: nn.Module) -> dict:
    state = dict(module.__dict__)
    for k in ENGINE_ATTRS:
        if k in state and not callable(state[k]):
            state[k] = None
    return state


class FlatModule(nn.Module):
    """An ``nn.Module`` over an ordered table of segments ``(root, specs, flat, grad)``: ``root``
    names the child module the specs hang under (None: this module), ``flat`` / ``grad`` name the
    attributes holding the segment's buffers (``grad`` None for a target network, whose
    parameters do not require grad).  A subclass gives the table in ``_segment_table``, from
    attributes every pickle of it carries, so nothing about the layout is pickled state.
    ``_version`` counts writes to the buffers from outside the HIP update; engines compare it to
    re-derive their kernel-layout weights lazily."""

    def __init__(self):
        super().__init__()
        self._version = 0
        self.downstream = None  # the inference copy push() publishes to

    def _segment_table(self):
        raise NotImplementedError

    def _segments(self):
        """-> (root module, specs, flat buffer, grad buffer or None) per segment."""
        return [(self if root is None else getattr(self, root), specs, getattr(self, flat),
                 None if grad is None else getattr(self, grad))
                for root, specs, flat, grad in self._segment_table()]

    def _attach_segments(self, device) -> list:
        """Allocate every segment's zeroed buffers as ``self.<flat>`` / ``self.<grad>`` and attach
        the views; -> ``attach_views``' offsets, per segment."""
        for root, specs, flat, grad in self._segment_table():
            for attr in filter(None, (flat, grad)):
                setattr(self, attr, torch.zeros(spec_count(specs), dtype=torch.float32, device=device))
            if root is not None and not hasattr(self, root):
                self.add_module(root, _Node())
        return [attach_views(*seg, requires_grad=seg[3] is not None) for seg in self._segments()]

    # ---------------------------------------------------------------- parameters
    def params_changed(self) -> None:
        """Parameters were written from outside the HIP update: engines must re-derive their
        kernel-layout weights (lazily, before their next use)."""
        self._version = getattr(self, "_version", 0) + 1

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        res = super().load_state_dict(state_dict, strict=strict, assign=False)
        self.params_changed()
        return res

    # ---------------------------------------------------------------- pickling
    def __getstate__(self):
        """``torch.save(builder.learner_model)`` (reference main.py:117) works with engines
        attached: the engines hold native handles and are dropped (an unpickled model creates
        its inference engine lazily; a learner re-attaches its own)."""
        return picklable_state(self)

    def __setstate__(self, state):
        super().__setstate__(state)
        for seg in self._segments():
            rebind_views(*seg)
        self._rebound()
        self.params_changed()

    def _rebound(self) -> None:
        """Hook: rebind what is a view but no segment (after unpickling / deepcopy)."""

    # ---------------------------------------------------------------- publishing
    def push(self) -> None:
        """rlmeta DownstreamModel.push (utils.py:87-88): publish weights to the inference copy."""
        downstream = getattr(self, "downstream", None)  # (absent in older pickles of a critic)
        if downstream is not None:
            downstream.load_flat_from(self)

    def load_flat_from(self, other: "FlatModule") -> None:
        with torch.no_grad():
            for _, _, flat, _ in self._segment_table():
                dst = getattr(self, flat)
                dst.copy_(getattr(other, flat).to(dst.device, non_blocking=True))
        self.params_changed()

    def _frozen_clone(self, m: "FlatModule") -> "FlatModule":
        """What ``clone_to`` ends with: ``m``, a fresh instance of this class, gets this
        module's buffers and no parameter of it requires grad."""
        m.load_flat_from(self)
        for p in m.parameters():
            p.requires_grad_(False)
        return m
