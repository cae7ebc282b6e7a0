"""The IMPALA ResNet learner step's host side without a GPU (include/resnet_hip.h): the step's defaults,
the refusals that need no device and the flat buffer's scalar tail (three floats at A = 2 and A = 6)."""
import ctypes as C

import pytest

from impala_amd import _lib
from impala_amd.resnet import param_count


def _cfg(**kw):
    cfg = _lib.ResnetStepConfig()
    assert _lib.lib().resnet_step_config_default(C.byref(cfg)) == 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_step_config_default():
    cfg, f = _cfg(), C.c_float
    got = [getattr(cfg, k) for k, _ in _lib.ResnetStepConfig._fields_]
    assert got == [8, 20, f(1e-4).value, f(0.9).value, f(0.999).value, f(1e-5).value, 0.5, f(0.01).value, 1, 1, 1, 0]


@pytest.mark.parametrize("kw,why", [(dict(rollout_length=1), "rollout_length"), (dict(rollout_length=65), "rollout_length"),
                                    (dict(batch_size=0), "batch_size"), (dict(vtrace_grad_mode=3), "vtrace_grad_mode"),
                                    ({}, "null handle")])
def test_step_init_refuses_before_any_hip_call(kw, why):
    L = _lib.lib()
    assert L.resnet_step_init(None, C.byref(_cfg(**kw))) == 1001 and why in L.resnet_last_error().decode()


def test_null_handles_and_pointers():
    L, batch = _lib.lib(), C.byref(_lib.ImpalaBatch())
    assert L.resnet_step_config_default(None) == 1001 and L.resnet_step_init(None, None) == 1001
    assert L.resnet_bind_state(None, 0, 0, 0, 0, 0, 0) == 1001 and L.resnet_set_step(None, 0, 0) == 1001
    assert L.resnet_apply_update(None, 0) == 1001 and L.resnet_set_debug_vtrace(None, 0) == 1001
    assert all(getattr(L, f)(None, batch, 0) == 1001 for f in ("resnet_loss_head", "resnet_compute_grads", "resnet_train_step"))


@pytest.mark.parametrize("A", range(1, 16))
def test_flat_tail(A):
    n = _lib.lib().resnet_param_count(A)
    assert n == param_count(A) == 626240 + 257 * (A + 1)
    assert n % 4 == (A + 1) % 4  # a whole number of 16-byte vectors only where A = 3 (mod 4)
