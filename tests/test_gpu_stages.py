"""Every stage of the step held to float64 on the step's own tensors (teacher forcing).

The end-to-end checks of the bf16 step (metrics 5e-2, gradient cosine > 0.99) admit a gradient
that is 14 % wrong in norm, and a float64 oracle that rounds where the kernels round cannot be
compared end to end either: one rounding that lands the other way moves everything after it.
So each case runs ONE Engine.compute_grads on a fresh handle (no Adam: the weights stay the ones
loaded, and m.flat_grad is the pre-clip gradient -- reduce_grads writes it, the clip is the Adam
kernel's), exports the workspace tensors (Engine.debug_tensor) and, for each stage, evaluates
the float64 reference of that stage alone (oracle/ref_stages.py) on the tensors the kernel read.
The bounds are those of tests/stage_checks.py (its docstring): fp32 tensors normwise 1e-5; bf16
tensors within one ulp of the reference and equal to its correct rounding except for a share of
at most 5e-3; mask1 the bits of the exported act1 > 0; each of the 14 gradient blocks rel-L2
1e-4 (w1: stage_checks.w1_bound, measured on the CPU stand-in: 4 x {0, 2.4e-9, 4.8e-6, 3.7e-6,
1.8e-5} at 1x2, 2x3, 1x11, 3x7, 8x20, i.e. 1e-4 at every shape); the loss metrics 1e-5 relative
from the exported heads (train/pg normwise).  tests/test_ref_stages_host.py shows on the CPU
that the references are the network, that a float32 evaluation stays within a quarter of the
cap, and that the bounds catch a dropped chunk, a doubled frame, a shifted tap, an LN backward
from y and an unrounded dH.

Cases (A = 15, the parameters and batches of test_gpu_frame_edges.py), bf16 and, with the
rounding off, fp32:
  1x2, 2x3, 1x11   under `default` and `run5` (IMPALA_C12F_FPW = IMPALA_C1_FPW = 5: 5-frame runs
                   with a ragged last workgroup; the separate per-frame backward launches)
  3x7              default
  8x20             split plans `a` and `c` of test_gpu_wgrad_edges.py
  fwd              Engine.forward of one frame (a T = 1 rollout): the forward stages
  ppo              algo="ppo", N = 37, A = 6: the head stage alone (dz, the head gradients)
                   against ref_cpu.ppo_loss on the exported heads
"""
import hashlib

import numpy as np
import pytest
import torch

import stage_checks as sc
from oracle import ref_stages as rs

pytestmark = pytest.mark.gpu
PLANS = {
    "default": {},
    "run5": {"IMPALA_C12F_FPW": "5", "IMPALA_C1_FPW": "5"},
    "a": {"IMPALA_WG3_TARGET": "126", "IMPALA_WG2_TARGET": "180", "IMPALA_FC_WG": "48"},
    "c": {"IMPALA_WG3_TARGET": "360", "IMPALA_WG2_TARGET": "360", "IMPALA_FC_WG": "16"},
}
CASES = [pytest.param(s, p, id=f"B{s[0]}_T{s[1]}_{p}")
         for s in [(1, 2), (2, 3), (1, 11)] for p in ("default", "run5")] + \
    [pytest.param((3, 7), "default", id="B3_T7_default"),
     pytest.param((8, 20), "a", id="B8_T20_a"), pytest.param((8, 20), "c", id="B8_T20_c")]
EXPORTS = rs.T_TENSORS + rs.F32_TENSORS


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _engine(shape, dtype, plan, monkeypatch):
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    flat0, batch = sc.inputs(shape)
    kw = sc.case_kw(shape)
    m = AtariPPOModel((3, 64, 64), kw["A"], device=_dev(), dtype=dtype)
    m.load_flat(flat0)
    if shape == ("ppo",):
        e = Engine(m, batch_size=sc.PPO_N, algo="ppo")
    else:
        e = Engine(m, batch_size=batch[1].shape[0], rollout_length=max(batch[1].shape[1], 2))
    m._train_engine = e
    return m, e, batch


def _reference(shape, given, quant):
    """The float64 references on these tensors, once per distinct set of tensors (plans that do
    not change a tensor's bits share them)."""
    h = hashlib.sha1()
    for k in sorted(given):
        h.update(np.ascontiguousarray(given[k]).tobytes())
    return sc.reference(shape, given, quant, key=(quant, h.hexdigest()))


def _step(shape, dtype, plan, monkeypatch):
    m, e, batch = _engine(shape, dtype, plan, monkeypatch)
    dev = _dev()
    e.compute_grads(*[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in batch])
    torch.cuda.synchronize()
    got = {k: e.debug_tensor(k) for k in EXPORTS}
    mask1 = e.debug_tensor("mask1")
    grad = m.flat_grad.cpu().numpy().astype(np.float64)
    met = e.metrics.cpu().numpy()[:6].astype(np.float64)
    e.close()
    return got, mask1, grad, met


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape,plan", CASES)
def test_step_stages(shape, plan, dtype, monkeypatch):
    quant = dtype == "bf16"
    got, mask1, grad, met = _step(shape, dtype, plan, monkeypatch)
    ref = _reference(shape, got, quant)
    label = f"{dtype} {shape[0]}x{shape[1]} {plan}"
    bad = sc.hold_tensors(got, ref, EXPORTS, quant, label)
    bad += sc.hold_mask(mask1, got["act1"], label)
    assert np.isfinite(grad).all() and np.isfinite(met).all()
    bound, dist = sc.w1_bound(shape)
    print(f"{label} w1 bound {bound:.1e} (reference fed float32- vs float64-accumulated q(dY1): {dist:.2e})")
    bad += sc.hold_blocks(rs.split_flat(grad, sc.A), ref, label, {"w1": bound})
    bad += sc.hold_metrics(met, ref, label)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_forward_stages_one_frame(dtype, monkeypatch):
    shape, quant = ("fwd",), dtype == "bf16"
    m, e, batch = _engine(shape, dtype, "default", monkeypatch)
    e.forward(torch.from_numpy(batch[0].reshape(-1, 3, 64, 64)).to(_dev()))
    torch.cuda.synchronize()
    got = {k: e.debug_tensor(k, frames=1) for k in rs.FORWARD_TENSORS}
    mask1 = e.debug_tensor("mask1", frames=1)
    e.close()
    ref = _reference(shape, got, quant)
    label = f"{dtype} forward N=1"
    bad = sc.hold_tensors(got, ref, rs.FORWARD_TENSORS, quant, label)
    bad += sc.hold_mask(mask1, got["act1"], label)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ppo_head_stage(dtype, monkeypatch):
    shape, quant = ("ppo",), dtype == "bf16"
    got, _, grad, met = _step(shape, dtype, "default", monkeypatch)
    ref = _reference(shape, got, quant)
    label = f"{dtype} ppo N={sc.PPO_N} A={sc.PPO_A}"
    print(f"{label} metrics (loss, entropy, td, pg, kl, ratio): kernel {met.tolist()}, "
          f"float64 on the exported heads {[ref['met'][k] for k in sc.MET_NAMES]}")
    bad = sc.hold_tensors(got, ref, ("dz",), quant, label)
    bad += sc.hold_blocks(rs.split_flat(grad, sc.PPO_A), ref, label, names=("wa", "ba", "wc", "bc"))
    assert not bad, bad
