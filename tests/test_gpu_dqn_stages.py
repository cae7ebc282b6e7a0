"""Every stage of the Ape-X DQN step held to float64 on the step's own tensors (teacher forcing),
as tests/test_gpu_stages.py holds the IMPALA / PPO step: the 512-wide instantiations of the FC
forward, the FC backward and the weight-gradient GEMM, and all of dqn_head_step_body, in bf16
and in fp32.

Each case makes a fresh handle and runs ONE DqnEngine.compute_grads (dqn_compute_grads: the
step without clip and Adam, so m.flat_grad is the pre-clip gradient -- dqn_train_step's Adam
kernel writes g * min(1, max_grad_norm / norm) back into it, kernels.h adam_kernel), exports the
workspace tensors (DqnEngine.debug_tensor) and evaluates each stage's float64 reference
(oracle/ref_stages.py, algo="dqn") on the tensors that stage read.  Then the full
DqnEngine.train_step runs on the same handle -- the weights are still the loaded ones -- and
must reproduce the priorities, metrics 0..3 and dz bit for bit and leave coef x that gradient,
so what is held for the one is held for the other; its grad_norm is held to the float64 norm
of the pre-clip gradient at 1e-4 relative (test_gpu_dqn.py's).

Bounds: those of tests/stage_checks.py, unchanged -- fp32 tensors normwise 1e-5; bf16 tensors
within one ulp and equal to RNE except on a share of at most CAP = 5e-3; the 14 blocks rel-L2
1e-4; metrics 1e-5 relative.  w1 by stage_checks.w1_bound; measured on the CPU stand-in the
distance is 0 (N = 1, A = 15), 0 (1, 1), 1.3e-5 (32, 6), 1.1e-5 (33, 2), 6.9e-6 (33, 15),
9.9e-6 (65, 6), 6.8e-6 (100, 15): the bound is 1e-4 at every case.  In addition:
  priorities  |prio - |target - q_ref|| <= 1e-5 (|q_ref| + rms q_ref + |target|), q_ref from
              the exported h: the heads' normwise bound carried through one subtraction.
  metric q    normwise against mean |q_a|, as train/pg against pg_abs.
  q           dqn_forward's output against the dueling formula on the exported heads, each
              element within (A + 3) 2^-24 (|v| + |adv_k| + mean |adv|): dqn_q_kernel does A + 3
              fp32 roundings.

The hazard of the head stage: dz, d wh and d bh hang on the bf16 rounding of dH, which the kernel
takes from fp32 values; an element within fp32 error of a rounding boundary can round the other
way than the float64 reference, which moves a whole dz row and, at N = 1, the head blocks by
about 5e-4.  It is handled, not tolerated: err is pinned from the export (the kernel stores
fabsf(err); the sign is the reference's), which leaves w, two divisions and the products in
fp32; an element is undecided when its float64 value is within the margin those operations
allow of a boundary (stage_checks.dqn_margins, with the derivation and the powf accuracy
assumed: 1 ULP, the HIP programming guide's table of device math functions); for undecided
elements both roundings are evaluated and ONE assignment must hold dz, wa, ba, wc and bc
together (stage_checks.dqn_resolve_head).  More than 4 undecided decisions fail the case.  The
A - 1 copies of da = -dq / A in a row are one fp32 number stored A - 1 times: one decision.  The
seeds are those for which the CPU stand-in has none (test_ref_stages_host.py asserts it).

Cases:
  step     (N, A, probabilities) = (1, 15, yes), (1, 1, no), (32, 6, yes), (33, 2, no),
           (33, 15, yes), (65, 6, no), (100, 15, yes): one transition, A = 1, a full block of
           32, a block plus one row, padded head rows, three blocks with the last ragged
  head     N = 1030, A = 15, the batch minimum of the probabilities at index 1029 (only the
           second pass of dqn_batch_pmin's loop sees it): dz, the four head blocks, the
           priorities and the metrics from the exported h and zg
  forward  an inference_only handle of 8 frames, n = 1 and n = 5, A = 6, the online net and a
           nudged target net: FORWARD_TENSORS with each net's weights, and q
"""
import numpy as np
import pytest
import torch

import stage_checks as sc
from oracle import ref_stages as rs

pytestmark = pytest.mark.gpu
_ids = lambda s: "_".join(str(v) for v in s[1:])  # noqa: E731


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _engine(A, N, dtype, flat, target=None, **kw):
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    with torch.random.fork_rng(devices=[]):
        m = AtariDQNModel((3, 64, 64), A, device=_dev(), dtype=dtype, seed=0)
    m.load_flat(flat, target)
    e = DqnEngine(m, batch_size=N, **kw)
    m._train_engine = e
    return m, e


def _step(shape, dtype, names):
    """One compute_grads, its exports, then the full step on the same weights."""
    _, N, A, _ = shape
    flat0, batch = sc.inputs(shape)
    dev = _dev()
    m, e = _engine(A, N, dtype, flat0)
    args = [_t(x, dev) for x in batch]
    prio = e.compute_grads(*args).cpu().numpy()
    got = {k: e.debug_tensor(k) for k in names}
    got["prio"] = prio.astype(np.float64)
    mask1 = e.debug_tensor("mask1")
    grad = m.flat_grad.cpu().numpy().astype(np.float64)
    met = e.metrics.cpu().numpy().astype(np.float64)
    assert np.isfinite(grad).all() and np.isfinite(met[:4]).all() and np.isfinite(prio).all()
    assert np.array_equal(m.flat.cpu().numpy(), flat0), "compute_grads moved the parameters"
    # the full step: the same numbers, then clip and Adam
    prio2 = e.train_step(*args).cpu().numpy()
    met2 = e.metrics.cpu().numpy().astype(np.float64)
    label = f"{dtype} dqn N={N} A={A}"
    bad = []
    if not (np.array_equal(prio2, prio) and np.array_equal(met2[:4], met[:4])
            and np.array_equal(e.debug_tensor("dz"), got["dz"])):
        bad.append("train_step and compute_grads differ in priorities, metrics 0..3 or dz")
    norm = float(np.sqrt(np.sum(grad * grad)))
    rel = abs(met2[6] - norm) / norm
    print(f"{label} grad_norm {met2[6]:.8g}, float64 norm of the step's flat_grad {norm:.8g}: rel {rel:.1e}")
    if not rel <= sc.GRAD_NORM_RTOL:
        bad.append(f"metric grad_norm: {rel:.2e}")
    coef = min(1.0, 40.0 / (float(met2[6]) + 1e-6))
    clipped = rs.rel_l2(m.flat_grad.cpu().numpy(), coef * grad)
    print(f"{label} clip factor {coef:.6g}: flat_grad after train_step vs coef x pre-clip rel-L2 {clipped:.1e}")
    if not clipped <= 1e-6:
        bad.append(f"flat_grad after train_step is not coef x the pre-clip gradient: {clipped:.2e}")
    e.close()
    return got, mask1, grad, met[:4], bad, label, batch


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", sc.DQN_CASES, ids=_ids)
def test_dqn_step_stages(shape, dtype):
    quant = dtype == "bf16"
    got, mask1, grad, met, bad, label, batch = _step(shape, dtype, sc.DQN_STEP_TENSORS)
    A = shape[2]
    blocks = rs.split_flat(grad, A, "dqn")
    ref = sc.reference(shape, got, quant)
    ref, more = sc.dqn_resolve_head(shape, got, blocks, ref, quant, label)
    bad += more
    bad += sc.hold_tensors(got, ref, sc.DQN_STEP_TENSORS, quant, label)
    bad += sc.hold_mask(mask1, got["act1"], label)
    bound, dist = sc.w1_bound(shape)
    print(f"{label} w1 bound {bound:.1e} (reference fed float32- vs float64-accumulated q(dY1): {dist:.2e})")
    bad += sc.hold_blocks(blocks, ref, label, {"w1": bound})
    bad += sc.hold_dqn_prio(got["prio"], ref, batch, label)
    bad += sc.hold_dqn_metrics(met, ref, label)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_dqn_head_stage(dtype):
    shape, quant = sc.DQN_HEAD, dtype == "bf16"
    got, _, grad, met, bad, label, batch = _step(shape, dtype, ("h", "zg", "dz"))
    assert int(np.argmin(batch[3])) == shape[1] - 1 > 1024
    blocks = rs.split_flat(grad, shape[2], "dqn")
    ref = sc.reference(shape, got, quant)
    print(f"{label} metrics (q, target, priorities, loss): kernel {met.tolist()}, "
          f"float64 on the exported h {[ref['met'][k] for k in sc.DQN_MET_NAMES]}")
    ref, more = sc.dqn_resolve_head(shape, got, blocks, ref, quant, label)
    bad += more
    bad += sc.hold_tensors(got, ref, ("dz",), quant, label)
    bad += sc.hold_blocks(blocks, ref, label, names=sc.DQN_HEAD_BLOCKS)
    bad += sc.hold_dqn_prio(got["prio"], ref, batch, label)
    bad += sc.hold_dqn_metrics(met, ref, label)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_dqn_forward_stages(dtype):
    quant = dtype == "bf16"
    A, F = sc.DQN_FWD_A, sc.DQN_FWD_FRAMES
    online, _ = sc.inputs(("dqn_fwd", 1, False))
    _, e = _engine(A, F, dtype, online, sc.dqn_target_flat(A), inference_only=True)
    dev = _dev()
    bad = []
    for shape in sc.DQN_FWD_CASES:
        _, n, target = shape
        _, (obs,) = sc.inputs(shape)
        q = e.forward(_t(obs, dev), target=target).cpu().numpy()
        got = {k: e.debug_tensor(k, frames=n, target=target) for k in rs.FORWARD_TENSORS}
        mask1 = e.debug_tensor("mask1", frames=n)
        ref = sc.reference(shape, got, quant)
        label = f"{dtype} dqn forward n={n} {'target' if target else 'online'}"
        bad += [f"{label}: {b}" for b in
                sc.hold_tensors(got, ref, rs.FORWARD_TENSORS, quant, label)
                + sc.hold_mask(mask1, got["act1"], label)
                + sc.hold_dqn_q(q, got["heads"], A, label)]
    e.close()
    assert not bad, bad
