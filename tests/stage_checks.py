"""Cases and bounds shared by tests/test_ref_stages_host.py (CPU) and tests/test_gpu_stages.py:
one step's workspace tensors, gradient blocks and metrics held, stage by stage, to the float64
stage references (oracle/ref_stages.py) evaluated on that step's OWN input tensors.

Bounds (r = the float64 reference of a stage's output on the step's own inputs):
  fp32 tensors  |d| <= 1e-5 (|r| + rms r): the normwise bound of test_gpu_parity_full.py and
                test_gpu_frame_edges.py.  The bf16 mode's fp32 outputs hold it too: its inputs
                are exact in bf16, so their products are exact in fp32 and the stage is an
                fp32-accumulating computation like the fp32 mode's.
  bf16 tensors  every element |got - r| <= ulp(r) + 1e-5 (|r| + rms r), ulp(r) =
                2^(floor(log2 |r|) - 7); and got == RNE_bf16(r) except for a share of at most
                CAP = 5e-3 of the tensor's elements (those whose fp32 accumulation error crosses
                a rounding boundary).  The cap is a condition, not a measurement: the CPU
                stand-in (the same stages in torch float32) must stay below a quarter of it for
                every tensor at every shape (test_ref_stages_host.py).
  blocks        each of the 14 canonical gradient blocks rel-L2 <= 1e-4 (BLOCK_RL2 of
                test_gpu_wgrad_edges.py: an fp32 sum over M <= 5760 rows of exact products).
                w1 rests on the reference's own rounding of dY1, which never leaves LDS: its
                bound is 4 x the distance between the reference fed a float32-accumulated q(dY1)
                and fed a float64-accumulated one (w1_bound), never below 1e-4.  Measured on the
                CPU: 0 (1x2), 2.4e-9 (2x3), 4.8e-6 (1x11), 3.7e-6 (3x7), 1.8e-5 (8x20) -> the
                bound is 1e-4 at every shape.  b1 sums the unrounded dY1 and the head blocks
                reach 1.6e-7 on the stand-in (its own rounding of dH against the reference's),
                so they keep 1e-4.
  metrics       1e-5 relative from the exported heads; train/pg normwise, |d| <= 1e-5 (|pg| +
                mean |log pi(a) adv|).
"""
import numpy as np
import torch

from oracle import ref_cpu
from oracle import ref_stages as rs

A = 15
CAP = 5e-3
STAND_IN_CAP = CAP / 4
F32_NORMWISE = 1e-5
BLOCK_RL2 = 1e-4
MET_RTOL = 1e-5
MET_NAMES = ("loss", "entropy", "td", "pg", "kl", "ratio")
STEP_SHAPES = [(1, 2), (2, 3), (1, 11), (3, 7), (8, 20)]
# the batch seed of a shape (test_gpu_frame_edges.py's 1234 unless a tensor's stand-in share
# exceeded STAND_IN_CAP there: none did)
SEEDS = {}
PPO_N, PPO_A = 37, 6

_INPUTS = {}


def inputs(shape):
    """(flat0, batch) of a case: ("ppo",), ("fwd",) or (B, T)."""
    if shape not in _INPUTS:
        if shape == ("ppo",):
            v = (ref_cpu.flat_params(ref_cpu.make_model(0, PPO_A)),
                 ref_cpu.synthetic_ppo_batch(PPO_N, PPO_A))
        elif shape == ("fwd",):  # one frame (a T = 1 rollout): the forward stages alone
            v = (ref_cpu.flat_params(ref_cpu.make_model(0, A)),
                 ref_cpu.synthetic_batch(1, 1, A, seed=1234))
        else:
            B, T = shape
            v = (ref_cpu.flat_params(ref_cpu.make_model(0, A)),
                 ref_cpu.synthetic_batch(B, T, A, seed=SEEDS.get(shape, 1234)))
        _INPUTS[shape] = v
    return _INPUTS[shape]


def case_kw(shape):
    if shape == ("ppo",):
        return dict(A=PPO_A, algo="ppo")
    if shape == ("fwd",):
        return dict(A=A, forward_only=True)
    return dict(A=A)


_REF = {}


def reference(shape, given, quant, key=None):
    """The float64 stage references on a step's own tensors; cached under `key` when given (a
    deterministic step of one plan and dtype gives the same tensors every time)."""
    if key is not None and (shape, key) in _REF:
        return _REF[(shape, key)]
    flat0, batch = inputs(shape)
    out = rs.run(flat0, batch, given=given, quant=quant, **case_kw(shape))
    if key is not None:
        _REF[(shape, key)] = out
    return out


_STAND_IN = {}


def stand_in(shape, quant=True):
    """The stages chained in torch float32, rounding where the kernels round: the CPU stand-in
    of a step -> (the run, the tensors it would export)."""
    if (shape, quant) not in _STAND_IN:
        flat0, batch = inputs(shape)
        s = rs.run(flat0, batch, quant=quant, dtype=torch.float32, **case_kw(shape))
        _STAND_IN[(shape, quant)] = (s, rs.stand_in_tensors(s, quant))
    return _STAND_IN[(shape, quant)]


_W1 = {}


def w1_bound(shape):
    """4 x the rel-L2 distance between the reference's w1 fed a float32-accumulated q(dY1) and
    fed a float64-accumulated one, on the stand-in's tensors; never below BLOCK_RL2."""
    if shape not in _W1:
        s, S = stand_in(shape)
        r = reference(shape, S, True, key="stand-in")
        r32 = reference(shape, dict(S, dY1=s["t"]["dY1"]), True)
        _W1[shape] = rs.rel_l2(r32["grads"]["w1"], r["grads"]["w1"])
    return max(BLOCK_RL2, 4 * _W1[shape]), _W1[shape]


def hold_tensors(got, ref, names, quant, label, cap=CAP):
    """Print every tensor's figures; -> the list of violated bounds."""
    bad = []
    for k in names:
        r = ref["t"][k]
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        if not np.isfinite(g).all():
            bad.append(f"{k}: not finite")
        elif quant and k in rs.T_TENSORS:
            worst, share, wu = rs.bf16_figures(g, r)
            print(f"{label} {k:6s} worst |d| / (ulp + 1e-5 (|r| + rms)) {worst:.3f}, "
                  f"share != RNE {share:.2e} (worst {wu:.2f} ulp), rel-L2 {rs.rel_l2(g, r):.2e}")
            if worst > 1.0:
                bad.append(f"{k}: element bound x{worst:.3f}")
            if share > cap:
                bad.append(f"{k}: mismatch share {share:.2e} > {cap:.2e}")
        else:
            w = rs.f32_figures(g, r)
            print(f"{label} {k:6s} normwise {w:.2e}, rel-L2 {rs.rel_l2(g, r):.2e}")
            if w > F32_NORMWISE:
                bad.append(f"{k}: normwise {w:.2e}")
    return bad


def hold_mask(mask1, act1, label):
    want = rs.mask_bits(act1)
    n = int(np.sum(np.asarray(mask1).reshape(want.shape) != want))
    print(f"{label} mask1  words != bits of act1 > 0: {n}")
    return [f"mask1: {n} words differ"] if n else []


def hold_blocks(got, ref, label, bounds=None, names=rs.BLOCKS):
    bad, line = [], []
    for k in names:
        v = rs.rel_l2(got[k], ref["grads"][k])
        b = (bounds or {}).get(k, BLOCK_RL2)
        line.append(f"{k} {v:.1e}")
        if not np.isfinite(v) or v > b:
            bad.append(f"block {k}: rel-L2 {v:.2e} > {b:.1e}")
    print(f"{label} blocks rel-L2: " + ", ".join(line))
    return bad


def hold_metrics(got, ref, label):
    m = ref["met"]
    bad, line = [], []
    for k, g in zip(MET_NAMES, got):
        scale = abs(m["pg"]) + m["pg_abs"] if k == "pg" else abs(m[k])
        v = abs(float(g) - m[k]) / max(scale, 1e-30)
        line.append(f"{k} {v:.1e}")
        if not v <= MET_RTOL:
            bad.append(f"metric {k}: {v:.2e}")
    print(f"{label} metrics rel: " + ", ".join(line))
    return bad
