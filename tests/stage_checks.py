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

The Ape-X DQN step (tests/test_gpu_dqn_stages.py) is held to the same bounds; its cases, the
priorities' and q's bounds and the handling of an undecided rounding of dH are in the section
after these; the IQN actor path's forward (tests/test_gpu_iqn_stages.py) follows, and the SAC step
(tests/test_gpu_sac_stages.py, references oracle/sac_stages.py) is the last section.
"""
import math

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
        if shape[0] in ("dqn", "dqn_fwd"):
            v = _dqn_inputs(shape)
        elif shape[0] == "iqn":
            v = _iqn_inputs(shape)
        elif shape == ("ppo",):
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
    if shape[0] == "iqn":
        return dict(A=shape[3], algo="iqn", head_only=shape[:4] == IQN_LARGE[:4])
    if shape[0] == "dqn":
        return dict(A=shape[2], algo="dqn", beta=DQN_BETA, head_only=shape == DQN_HEAD)
    if shape[0] == "dqn_fwd":
        return dict(A=DQN_FWD_A, algo="dqn", forward_only=True)
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
        S = rs.stand_in_tensors(s, quant)
        if "prio" in s:  # (the DQN step's priorities: what the kernel would write, a float32)
            S["prio"] = s["prio"]
        _STAND_IN[(shape, quant)] = (s, S)
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


# ------------------------------------------------------------------------------ Ape-X DQN
# The dueling net's step (tests/test_gpu_dqn_stages.py; the module docstring there has the
# bounds' sources).  A case is ("dqn", N, A, probabilities?) or ("dqn_fwd", frames, target net?).
DQN_CASES = [("dqn", 1, 15, True), ("dqn", 1, 1, False), ("dqn", 32, 6, True),
             ("dqn", 33, 2, False), ("dqn", 33, 15, True), ("dqn", 65, 6, False),
             ("dqn", 100, 15, True)]
DQN_HEAD = ("dqn", 1030, 15, True)  # the head stage alone; min p at index 1029
DQN_FWD_FRAMES, DQN_FWD_A = 8, 6
DQN_FWD_CASES = [("dqn_fwd", n, t) for n in (1, 5) for t in (False, True)]
DQN_BETA = 0.4
DQN_STEP_TENSORS = tuple(k for k in rs.T_TENSORS + rs.F32_TENSORS if k != "heads")
DQN_HEAD_BLOCKS = ("wa", "ba", "wc", "bc")
DQN_MET_NAMES = ("q", "target", "priorities", "loss")
PRIO_NORMWISE = 1e-5
GRAD_NORM_RTOL = 1e-4
MAX_UNDECIDED = 4
# u = 2^-24, the unit roundoff of fp32.  With err pinned, the kernel's dq = -(err w) (1 / N) takes:
# two powf (<= 1 ulp = 2u each: the HIP programming guide's table of device math functions lists
# powf at 1 ULP, and nothing is compiled with fast-math) and their quotient (u): w within 5u;
# err w (u); fl(1 / N) (u) and the product with it (u): dq within 8u |dq| to first order.  da =
# fl(-dq / A) adds u: within 9u |da|; dq + da adds u |dq + da|.  With one u each for the
# second-order terms, the margins of the three numbers of a row:
#   dq: 9u |dq|     da: 10u |da|     dq + da: 9u |dq| + 10u |da| + u |dq + da|
DQN_U = 2.0 ** -24


def dqn_margins(dH, act, A):
    """-> the margin of every element of dH [N,16] (above), zero where dH is zero."""
    dH = np.asarray(dH, np.float64)
    dq = np.abs(dH[:, rs.VCOL])
    da = dq / A
    m = np.zeros_like(dH)
    m[:, :A] = (10 * DQN_U * da)[:, None]
    n = np.arange(dH.shape[0])
    a = np.asarray(act).reshape(-1)
    m[n, a] = DQN_U * (9 * dq + 10 * da + np.abs(dH[n, a]))
    m[:, rs.VCOL] = 9 * DQN_U * dq
    return np.where(dH == 0, 0.0, m)


# the batch seed of a DQN case (100 N + A, test_gpu_dqn.py's, unless the stand-in's share of
# elements != RNE exceeded STAND_IN_CAP for a tensor there, or an element of its dH was undecided:
# none did; the largest share is 2.4e-4, h at N = 33, A = 15)
DQN_SEEDS = {}


def _dqn_flat(A):
    """The dueling net's seed-0 initialisation with every bias and the LayerNorm affine moved off
    0 / 1 (a stage that dropped one could not pass) -> (online, nudged target), float32."""
    import torch
    from impala_amd.dqn import AtariDQNModel
    with torch.random.fork_rng(devices=[]):
        flat = AtariDQNModel((3, 64, 64), A, device="cpu", seed=0).flat.numpy().copy()
    rng = np.random.default_rng(3)
    off = 0
    for n, s in rs.block_shapes(A, "dqn"):
        k = int(np.prod(s))
        if len(s) == 1:
            flat[off:off + k] += (0.02 * rng.standard_normal(k)).astype(np.float32)
        off += k
    target = flat + (0.01 * rng.standard_normal(flat.size)).astype(np.float32)
    return flat, target


_DQN_FLAT = {}


def _dqn_inputs(shape):
    import dqn_oracle as orc
    A = DQN_FWD_A if shape[0] == "dqn_fwd" else shape[2]
    if A not in _DQN_FLAT:
        _DQN_FLAT[A] = _dqn_flat(A)
    online, target = _DQN_FLAT[A]
    if shape[0] == "dqn_fwd":
        _, n, tgt = shape
        obs = np.random.default_rng(77).integers(0, 256, size=(DQN_FWD_FRAMES, 3, 64, 64), dtype=np.uint8)
        return (target if tgt else online), (obs[:n],)
    _, N, A, probs = shape
    obs, act, tgt, p = orc.synthetic_batch(N, A, seed=DQN_SEEDS.get(shape, 100 * N + A), probs=probs)
    if shape == DQN_HEAD:  # the batch minimum where only the second pass of the loop sees it
        p = p.copy()
        p[N - 1] = np.float32(0.5) * p.min()
    return online, (obs, act, tgt, p)


def dqn_target_flat(A=DQN_FWD_A):
    if A not in _DQN_FLAT:
        _DQN_FLAT[A] = _dqn_flat(A)
    return _DQN_FLAT[A][1]


def dqn_undecided(dH, act, A):
    """The rounding decisions of dH that fp32 cannot be trusted with: a row holds three distinct
    numbers -- dq (column 15), da = -dq / A (the A - 1 columns k != a: one fp32 value stored A - 1
    times, one decision) and dq + da (column a) -- and one of them is undecided when its float64
    value lies within its margin (dqn_margins) of a bf16 rounding boundary, i.e. when the two
    ends of that interval round differently.  -> [(row, columns, lower rounding, upper rounding)]"""
    import torch
    dH = np.asarray(dH, np.float64)
    act = np.asarray(act).reshape(-1)
    m = dqn_margins(dH, act, A)
    lo = rs.rne_bf16(torch.from_numpy(dH - m)).numpy()
    hi = rs.rne_bf16(torch.from_numpy(dH + m)).numpy()
    out = []
    for n in np.nonzero((lo != hi).any(1))[0]:
        a = int(act[n])
        groups = [[rs.VCOL], [a]] + ([[k for k in range(A) if k != a]] if A > 1 else [])
        for cols in groups:
            c = cols[0]
            if dH[n, c] != 0 and lo[n, c] != hi[n, c]:
                out.append((int(n), cols, float(lo[n, c]), float(hi[n, c])))
    return out


def dqn_head_assignments(dH, act, A):
    """-> (the undecided decisions, the rounded dH of every assignment of them: the reference's
    own rounding first).  More than MAX_UNDECIDED decisions: no assignments."""
    import itertools
    import torch
    und = dqn_undecided(dH, act, A)
    base = rs.rne_bf16(torch.from_numpy(np.asarray(dH, np.float64))).numpy()
    if len(und) > MAX_UNDECIDED:
        return und, []
    out = []
    for pick in itertools.product((0, 1), repeat=len(und)):
        q = base.copy()
        for (n, cols, lo, hi), b in zip(und, pick):
            q[n, cols] = hi if b else lo
        out.append(q)
    out.sort(key=lambda q: not np.array_equal(q, base))
    return und, out


def _head_holds(got, blocks, r, quant, A):
    """dz and the four head blocks against one head-only reference, without printing."""
    g = np.asarray(got["dz"], np.float64)
    if quant:
        worst, share, _ = rs.bf16_figures(g, r["t"]["dz"])
        ok = worst <= 1.0 and share <= CAP
    else:
        ok = rs.f32_figures(g, r["t"]["dz"]) <= F32_NORMWISE
    return ok and all(rs.rel_l2(blocks[k], r["grads"][k]) <= BLOCK_RL2 for k in DQN_HEAD_BLOCKS)


def dqn_resolve_head(shape, got, blocks, ref, quant, label):
    """The head stage's hazard (test_gpu_dqn_stages.py): dz, d wh and d bh hang on the bf16
    rounding of dH, which the kernel takes from fp32 values.  For every assignment of the
    undecided decisions (at most MAX_UNDECIDED, else the case fails) the head-only reference is
    evaluated with that rounded dH; the first under which dz, wa, ba, wc and bc hold TOGETHER
    replaces the reference's own.  -> (ref with dz and the head blocks of the chosen assignment,
    violations).  Nothing is widened: with no such assignment the reference stays as it was and
    the ordinary checks report what fails."""
    if not quant:
        return ref, []
    flat0, batch = inputs(shape)
    A = shape[2]
    und, cands = dqn_head_assignments(ref["t"]["dH"], batch[1], A)
    print(f"{label} dH: {len(und)} undecided rounding decisions (row, column, lower, upper) "
          f"{[(n, cols[0], lo, hi) for n, cols, lo, hi in und[:8]]}")
    if not cands:
        return ref, [f"dH: {len(und)} undecided rounding decisions > {MAX_UNDECIDED}"]
    for i, qdH in enumerate(cands):
        if i == 0 and "dz" in ref["t"] and len(cands) == 1:
            return ref, []  # (nothing undecided: the reference's own rounding is the only one)
        kw = dict(case_kw(shape), head_only=True)
        r = rs.run(flat0, batch, given=dict(got, qdH=qdH), quant=True, **kw)
        if _head_holds(got, blocks, r, quant, A):
            print(f"{label} dH: assignment {i} of {len(cands)} holds dz and the head blocks together")
            out = dict(ref, t=dict(ref["t"], dz=r["t"]["dz"]), grads=dict(ref["grads"]))
            out["grads"].update({k: r["grads"][k] for k in DQN_HEAD_BLOCKS})
            return out, []
    print(f"{label} dH: no assignment of {len(cands)} holds dz and the head blocks together")
    return ref, []


def hold_dqn_prio(prio, ref, batch, label):
    """|prio - |target - q_ref|| <= 1e-5 (|q_ref| + rms q_ref + |target|): the heads' normwise
    bound carried through one subtraction."""
    q = np.asarray(ref["q"], np.float64)
    t = np.asarray(batch[2], np.float64).reshape(-1)
    p = np.asarray(prio, np.float64).reshape(-1)
    tol = PRIO_NORMWISE * (np.abs(q) + np.sqrt(np.mean(q * q)) + np.abs(t))
    w = float(np.max(np.abs(p - np.abs(t - q)) / (tol + 1e-300))) if np.isfinite(p).all() else np.inf
    print(f"{label} prio   worst |d| / (1e-5 (|q| + rms q + |target|)) {w:.3f}")
    return [f"priorities: bound x{w:.3f}"] if not w <= 1.0 else []


def hold_dqn_metrics(got, ref, label):
    """q normwise against mean |q_a| (as train/pg against pg_abs); target, priorities, loss
    1e-5 relative."""
    m = ref["met"]
    bad, line = [], []
    for k, g in zip(DQN_MET_NAMES, got):
        scale = abs(m["q"]) + m["q_abs"] if k == "q" else abs(m[k])
        v = abs(float(g) - m[k]) / max(scale, 1e-30)
        line.append(f"{k} {v:.1e}")
        if not v <= MET_RTOL:
            bad.append(f"metric {k}: {v:.2e}")
    print(f"{label} metrics rel: " + ", ".join(line))
    return bad


def hold_dqn_q(q, heads, A, label):
    """dqn_forward's q [n,A] against the dueling formula on the exported heads: each element
    within (A + 3) 2^-24 (|v| + |adv_k| + mean |adv|) -- dqn_q_kernel does A + 3 fp32 roundings
    (A - 1 in the sum, the division, v + adv_k, the subtraction, and one to spare)."""
    hd = np.asarray(heads, np.float64)
    adv, v = hd[:, :A], hd[:, rs.VCOL:rs.VCOL + 1]
    want = (v + adv) - adv.mean(1, keepdims=True)
    tol = (A + 3) * 2.0 ** -24 * (np.abs(v) + np.abs(adv) + np.abs(adv).mean(1, keepdims=True))
    w = float(np.max(np.abs(np.asarray(q, np.float64) - want) / (tol + 1e-300)))
    print(f"{label} q      worst |d| / ((A + 3) 2^-24 (|v| + |adv_k| + mean |adv|)) {w:.3f}")
    return [f"q: bound x{w:.3f}"] if not w <= 1.0 else []


# ------------------------------------------------------------------------------ IQN forward
# The distributional actor path's forward (tests/test_gpu_iqn_stages.py; the module docstring there
# has the cases' reasons).  A case is ("iqn", frames n, quantiles W, A, target net?); the stages and
# the bounds are those above, y held as a tensor of the compute type over R = n W rows.
IQN_SMALL = [(1, 1, 2), (3, 8, 6), (2, 5, 15), (1, 32, 15), (5, 32, 15)]
IQN_CASES = [("iqn",) + s + (t,) for s in IQN_SMALL for t in (False, True)]
IQN_LARGE = ("iqn", 63, 31, 6, False)  # R = 1953 = 16 * 122 + 1: past the FC's grid cap
IQN_STALE = (("iqn", 5, 32, 15, False), ("iqn", 1, 32, 15, False))  # the second after the first
IQN_MAX_UNDECIDED = 3      # undecided elements of one row of the cosine tile
IQN_LARGE_UNDECIDED = 0.02  # share of the large case's rows that may hold one
# the seed of a case's taus, iqn_oracle.edge_taus(n, W, seed): the first seed >= n (test_gpu_iqn.py
# uses n) at which NO element of the bf16 cosine tile is undecided (rs.iqn_undecided: 8 fp32 ulps
# of margin) and the stand-in's share of elements != RNE stays under STAND_IN_CAP for every
# tensor; the large case's: the first >= n that leaves at most 1 % of its rows undecided and none
# with more than IQN_MAX_UNDECIDED elements.  test_ref_stages_host.py asserts all of it.
# Undecided rows by seed, on the reference alone: (2, 5) seed 2: 1; (1, 32) seeds 1, 2: 1, 3;
# (5, 32) seeds 5..10: 3, 1, 2, 3, 4, 3; (63, 31) seeds 63, 64: 25, 27 of 1953, seed 65: 16 (0.8 %).
IQN_TAU_SEEDS = {(1, 1): 1, (3, 8): 3, (2, 5): 3, (1, 32): 3, (5, 32): 11, (63, 31): 65}

_IQN_FLAT = {}


def iqn_flats(A):
    """(online, nudged target) of test_gpu_iqn.py's edge shapes: iqn_oracle.fixture_params, every
    bias and the LayerNorm affine off 0 / 1."""
    import iqn_oracle as orc
    if A not in _IQN_FLAT:
        online = orc.fixture_params(A, 31 + A)
        target = (online + 0.05 * (orc.fixture_params(A, 32 + A) - online)).astype(np.float32)
        _IQN_FLAT[A] = (online, target)
    return _IQN_FLAT[A]


def iqn_taus(n, W):
    import iqn_oracle as orc
    return orc.edge_taus(n, W, seed=IQN_TAU_SEEDS[(n, W)])


def _iqn_inputs(shape):
    import iqn_oracle as orc
    _, n, W, A, tgt = shape
    return iqn_flats(A)[1 if tgt else 0], (orc.fixture_obs(100 + n, n), iqn_taus(n, W))


def iqn_undecided_rows(shape):
    """-> (lower rounding, upper rounding, mask [R,64]) of the case's cosine tile."""
    _, n, W, _, _ = shape
    return rs.iqn_undecided(iqn_taus(n, W).reshape(-1))


def _row_holds(g, r, rms):
    """One row of a bf16 tensor under hold_tensors' two conditions (rms: the whole tensor's)."""
    d = np.abs(g - r)
    want = rs.rne_bf16(torch.from_numpy(np.ascontiguousarray(r))).numpy()
    return bool(np.all(d <= rs.ulp_bf16(r) + 1e-5 * (np.abs(r) + rms)) and np.mean(g != want) <= CAP)


def iqn_resolve_embed(shape, got, ref, quant, label):
    """The embed_ln stage's hazard (test_gpu_iqn_stages.py): the bf16 cosine tile never leaves LDS
    and its rounding is taken from the device cosf.  Rows are independent in this stage: for a row
    with undecided elements (at most IQN_MAX_UNDECIDED, else the case fails) the row of y is
    evaluated under every assignment of them, the reference's own rounding first; the first under
    which the row holds (_row_holds: hold_tensors' conditions on the row) replaces the
    reference's row.  -> (ref with those rows of y, violations).  Nothing is widened: a row no
    assignment holds stays as it was and the ordinary check reports it."""
    import itertools
    if not quant:
        return ref, []
    flat, (_, taus) = inputs(shape)
    n_tau = taus.shape[1]
    lo, hi, und = iqn_undecided_rows(shape)
    cnt = und.sum(1)
    rows = np.nonzero(cnt)[0]
    print(f"{label} cosine tile: {len(rows)} of {len(cnt)} rows hold undecided roundings "
          f"({int(cnt.sum())} elements, at most {int(cnt.max())} in a row)")
    bad = []
    if cnt.max() > IQN_MAX_UNDECIDED:
        bad.append(f"cosine tile: a row with {int(cnt.max())} undecided elements > {IQN_MAX_UNDECIDED}")
    if not len(rows):
        return ref, bad
    W = rs.IqnWeights(flat, shape[3], True)
    act3 = torch.from_numpy(np.ascontiguousarray(got["act3"], dtype=np.float64))
    base = rs.rne_bf16(torch.from_numpy(ref["e"])).numpy()
    y = ref["t"]["y"].copy()
    g = np.asarray(got["y"], np.float64).reshape(y.shape)
    rms = float(np.sqrt(np.mean(y * y)))
    moved = []
    for r in rows:
        idx = np.nonzero(und[r])[0]
        if len(idx) > IQN_MAX_UNDECIDED:
            continue
        cands = []
        for pick in itertools.product((0, 1), repeat=len(idx)):
            e = base[r].copy()
            e[idx] = np.where(np.array(pick, bool), hi[r, idx], lo[r, idx])
            cands.append(e)
        cands.sort(key=lambda e: not np.array_equal(e, base[r]))
        with torch.no_grad():
            Y = rs.iqn_embed_ln_rows(act3[r // n_tau][None].expand(len(cands), -1),
                                     torch.from_numpy(np.stack(cands)), W).numpy()
        for i, yr in enumerate(Y):
            if _row_holds(g[r], yr, rms):
                if not np.array_equal(cands[i], base[r]):
                    y[r] = yr
                    moved.append(int(r))
                break
    print(f"{label} cosine tile: rows held under another assignment than the reference's own: {moved}")
    return dict(ref, t=dict(ref["t"], y=y)), bad


def hold_iqn_forward(shape, got, mask1, q, quant, label, cap=CAP):
    """Every stage of one IQN forward on its own exports -> violations.  The large case holds the
    head stages alone (its trunk is not evaluated)."""
    trunk = shape[:4] != IQN_LARGE[:4]
    A = shape[3]
    ref = reference(shape, got, quant)
    ref, bad = iqn_resolve_embed(shape, got, ref, quant, label)
    bad += hold_tensors(got, ref, rs.IQN_FORWARD_TENSORS if trunk else rs.IQN_HEAD_TENSORS, quant,
                        label, cap)
    if trunk:
        bad += hold_mask(mask1, got["act1"], label)
    bad += hold_dqn_q(np.asarray(q).reshape(-1, A), got["heads"], A, label)
    return bad


# ------------------------------------------------------------------------------ SAC step
# The SAC learner's step (tests/test_gpu_sac_stages.py; CPU: tests/test_sac_stages_host.py), every
# launch of the per-layer path against oracle/sac_stages.py on that launch's own exported inputs.
# A case is (N, D, K); Cp = rup(D + K, 32) and Dp = rup(D, 32) pick the first-layer regime of the
# chain kernels (<= 64 prefetched, <= 256 wide, above: per-layer path only).
SAC_CASES = [
    (1, 1, 1),       # one transition; uniform weights
    (16, 3, 1),      # exactly one row block
    (17, 11, 16),    # one row into the second row block; K = MAXK
    (37, 26, 6),     # D + K = 32 = Cp (no padding) while Dp pads
    (33, 58, 6),     # Cp = 64, the small regime's limit
    (37, 60, 6),     # Dp = 64 small, Cp = 96 wide: mixed regimes
    (100, 111, 8),   # both first layers wide
    (37, 240, 16),   # Cp = 256, the fused limit
    (37, 241, 16),   # Cp = 288: per-layer path only
    (33, 760, 4),    # nsq_c = 2114 > 2048; max_grad_norm 0.05: the clip is active
    (520, 17, 6),    # the smallest probability at index 519
]
SAC_CLIP_CASE, SAC_CLIP_NORM = (33, 760, 4), 0.05
SAC_TAIL_CASE = (520, 17, 6)
SAC_NO_ALPHA = ((520, 17, 6), "fp32")  # tune_alpha=False in this dtype of this case
SAC_LA0 = -0.3
SAC_PARAM_ATOL, SAC_LA_ATOL = 2e-6, 1e-6  # test_gpu_sac.py's header
SAC_SLOT_RTOL = 1e-5
SAC_MAX_TIES = 1
# the batch seed of a case (1000 N + D unless the float32 stand-in exceeded a quarter of a cap
# there, or the reference's actor loss had an undecided row: chosen on the CPU by
# test_sac_stages_host.py's conditions alone).  (37, 26, 6) at 37026: row 26 undecided in bf16;
# (37, 240, 16) at 37240: one of gu's 592 elements != RNE, 1.7e-3 > CAP / 4; (33, 760, 4) at
# 33760..33763: a first layer's fp32 sum over 764 inputs at 2.5e-6 .. 2.7e-6 normwise on the
# stand-in, just over a quarter of 1e-5.
SAC_SEEDS = {(37, 26, 6): 37027, (37, 240, 16): 37241, (33, 760, 4): 33764}
# (the exported gradient blocks are the clipped ones, so the clip -- the slots' sum against the
# exported gradient's own norm, which needs no reference block -- is held before them)
SAC_STAGES = ("layout", "pack", "fwd", "heads", "target_critic", "critic_loss", "critic_bwd",
              "critic_clip", "critic_wgrad", "critic_adam", "weights", "actor_q", "actor_loss",
              "actor_q_dgrad", "actor_head_bwd", "actor_bwd", "actor_clip", "actor_wgrad",
              "actor_adam", "alpha", "metrics")
SAC_KEYS = ("qf1_loss", "qf2_loss", "qf1", "qf2", "qf_loss", "critic_grad_norm", "actor_loss",
            "actor_std", "actor_grad_norm", "alpha_loss", "alpha")


def sac_kw(case, dtype):
    """Engine / reference options of a case in one dtype ("fp32" | "bf16")."""
    return dict(max_grad_norm=SAC_CLIP_NORM if case == SAC_CLIP_CASE else 40.0,
                tune_alpha=(case, dtype) != SAC_NO_ALPHA)


_SAC_IN = {}


def sac_inputs(case, step=0):
    """-> dict(actor0, critic0, tactor0, tcritic0 (flat float32), batch, probs, eps) of a case.
    Parameters: the reference's initialisation (oracle/sac_cpu.py, seeds 3 / 4) with every bias
    moved off 0 and the targets nudged off the online networks, so that no stage can drop a bias
    or read the wrong network and pass.  step = 1: the second step's batch."""
    from oracle import sac_cpu
    from oracle import sac_stages as sst
    if (case, step) in _SAC_IN:
        return _SAC_IN[(case, step)]
    N, D, K = case
    with torch.random.fork_rng(devices=[]):
        a0 = sac_cpu.flat(sac_cpu.make_models(D, K, seed=3)[0].parameters())
        c0 = sac_cpu.flat(sac_cpu.make_models(D, K, seed=4)[1].critic.parameters())
    rng = np.random.default_rng(5)

    def nudge(flat, shapes, reps):
        off = 0
        for _ in range(reps):
            for _, s in shapes:
                k = int(np.prod(s)) if len(s) else 1
                if len(s) <= 1:
                    flat[off:off + k] += (0.02 * rng.standard_normal(k)).astype(np.float32)
                off += k
        assert off == flat.size
    # (a critic's w3 is a vector too: nudged with the biases, harmlessly)
    nudge(a0, sst.actor_shapes(D, K), 1)
    nudge(c0, sst.q_shapes(D, K), 2)
    ta0 = a0 + (0.01 * rng.standard_normal(a0.size)).astype(np.float32) * np.abs(a0).max()
    tc0 = c0 + (0.01 * rng.standard_normal(c0.size)).astype(np.float32) * np.abs(c0).max()
    seed = SAC_SEEDS.get(case, 1000 * N + D) + 7919 * step
    batch = sac_cpu.synthetic_batch(N, D, K, seed)
    r2 = np.random.default_rng(seed + 1)
    probs = None if N == 1 else (r2.uniform(0.5, 2.0, N) / 1000).astype(np.float32)
    if case == SAC_TAIL_CASE:  # the largest weight where only a later round of the loops sees it
        probs[N - 1] = np.float32(0.5) * probs.min()
    eps = r2.standard_normal((3, N, K)).astype(np.float32)
    v = dict(actor0=a0, critic0=c0, tactor0=ta0.astype(np.float32), tcritic0=tc0.astype(np.float32),
             batch=batch, probs=probs, eps=eps)
    _SAC_IN[(case, step)] = v
    return v


def sac_reference(case, dtype, given=None, quant=None, torch_dtype=torch.float64, defect=None):
    from oracle import sac_stages as sst
    i = sac_inputs(case)
    return sst.run(case[1], case[2], i["actor0"], i["critic0"], SAC_LA0, i["batch"], i["probs"],
                   i["eps"], tactor0=i["tactor0"], tcritic0=i["tcritic0"], given=given,
                   quant=(dtype == "bf16") if quant is None else quant, dtype=torch_dtype,
                   defect=defect, **sac_kw(case, dtype))


def _rup(x, m):
    return (x + m - 1) // m * m


def sac_dims(case):
    N, D, K = case
    return dict(N=N, D=D, K=K, DK=D + K, Np=_rup(N, 32), Dp=_rup(D, 32), Cp=_rup(D + K, 32),
                Dt=_rup(D + 1, 16), Ct=_rup(D + K + 1, 16))


def sac_export(run_out, case, dtype, defect=None):
    """What a device whose kernels computed `run_out` (a chained float32 run: the stand-in) would
    export: (raw workspace buffers by sac_debug_info's names, padded as the kernels lay them out;
    the bound state after the step).  defect "pad_col": a non-zero padded column in xct."""
    from oracle import sac_stages as sst
    d = sac_dims(case)
    N, D, K, DK, Np = d["N"], d["D"], d["K"], d["DK"], d["Np"]
    t = run_out["t"]
    raw = {}

    def rm(x, ld):  # row-major [Np][ld]
        b = np.zeros((Np, ld), np.float32)
        b[:N, :x.shape[1]] = x
        return b

    def tr(x, rows, ones=False):  # transposed [rows][Np]
        b = np.zeros((rows, Np), np.float32)
        b[:x.shape[1], :N] = x.T
        if ones:
            b[x.shape[1], :N] = 1.0
        return b
    raw["xs"], raw["xs1"] = rm(t["xs"], d["Dp"]), rm(t["xs1"], d["Dp"])
    for k in ("xc", "xt", "xp"):
        raw[k] = rm(t[k], d["Cp"])
    raw["xst"], raw["xct"] = tr(t["xs"], d["Dt"], True), tr(t["xc"], d["Ct"], True)
    if defect == "pad_col":
        raw["xct"][1 % DK, Np - 1] = 0.5
    for k in sst.HID:
        if k in t:
            raw[k] = rm(t[k], sst.H)
    for k in ("hc1_0", "hc1_1", "hc2_0", "hc2_1", "ha1", "ha2"):
        n, q = (k.split("_") + [None])[:2]
        raw[n + "t" + ("_" + q if q else "")] = tr(t[k], 272, True)
    for q in ("0", "1"):
        raw["dh2_" + q], raw["dh2t_" + q] = rm(t["dh2_" + q], sst.H), tr(t["dh2_" + q], sst.H)
        raw["dhc1t_" + q] = tr(t["dhc1_" + q], sst.H)
        raw["dhp2_" + q], raw["dhp1_" + q] = rm(t["dhp2_" + q], sst.H), rm(t["dhp1_" + q], sst.H)
        raw["dqt_" + q] = tr(t["dq_" + q][:, None], 16)
    raw["dha2"], raw["dha2t"] = rm(t["dha2"], sst.H), tr(t["dha2"], sst.H)
    raw["dha1t"], raw["gmt"], raw["gut"] = tr(t["dha1"], sst.H), tr(t["gm"], 16), tr(t["gu"], 16)
    for k in ("q1", "q2", "logp1", "logp", "logp2"):
        if k in t:
            raw[k] = np.zeros((1, Np), np.float32)
            raw[k][0, :N] = t[k]
    raw["save"] = t["save"].reshape(4, N * K).astype(np.float32)
    raw["rowm"] = np.zeros((8, Np), np.float32)
    raw["rowm"][:6, :N] = t["rowm"]
    f32 = lambda x: np.asarray(x, np.float32)  # noqa: E731
    cg = np.concatenate([run_out["cgrads"][k].reshape(-1) for k in sst.C_BLOCKS])
    ag = np.concatenate([run_out["agrads"][k].reshape(-1) for k in sst.A_BLOCKS])
    raw["sq_c"] = np.array([[float(cg @ cg), 0.0]], np.float32)
    raw["sq_a"] = np.array([[float(ag @ ag), 0.0]], np.float32)
    la = run_out["la"]
    met = np.zeros(12, np.float32)
    met[:11] = [run_out["met"][k] for k in SAC_KEYS]
    state = dict(actor=f32(run_out["actor1"]), critic=f32(run_out["critic1"]),
                 tactor=f32(run_out["tactor1"]), tcritic=f32(run_out["tcritic1"]),
                 actor_grad=f32(ag * run_out["acoef"]), critic_grad=f32(cg * run_out["ccoef"]),
                 actor_m=f32(run_out["am"]), actor_v=f32(run_out["av"]), critic_m=f32(run_out["cm"]),
                 critic_v=f32(run_out["cv"]), la_buf=f32([la["la"], la["g"], la["m"], la["v"]]),
                 metrics=met, prio=f32(t["prio"]))
    q_ = (lambda x: rs.rne_bf16(torch.from_numpy(f32(x))).numpy()) if dtype == "bf16" else f32
    for name, flat, split, in1 in (("ka", state["actor"], "a", D), ("kta", state["tactor"], "a", D),
                                   ("kq", state["critic"], "c", DK), ("ktq", state["tcritic"], "c", DK)):
        nets = [sst.split_actor(flat, D, K)] if split == "a" else sst.split_critic(flat, D, K)
        for q, P in enumerate(nets):
            pre = name if split == "a" else f"{name}{q}"
            w1 = np.zeros((sst.H, _rup(in1, 32)), np.float32)
            w1[:, :in1] = q_(P["w1"].numpy())
            raw[pre + "_w1"], raw[pre + "_w2"] = w1, q_(P["w2"].numpy())
            if name in ("ka", "kq"):
                raw[pre + "_w2t"] = np.ascontiguousarray(raw[pre + "_w2"].T)
    return raw, state


class _Bad(list):
    """Violations, each under the stage that owns it."""

    def add(self, stage, msg):
        assert stage in SAC_STAGES
        self.append((stage, msg))

    def first_stage(self):
        return min((SAC_STAGES.index(s) for s, _ in self), default=None)


def sac_logical(raw, case, tune_alpha, bad):
    """Strip the padding of the exported buffers -> the logical tensors (oracle/sac_stages.py).
    Holds on the way (stage "layout"): every padded row or column is exactly 0, every transposed
    copy equals its row-major tensor bit for bit, every ones row is 1."""
    from oracle import sac_stages as sst
    d = sac_dims(case)
    N, D, K, DK, Np = d["N"], d["D"], d["K"], d["DK"], d["Np"]
    t = {}

    def zero(name, buf, *regions):
        n = sum(int(np.count_nonzero(buf[r])) for r in regions)
        if n:
            bad.add("layout", f"{name}: {n} non-zero padded elements")

    def rm(name, cols):
        b = raw[name]
        assert b.shape[0] == Np, (name, b.shape)
        zero(name, b, np.s_[N:, :], np.s_[:N, cols:])
        return b[:N, :cols]

    def tr(name, rows, of=None, ones=False):
        b = raw[name]
        assert b.shape[1] == Np, (name, b.shape)
        zero(name, b, np.s_[:, N:], np.s_[rows + (1 if ones else 0):, :N])
        if ones and not np.all(b[rows, :N] == 1.0):
            bad.add("layout", f"{name}: the ones row is not 1")
        x = np.ascontiguousarray(b[:rows, :N].T)
        if of is not None and not np.array_equal(x, of):
            bad.add("layout", f"{name}: {int(np.sum(x != of))} elements differ from the row-major tensor")
        return x
    t["xs"], t["xs1"] = rm("xs", D), rm("xs1", D)
    for k in ("xc", "xt", "xp"):
        t[k] = rm(k, DK)
    tr("xst", D, t["xs"], True)
    tr("xct", DK, t["xc"], True)
    for k in sst.HID:
        if k in raw and (tune_alpha or k not in ("hb1", "hb2")):
            t[k] = rm(k, sst.H)
    for k in ("hc1_0", "hc1_1", "hc2_0", "hc2_1", "ha1", "ha2"):
        n, q = (k.split("_") + [None])[:2]
        tr(n + "t" + ("_" + q if q else ""), sst.H, t[k], True)
    for q in ("0", "1"):
        t["dh2_" + q] = rm("dh2_" + q, sst.H)
        tr("dh2t_" + q, sst.H, t["dh2_" + q])
        t["dhc1_" + q] = tr("dhc1t_" + q, sst.H)
        t["dhp2_" + q], t["dhp1_" + q] = rm("dhp2_" + q, sst.H), rm("dhp1_" + q, sst.H)
        t["dq_" + q] = tr("dqt_" + q, 1)[:, 0]
    t["dha2"] = rm("dha2", sst.H)
    tr("dha2t", sst.H, t["dha2"])
    t["dha1"], t["gm"], t["gu"] = tr("dha1t", sst.H), tr("gmt", K), tr("gut", K)
    for k in ("q1", "q2", "logp1", "logp") + (("logp2",) if tune_alpha else ()):
        zero(k, raw[k], np.s_[:, N:])
        t[k] = raw[k][0, :N]
    t["save"] = raw["save"].reshape(4, N, K)
    zero("rowm", raw["rowm"], np.s_[:, N:], np.s_[6:, :N])
    t["rowm"] = raw["rowm"][:6, :N]
    return t


_SAC_STAGE_OF = {}
for _k in ("hta1", "hta2", "ha1", "ha2", "hc1_0", "hc1_1", "hc2_0", "hc2_1"):
    _SAC_STAGE_OF[_k] = "fwd"
for _k in ("xt", "xp", "logp1", "logp", "save", "q1", "q2"):
    _SAC_STAGE_OF[_k] = "heads"
for _k in ("htc1_0", "htc1_1", "htc2_0", "htc2_1"):
    _SAC_STAGE_OF[_k] = "target_critic"
for _k in ("dq_0", "dq_1", "dh2_0", "dh2_1", "prio"):
    _SAC_STAGE_OF[_k] = "critic_loss"
for _k in ("dhc1_0", "dhc1_1"):
    _SAC_STAGE_OF[_k] = "critic_bwd"
for _k in ("hp1_0", "hp1_1", "hp2_0", "hp2_1"):
    _SAC_STAGE_OF[_k] = "actor_q"
for _k in ("dhp2_0", "dhp2_1"):
    _SAC_STAGE_OF[_k] = "actor_loss"
for _k in ("dhp1_0", "dhp1_1"):
    _SAC_STAGE_OF[_k] = "actor_q_dgrad"
for _k in ("gm", "gu", "dha2"):
    _SAC_STAGE_OF[_k] = "actor_head_bwd"
_SAC_STAGE_OF["dha1"] = "actor_bwd"
for _k in ("hb1", "hb2", "logp2"):
    _SAC_STAGE_OF[_k] = "alpha"
SAC_ROWM = ("qf1_term", "qf2_term", "q1", "q2", "actor_term", "std_mean")
SAC_ROWM_STAGE = ("critic_loss", "critic_loss", "critic_loss", "critic_loss", "actor_loss", "heads")
SAC_SAVE = ("std", "y", "x-mean", "tanh_u")


def _hold_one(bad, fig, stage, name, g, r, as_t, label, cap):
    """One tensor under the bf16 (as_t) or the fp32 bound; figures into `fig` and printed."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    if not np.isfinite(g).all():
        bad.add(stage, f"{name}: not finite")
        return
    if as_t:
        worst, share, wu = rs.bf16_figures(g, r)
        fig[name] = (worst, share)
        print(f"{label} {name:10s} worst |d| / (ulp + 1e-5 (|r| + rms)) {worst:.3f}, share != RNE "
              f"{share:.2e} (worst {wu:.2f} ulp)")
        if worst > 1.0:
            bad.add(stage, f"{name}: element bound x{worst:.3f}")
        if share > cap:
            bad.add(stage, f"{name}: mismatch share {share:.2e} > {cap:.2e}")
    else:
        w = rs.f32_figures(g, r)
        fig[name] = (w,)
        print(f"{label} {name:10s} normwise {w:.2e}")
        if w > F32_NORMWISE * (cap / CAP):
            bad.add(stage, f"{name}: normwise {w:.2e}")


def hold_sac_step(raw, state, case, dtype, label, cap=CAP):
    """Every stage of one SAC step (from zero Adam state) on the step's own exports -> (the
    violations, each under its stage; the figures).  cap: CAP for the device, STAND_IN_CAP for the
    stand-in, which scales every other bound by the same quarter."""
    from oracle import sac_stages as sst
    N, D, K = case
    quant = dtype == "bf16"
    kw = sac_kw(case, dtype)
    tune = kw["tune_alpha"]
    scale = cap / CAP
    i = sac_inputs(case)
    bad, fig = _Bad(), {}
    t = sac_logical(raw, case, tune, bad)
    # ---- pack: exact
    s, a, r_, s1, _ = i["batch"]
    p = sst.pack(*(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(N, -1))
                   for x in (s, a, s1)), quant)
    for k, want in (("xs", p["xs"]), ("xs1", p["xs1"]), ("xc", p["xc"]), ("xt", p["xt_obs"]),
                    ("xp", p["xp_obs"])):
        want = want.numpy().astype(np.float32)
        n = int(np.sum(t[k][:, :want.shape[1]] != want))
        if n:
            bad.add("pack", f"{k}: {n} elements are not RNE of the fp32 source")
    print(f"{label} pack       exact")
    given = dict(t, critic1=state["critic"], actor1=state["actor"], critic_grad=state["critic_grad"],
                 actor_grad=state["actor_grad"])
    ref = sac_reference(case, dtype, given=given)
    # ---- tensors, in launch order
    names = [k for k in sst.T_TENSORS + sst.F32_TENSORS if k in _SAC_STAGE_OF and (tune or _SAC_STAGE_OF[k] != "alpha")]
    names.sort(key=lambda k: SAC_STAGES.index(_SAC_STAGE_OF[k]))
    for k in names:
        g = state["prio"] if k == "prio" else t[k]
        if k == "save":
            for j, nm in enumerate(SAC_SAVE):
                _hold_one(bad, fig, "heads", "save." + nm, g[j], ref["t"][k][j], False, label, cap)
            continue
        cols = np.s_[:, D:] if k in ("xt", "xp") else np.s_[...]
        _hold_one(bad, fig, _SAC_STAGE_OF[k], k, g[cols], ref["t"][k][cols], quant and k in sst.T_TENSORS,
                  label, cap)
    for j, nm in enumerate(SAC_ROWM):
        _hold_one(bad, fig, SAC_ROWM_STAGE[j], "rowm." + nm, t["rowm"][j], ref["t"]["rowm"][j], False,
                  label, cap)
    und = ref["undecided"]
    fig["undecided"] = len(und)
    print(f"{label} actor loss: {len(und)} undecided rows {und[:4]} (assigned {ref['assign']})")
    if len(und) > SAC_MAX_TIES:
        bad.add("actor_loss", f"{len(und)} undecided rows > {SAC_MAX_TIES}")
    # ---- gradient blocks (the reference scaled by its own clip coefficient), clip, Adam
    for net, blocks, gk, names_b, sq in (("critic", sst.critic_blocks, "cgrads", sst.C_BLOCKS, "sq_c"),
                                         ("actor", sst.actor_blocks, "agrads", sst.A_BLOCKS, "sq_a")):
        got = blocks(state[net + "_grad"], D, K)
        rnorm = ref["cnorm" if net == "critic" else "anorm"]
        coef = ref["ccoef" if net == "critic" else "acoef"]
        line = []
        for k in names_b:
            v = rs.rel_l2(got[k], ref[gk][k] * coef)
            line.append(f"{k} {v:.1e}")
            fig[f"{net}.{k}"] = (v,)
            if not v <= BLOCK_RL2 * scale:
                bad.add(net + "_wgrad", f"block {k}: rel-L2 {v:.2e}")
        print(f"{label} {net} blocks rel-L2: " + ", ".join(line))
        slots = float(np.sum(np.asarray(raw[sq], np.float64)))
        g = np.asarray(state[net + "_grad"], np.float64)
        c_dev = sst.clip_coef(math.sqrt(slots), kw["max_grad_norm"])
        v = abs(float(g @ g) - c_dev ** 2 * slots) / max(c_dev ** 2 * slots, 1e-300)
        mi = 5 if net == "critic" else 8
        gn = abs(float(state["metrics"][mi]) - rnorm) / rnorm
        gs = abs(float(state["metrics"][mi]) - math.sqrt(slots)) / math.sqrt(slots)
        fig[f"{net}.clip"] = (v, gn, coef)
        print(f"{label} {net} clip: coefficient {coef:.4f} (norm {rnorm:.4e}); |g|^2 against coef^2 x the "
              f"slots' sum {v:.1e}; grad-norm metric against the reference {gn:.1e}, the slots {gs:.1e}")
        if not v <= SAC_SLOT_RTOL:
            bad.add(net + "_clip", f"|g|^2 against coef^2 x the slots' sum: {v:.2e}")
        if not gs <= GRAD_NORM_RTOL * scale:
            bad.add(net + "_clip", f"grad-norm metric against the slots: {gs:.2e}")
        if not gn <= GRAD_NORM_RTOL * scale:
            bad.add(net + "_wgrad", f"grad-norm metric against the reference: {gn:.2e}")
        line = []
        for k, gotv, want, tol in ((net, state[net], ref[net + "1"], SAC_PARAM_ATOL),
                                   ("t" + net, state["t" + net], ref["t" + net + "1"], SAC_PARAM_ATOL)):
            v = float(np.max(np.abs(np.asarray(gotv, np.float64) - want)))
            line.append(f"{k} {v:.1e}")
            fig[f"{k}.adam"] = (v,)
            if not v <= tol * scale:
                bad.add(net + "_adam", f"{k} after Adam: max |d| {v:.2e}")
        for k, want in ((net + "_m", ref[net[0] + "m"]), (net + "_v", ref[net[0] + "v"])):
            v = rs.f32_figures(state[k], want)
            line.append(f"{k} {v:.1e}")
            if not v <= F32_NORMWISE * scale:
                bad.add(net + "_adam", f"{k}: normwise {v:.2e}")
        print(f"{label} {net} Adam (given the device's clipped gradient) max |d|: " + ", ".join(line))
    # ---- the re-emitted kernel layouts: exact
    q_ = (lambda x: rs.rne_bf16(torch.from_numpy(np.asarray(x, np.float32))).numpy()) if quant else \
        (lambda x: np.asarray(x, np.float32))
    for name, flat, split, in1 in (("ka", state["actor"], "a", D), ("kta", state["tactor"], "a", D),
                                   ("kq", state["critic"], "c", D + K), ("ktq", state["tcritic"], "c", D + K)):
        nets = [sst.split_actor(flat, D, K, torch.float32)] if split == "a" else \
            sst.split_critic(flat, D, K, torch.float32)
        for q, P in enumerate(nets):
            pre = name if split == "a" else f"{name}{q}"
            w1 = raw[pre + "_w1"]
            n = int(np.sum(w1[:, :in1] != q_(P["w1"].numpy()))) + int(np.count_nonzero(w1[:, in1:]))
            n += int(np.sum(raw[pre + "_w2"] != q_(P["w2"].numpy())))
            if pre + "_w2t" in raw:
                n += int(np.sum(raw[pre + "_w2t"] != raw[pre + "_w2"].T))
            if n:
                bad.add("weights", f"{pre}: {n} elements are not RNE of the fp32 master (or padding != 0)")
    print(f"{label} weights    exact")
    # ---- alpha and the metrics
    la = np.asarray(state["la_buf"], np.float64)
    if tune:
        rl = ref["la"]
        v = abs(la[0] - rl["la"])
        fig["log_alpha"] = (v,)
        print(f"{label} log_alpha |d| {v:.1e}; grad rel {abs(la[1] - rl['g']) / abs(rl['g']):.1e}")
        if not v <= SAC_LA_ATOL * scale:
            bad.add("alpha", f"log_alpha: |d| {v:.2e}")
        for j, k in ((1, "g"), (2, "m"), (3, "v")):
            if not abs(la[j] - rl[k]) <= MET_RTOL * scale * abs(rl[k]):
                bad.add("alpha", f"log_alpha {k}: {la[j]} against {rl[k]}")
    elif la[0] != np.float32(SAC_LA0) or np.any(la[1:] != 0):
        bad.add("alpha", f"log_alpha moved with tune_alpha off: {la}")
    line = []
    for j, k in enumerate(SAC_KEYS):
        if k.endswith("grad_norm") or (not tune and k in ("alpha_loss", "alpha")):
            continue
        v = abs(float(state["metrics"][j]) - ref["met"][k]) / max(abs(ref["met"][k]), 1e-30)
        line.append(f"{k} {v:.1e}")
        fig["met." + k] = (v,)
        if not v <= MET_RTOL * scale:
            bad.add("metrics", f"metric {k}: {v:.2e}")
    print(f"{label} metrics rel: " + ", ".join(line))
    return bad, fig, ref


# ---- the policy head where 1 - y^2 is small (sac_policy, forward only)
SAC_POLICY_CASE = (5, 17, 6)  # n, D, K
SAC_POLICY_BM = (0.5, 3.0, 6.0, 9.5, -9.5, 12.0)  # fc_mean's bias: |x| > 9 in three columns
SAC_U = 2.0 ** -24  # fp32's unit roundoff: |fl(a) - a| <= u |a|
SAC_TANH_ULPS = 4   # |y - tanh x| <= 4 x 2^-24: tanhf within 2 ulp of a value below 1 (spacing 2^-24), doubled


def sac_policy_inputs():
    """-> (actor flat float32 with fc_mean's bias raised, obs [n, D], noise [n, K])."""
    from oracle import sac_stages as sst
    n, D, K = SAC_POLICY_CASE
    a0 = sac_inputs((37, D, K))["actor0"].copy()
    off = sum(int(np.prod(s)) for _, s in sst.actor_shapes(D, K)[:5])
    a0[off:off + K] = np.asarray(SAC_POLICY_BM, np.float32)
    rng = np.random.default_rng(11)
    return a0, rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, K)).astype(np.float32)


def hold_sac_policy(mean, std, y, logp, eps, label, share=1.0):
    """sac_policy's y and log-prob on the head's own float32 mean and std -> violations.

    x = fl(mean + fl(eps std)) and x - mean = fl(x - mean) are single correctly rounded fp32
    operations of exported numbers, so they are reproduced exactly here.  y is held to tanh x
    within SAC_TANH_ULPS.  logp is held to the formula in float64 on (x - mean, std, y):
        logp = sum_k -A_k - log std_k - log sqrt(2 pi) - L_k,   A = (x - mean)^2 / (2 std^2),
        L = log z,  z = 1 - y^2 + 1e-6.
    The kernel's z takes three roundings: fl(y y) errs by at most u y^2 <= u; 1 - fl(y y) is exact
    where fl(y y) >= 1/2 (Sterbenz) and errs by at most u otherwise; adding 1e-6f errs by u z (the
    constant itself by 1e-6 u).  So |dz| <= 2 u + u z: RELATIVE to z that is 2 u / z + u, which at
    z = 1e-6 (y one spacing from 1) is 0.12 -- this is the ill-conditioning, in torch as much as
    here -- and at y = +-1 exactly is 0 (1 - 1 = 0 and 0 + 1e-6f are exact).  Through the
    logarithm: |dL| <= -log(1 - |dz| / z) + 2 u |L| (logf within 2 ulp).  The other terms:
    A takes four roundings (4 u A), log std 2 u |log std|; the 4 K subtractions and additions that
    build logp err by at most u S each, S = sum_k (A + |log std| + log sqrt(2 pi) + |L|).  The
    bound is the sum; `share` scales it (1/4 for the stand-in)."""
    u = SAC_U
    m32, s32, e32 = (np.asarray(v, np.float32) for v in (mean, std, eps))
    x32 = (m32 + e32 * s32).astype(np.float32)
    xm = (x32 - m32).astype(np.float64)
    sd, yy = s32.astype(np.float64), np.asarray(y, np.float64)
    bad = []
    if not all(np.isfinite(np.asarray(v, np.float64)).all() for v in (mean, std, y, logp)):
        return ["policy: not finite"]
    dy = float(np.max(np.abs(yy - np.tanh(x32.astype(np.float64)))))
    z = (1.0 - yy * yy) + 1e-6
    A, L = xm * xm / (2.0 * sd * sd), np.log(z)
    want = (-A - np.log(sd) - math.log(math.sqrt(2 * math.pi)) - L).sum(-1)
    dz = np.where(np.abs(yy) == 1.0, 0.0, 2 * u + u * z)
    S = (A + np.abs(np.log(sd)) + math.log(math.sqrt(2 * math.pi)) + np.abs(L)).sum(-1)
    bound = (-np.log1p(-dz / z) + 2 * u * np.abs(L) + 4 * u * A + 2 * u * np.abs(np.log(sd))).sum(-1) \
        + 4 * yy.shape[1] * u * S
    w = float(np.max(np.abs(np.asarray(logp, np.float64) - want) / bound))
    print(f"{label} |x| max {np.abs(x32).max():.2f}, y == +-1 in {int(np.sum(np.abs(yy) == 1.0))} elements, "
          f"smallest z {z.min():.2e}; |y - tanh x| max {dy / u:.2f} x 2^-24; logp |d| / bound {w:.3f} "
          f"(bounds {bound.min():.1e} .. {bound.max():.1e})")
    if not np.abs(x32).max() > 9 or not np.any(np.abs(yy) == 1.0):
        bad.append("policy: the case does not reach |x| > 9 and y == +-1")
    if not dy <= SAC_TANH_ULPS * u:
        bad.append(f"policy: |y - tanh x| {dy / u:.2f} x 2^-24")
    if not w <= share:
        bad.append(f"policy: logp bound x{w:.3f}")
    return bad
