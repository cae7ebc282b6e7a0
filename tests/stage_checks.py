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
after these; the IQN actor path's forward (tests/test_gpu_iqn_stages.py) is the last section.
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
