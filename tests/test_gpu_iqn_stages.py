"""Every stage of the distributional (IQN) actor path's forward held to float64 on the forward's
own tensors (teacher forcing), in bf16 and in fp32, as tests/test_gpu_dqn_stages.py holds the
Ape-X DQN step; and iqn_act held bit for bit to the kernel's own forwards.

Each forward case runs ONE IqnEngine.forward, exports the workspace (IqnEngine.debug_tensor:
act1, act2, act3 and mask1 of the conv trunk, which the handle runs in trunk-only mode; y, zg, h
and heads of the quantile head over R = n W rows) and evaluates each stage's float64 reference
(oracle/ref_stages.py, algo="iqn") on the tensors that stage read:
  trunk     conv1, conv2, conv3 without the LayerNorm, and mask1
  embed_ln  y from the exported act3 and the given taus: the cosine tile, Wq e + bq on the MFMAs,
            erf-GELU, the modulation by act3[r // W] and the two-pass LayerNorm in one kernel
  fc/heads  the 512-wide FcFwd / HeadsFwd over R rows (the persistent loop of the FC past its
            grid cap at the large case)
  q         iqn_q_kernel on the exported heads

Bounds: those of tests/stage_checks.py, unchanged -- fp32 tensors normwise 1e-5; bf16 tensors
within one ulp and equal to RNE except on a share of at most CAP = 5e-3; q within (A + 3) 2^-24
(|v| + |adv_k| + mean |adv|) (hold_dqn_q: iqn_q_kernel does dqn_q_kernel's A + 3 roundings).
The fp32 mode's y rests on the device cosf against the float64 cosine of the SAME float32
argument (fl(fl(pi) i) tau, formed as the kernel and torch form it): an error of a few 2^-24 on
|e| <= 1, far inside 1e-5.

The hazard of embed_ln in bf16: the cosine tile never leaves LDS and its rounding is taken from
the device cosf; an element whose float64 value lies within cosf's error of a bf16 rounding
boundary can round the other way, which moves its whole row of y by about 1e-3 relative.  It is
handled, not tolerated: an element is undecided when the float64 cosine is within the margin of a
boundary -- twice cosf's maximum error, ASSUMED to be 4 fp32 ulps (the HIP programming guide's
table of device math functions, the source of the DQN stage test's powf figure, is not at hand),
so 8 fp32 ulps of the cosine (rs.iqn_undecided); rows are independent in this stage, so for a row
with undecided elements (at most 3, else the case fails) the row of y is evaluated under every
assignment and the first under which the row holds replaces the reference's own
(stage_checks.iqn_resolve_embed).  The taus' seeds leave NO undecided element at the small cases
and 16 of 1953 rows (0.8 %) with one each at the large case (test_ref_stages_host.py asserts it).

Cases (parameters: iqn_oracle.fixture_params, every bias and the LayerNorm affine off 0 / 1, the
target net nudged; taus: iqn_oracle.edge_taus, holding 0 and the two largest float32 below 1; one
handle per (A, W, dtype)):
  small   (n, W, A) = (1, 1, 2): one row, 15 clamped rows in the tile; (3, 8, 6): a tile spanning
          frames, then a ragged one; (2, 5, 15): W no power of two; (1, 32, 15): one frame over two
          tiles; (5, 32, 15); each on the online and on the target net (its own packed Wq)
  stale   n = 1 after n = 5 on the handle of (15, 32): rows >= R of the workspace hold the larger
          forward's values, and must still hold them afterwards
  large   n = 63, W = 31, A = 6: R = 1953 = 16 * 122 + 1, so the last embed tile has one valid row
          and the FC's last row tile is ragged in both tilings; the FC's grid is capped at 3 x CUs
          tiles, and ceil(R / 80) * 32 (fp32) and ceil(R / 32) * 16 (bf16) exceed it (asserted from
          the device's CU count): the loop body runs more than once.  The head stages on the
          exported act3; the trunk is not held at 63 frames.
  act     n = 5 (the clamped waves of iqn_act_kernel), (W, A) = (1, 2), (32, 15), (8, 6): q_star
          bitwise forward(target)'s q at greedy, q_pi bitwise the float32 k-ordered sum / W of the
          online q at the action, greedy the first maximal index of that mean; scalar and per-frame
          eps; eps = 1 over 8 counters never greedy
  ties    q.q.weight = 0 and q.q.bias = b with dyadic b, so adv = b exactly in both dtypes and
          equal b give bitwise-equal means: b = 0 at A = 15 -> greedy 0; the maximum at two later
          indices -> the first; the maximum at A - 1 with eps = 1 -> the fallback branch, never
          greedy; A = 2 -> always the other action
"""
import math

import numpy as np
import pytest
import torch

import iqn_oracle as orc
import stage_checks as sc
from oracle import ref_stages as rs

pytestmark = pytest.mark.gpu
_ids = lambda s: "_".join(str(v) for v in s[1:])  # noqa: E731
ACT_N = 5
ACT_SHAPES = [(1, 2), (32, 15), (8, 6)]
# frames of the one handle of an (A, W): the most any case runs on it
BATCH = {(2, 1): ACT_N, (6, 8): ACT_N, (15, 5): 2, (15, 32): 5, (6, 31): 63}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _make(A, W, dtype, batch, online, target):
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    with torch.random.fork_rng(devices=[]):
        m = DistributionalAtariDQN((3, 64, 64), A, W, device=_dev(), dtype=dtype, seed=0)
    m.load_flat(online, target)
    e = IqnEngine(m, batch_size=batch)
    m._train_engine = e
    return m, e


_ENGINES = {}


def _engine(A, W, dtype):
    if (A, W, dtype) not in _ENGINES:
        _ENGINES[(A, W, dtype)] = _make(A, W, dtype, BATCH[(A, W)], *sc.iqn_flats(A))
    return _ENGINES[(A, W, dtype)][1]


def _forward(shape, dtype):
    """One forward of a case and its exports -> (exports, mask1, q [R,A], label)."""
    _, n, W, A, target = shape
    e = _engine(A, W, dtype)
    dev = _dev()
    _, (obs, taus) = sc.inputs(shape)
    q, used = e.forward(_t(obs, dev), target=target, taus=_t(taus, dev))
    assert np.array_equal(used.cpu().numpy(), taus)
    trunk = shape[:4] != sc.IQN_LARGE[:4]
    names = rs.IQN_FORWARD_TENSORS if trunk else ("act3",) + rs.IQN_HEAD_TENSORS
    got = {k: e.debug_tensor(k, frames=n) for k in names}
    mask1 = e.debug_tensor("mask1", frames=n) if trunk else None
    assert got["y"].shape == (n * W, 1024) and got["heads"].shape == (n * W, 16)
    label = f"{dtype} iqn n={n} W={W} A={A} {'target' if target else 'online'}"
    return got, mask1, q.cpu().numpy().reshape(n * W, A), label


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", sc.IQN_CASES, ids=_ids)
def test_iqn_forward_stages(shape, dtype):
    got, mask1, q, label = _forward(shape, dtype)
    bad = sc.hold_iqn_forward(shape, got, mask1, q, dtype == "bf16", label)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_iqn_forward_stages_over_stale_rows(dtype):
    """n = 1 after n = 5 on one handle: every stage holds, and the rows past R = 32 of y, zg, h
    and heads are the larger forward's, bit for bit (the stores of every kernel are masked)."""
    first, second = sc.IQN_STALE
    _forward(first, dtype)
    e = _engine(first[3], first[2], dtype)
    before = {k: e.debug_tensor(k, frames=first[1]) for k in rs.IQN_HEAD_TENSORS}
    got, mask1, q, label = _forward(second, dtype)
    R = second[1] * second[2]
    bad = []
    for k, v in before.items():
        after = e.debug_tensor(k, frames=first[1])
        assert np.any(v[R:] != 0), k  # (the premise: stale rows sit there)
        if not np.array_equal(after[R:], v[R:]):
            bad.append(f"{k}: rows >= R changed")
        if not np.array_equal(after[:R], got[k]):
            bad.append(f"{k}: two exports of the first R rows differ")
    bad += sc.hold_iqn_forward(second, got, mask1, q, dtype == "bf16", label + " (stale rows behind)")
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_iqn_forward_stages_past_the_fc_grid_cap(dtype):
    shape = sc.IQN_LARGE
    _dev()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    R = shape[1] * shape[2]
    t32, t16 = math.ceil(R / 80) * 32, math.ceil(R / 32) * 16
    print(f"{cu} CUs: the FC's grid cap {3 * cu} tiles; R = {R}: {t32} tiles in fp32, {t16} in bf16")
    assert R == 16 * 122 + 1 and R % 80 and R % 32
    assert t32 > 3 * cu and t16 > 3 * cu
    got, mask1, q, label = _forward(shape, dtype)
    bad = sc.hold_iqn_forward(shape, got, mask1, q, dtype == "bf16", label)
    assert not bad, bad


# ---------------------------------------------------------------- act
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _act(e, obs, eps, counter, t_on, t_tg):
    return [x.cpu().numpy() for x in e.act(obs, eps, seed=20, counter=counter, taus_online=t_on,
                                           taus_target=t_tg)]


def _hold_act(out, parts, label):
    """One iqn_act's outputs against the float32 restatement on the kernel's own q."""
    act, q_pi, q_star, g = out
    n, A = parts["qbar"].shape
    bad = []
    if not np.array_equal(g, parts["greedy"]):
        bad.append(f"{label}: greedy {g.tolist()} != first maximal index {parts['greedy'].tolist()}")
    if act.min() < 0 or act.max() >= A:
        bad.append(f"{label}: action outside [0, A): {act.tolist()}")
    elif not np.array_equal(_bits(q_pi), _bits(parts["qbar"][np.arange(n), act])):
        bad.append(f"{label}: q_pi is not the k-ordered float32 mean at the action")
    if not np.array_equal(_bits(q_star), _bits(parts["q_star"])):
        bad.append(f"{label}: q_star is not the target forward's q at greedy")
    return bad


def _own_q(e, obs, t_on, t_tg):
    """The two forwards iqn_act runs, on their own -> act_parts in float32."""
    q_on = e.forward(obs, taus=t_on)[0].cpu().numpy()
    q_tg = e.forward(obs, target=True, taus=t_tg)[0].cpu().numpy()
    assert q_on.dtype == np.float32 and np.isfinite(q_on).all() and np.isfinite(q_tg).all()
    parts = orc.act_parts(q_on, q_tg)
    assert parts["qbar"].dtype == np.float32
    return parts


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("W,A", ACT_SHAPES)
def test_iqn_act_on_its_own_forwards(W, A, dtype):
    dev, n = _dev(), ACT_N
    e = _engine(A, W, dtype)
    obs = _t(orc.fixture_obs(100 + n, n), dev)
    t_on, t_tg = _t(orc.edge_taus(n, W, seed=41), dev), _t(orc.edge_taus(n, W, seed=42), dev)
    parts = _own_q(e, obs, t_on, t_tg)
    g = parts["greedy"]
    print(f"{dtype} act W={W} A={A}: greedy {g.tolist()}, top-two gap of the mean "
          f"{orc.top2_gap(parts['qbar']).tolist()}")
    out = _act(e, obs, 0.0, 1, t_on, t_tg)
    bad = _hold_act(out, parts, "eps 0")
    if not np.array_equal(out[0], g):
        bad.append(f"eps 0: action {out[0].tolist()} is not greedy")
    # the per-frame eps vector: even frames greedy, odd frames never
    out = _act(e, obs, torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0]), 2, t_on, t_tg)
    bad += _hold_act(out, parts, "eps per frame")
    if not (np.array_equal(out[0][0::2], g[0::2]) and not np.any(out[0][1::2] == g[1::2])):
        bad.append(f"eps per frame: actions {out[0].tolist()} against greedy {g.tolist()}")
    seen = set()
    for c in range(8):  # eps = 1: never the greedy action
        out = _act(e, obs, 1.0, 10 + c, t_on, t_tg)
        bad += _hold_act(out, parts, f"eps 1 counter {10 + c}")
        if np.any(out[0] == g):
            bad.append(f"eps 1 counter {10 + c}: a greedy action in {out[0].tolist()}")
        if A == 2 and not np.array_equal(out[0], 1 - g):
            bad.append(f"eps 1 counter {10 + c}: A = 2 and not the other action")
        seen.update(out[0].tolist())
    print(f"{dtype} act W={W} A={A}: actions drawn at eps 1 over 8 counters {sorted(seen)}")
    assert not bad, bad


def _crafted(A, b):
    """The case's two nets with q.q.weight = 0 and q.q.bias = b (float32, dyadic)."""
    from impala_amd.iqn import net_specs
    off, at = 0, {}
    for k, s in net_specs(A):
        at[k] = (off, int(np.prod(s)))
        off += at[k][1]
    flats = []
    for flat in sc.iqn_flats(A):
        flat = flat.copy()
        o, k = at["q.q.weight"]
        flat[o:o + k] = 0
        o, k = at["q.q.bias"]
        flat[o:o + k] = np.asarray(b, np.float32)
        flats.append(flat)
    return flats


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_iqn_act_exact_ties_and_the_fallback_branch(dtype):
    dev, n, W = _dev(), ACT_N, 8
    obs = _t(orc.fixture_obs(100 + n, n), dev)
    t_on, t_tg = _t(orc.edge_taus(n, W, seed=41), dev), _t(orc.edge_taus(n, W, seed=42), dev)
    two = np.zeros(15, np.float32)
    two[[4, 9]] = 0.5
    last = np.zeros(15, np.float32)
    last[14] = 0.5
    bad = []
    for A, b, want, name in ((15, np.zeros(15, np.float32), 0, "b = 0"), (15, two, 4, "max at 4 and 9"),
                             (15, last, 14, "max at A - 1"),
                             (2, np.array([0, 0.5], np.float32), 1, "A = 2, max at 1"),
                             (2, np.zeros(2, np.float32), 0, "A = 2, b = 0")):
        m, e = _make(A, W, dtype, n, *_crafted(A, b))
        parts = _own_q(e, obs, t_on, t_tg)
        qb = _bits(parts["qbar"])
        # the premise: adv = b exactly, so equal b give bitwise-equal means and a larger b a larger one
        for k in range(A):
            same = np.nonzero(b == b[k])[0][0]
            assert np.array_equal(qb[:, k], qb[:, same]), (name, k)
        assert np.all(parts["qbar"][:, b == b.max()][:, :1] > parts["qbar"][:, b < b.max()]), name
        label = f"{dtype} {name}"
        out = _act(e, obs, 0.0, 1, t_on, t_tg)
        bad += _hold_act(out, parts, label)
        if not (np.all(out[3] == want) and np.all(out[0] == want)):
            bad.append(f"{label}: greedy {out[3].tolist()}, action {out[0].tolist()}, want {want}")
        seen = set()
        for c in range(8):
            out = _act(e, obs, 1.0, 30 + c, t_on, t_tg)
            bad += _hold_act(out, parts, f"{label} eps 1 counter {30 + c}")
            if np.any(out[0] == want) or not np.all(out[3] == want):
                bad.append(f"{label} eps 1 counter {30 + c}: actions {out[0].tolist()}, "
                           f"greedy {out[3].tolist()}")
            if A == 2 and not np.all(out[0] == 1 - want):
                bad.append(f"{label} eps 1 counter {30 + c}: not the other action")
            seen.update(out[0].tolist())
        print(f"{label}: greedy {want}; actions drawn at eps 1 over 8 counters {sorted(seen)}")
        e.close()
    assert not bad, bad
