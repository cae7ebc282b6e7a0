"""The float64 stage references (oracle/ref_stages.py) and the bounds of tests/stage_checks.py,
checked on the CPU before tests/test_gpu_stages.py holds the kernels to them.

  chain identity  with every rounding off, the stage functions chained reproduce
                  ref_cpu.train_step_fp64's pre-clip gradient and metrics to 1e-10 relative:
                  the stage references are the network.
  cap check       the torch-float32 evaluation of every stage (the CPU stand-in of the kernels),
                  teacher-forced against float64 at every shape of the GPU test, holds every
                  bound of the GPU test, with the share of elements that round the other way at
                  most a quarter of the GPU test's cap.
  sensitivity     five defects a kernel could have, applied to the stand-in, each break the check
                  of their stage: the bounds bite.

The same three for the Ape-X DQN step (algo="dqn", tests/test_gpu_dqn_stages.py): the chain
against tests/dqn_oracle.train_step at A = 15 and A = 1, the stand-in at every GPU case in bf16
and fp32 (with no undecided rounding of dH at the chosen seeds), six defects of the dueling head
and the 512-wide FC, and the search over undecided roundings of dH.

And for the IQN actor path's forward (algo="iqn", tests/test_gpu_iqn_stages.py): the chain against
tests/iqn_oracle.make_net in float64 at every small case, the conditions on the taus' seeds (no
undecided rounding of the bf16 cosine tile at the small cases, at most 1 % of the rows at the
large one), the stand-in at every case, seven defects, and the row-by-row search over undecided
roundings of the cosine tile.
"""
import numpy as np
import pytest
import torch

import stage_checks as sc
from oracle import ref_cpu
from oracle import ref_stages as rs

_ids = lambda s: "x".join(str(v) for v in s)  # noqa: E731


def test_rne_bf16_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30,
                      -3.0 - 2.0 ** -6, 0.0, 2.0 ** -130], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0, 2.0 ** -130],
                        dtype=torch.float64)
    want[4] = -3.0 - 2.0 ** -6  # ulp(3) = 2^-6: representable
    assert torch.equal(rs.rne_bf16(x), want)
    # float32 inputs agree with torch's own conversion, and with the float64 path
    y = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    assert torch.equal(rs.rne_bf16(y), y.bfloat16().float())
    assert torch.equal(rs.rne_bf16(y.double()).float(), y.bfloat16().float())
    assert np.array_equal(rs.ulp_bf16(np.array([1.0, -1.5, 2.0, 0.0, 0.75])),
                          [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -8])


def test_chain_of_stages_is_the_network():
    B, T = 2, 3
    batch = ref_cpu.synthetic_batch(B, T, sc.A, seed=1234)
    # every bias and the LayerNorm affine away from their initial 0 / 1, so that a stage that
    # dropped or permuted one could not pass
    flat = ref_cpu.flat_params(ref_cpu.make_model(0, sc.A)).astype(np.float64)
    flat += 0.02 * np.random.default_rng(3).standard_normal(flat.size)
    _, g, met = ref_cpu.train_step_fp64(flat, batch, sc.A)
    coef = min(1.0, 0.5 / (met["train/grad_norm"] + 1e-6))  # clip_grad_norm_'s factor
    want = rs.split_flat(np.asarray(g, np.float64) / coef, sc.A)
    out = rs.run(flat, batch, sc.A, quant=False)
    for k in rs.BLOCKS:
        assert rs.rel_l2(out["grads"][k], want[k]) <= 1e-10, k
    for k in sc.MET_NAMES:
        assert abs(out["met"][k] - met["train/" + k]) <= 1e-10 * abs(met["train/" + k]), k
    norm = np.sqrt(sum(float(np.sum(v * v)) for v in out["grads"].values()))
    assert abs(norm - met["train/grad_norm"]) <= 1e-10 * norm


def _check_stand_in(shape, quant):
    s, S = sc.stand_in(shape, quant)
    r = sc.reference(shape, S, quant, key="stand-in" if quant else None)
    label = f"stand-in {'bf16' if quant else 'fp32'} {_ids(shape)}"
    fwd = shape == ("fwd",)
    names = rs.FORWARD_TENSORS if fwd else \
        ("dz",) if shape == ("ppo",) else rs.T_TENSORS + rs.F32_TENSORS
    bad = sc.hold_tensors(S, r, names, quant, label, cap=sc.STAND_IN_CAP)
    bad += sc.hold_mask(s["mask1"], S["act1"], label)
    if not fwd:
        ppo = shape == ("ppo",)
        bounds = {} if ppo else {"w1": sc.w1_bound(shape)[0]}
        if not ppo and quant:
            print(f"{label} w1: reference fed float32- vs float64-accumulated q(dY1) "
                  f"{sc.w1_bound(shape)[1]:.2e} -> bound {bounds['w1']:.1e}")
        bad += sc.hold_blocks(s["grads"], r, label, bounds,
                              ("wa", "ba", "wc", "bc") if ppo else rs.BLOCKS)
        if not ppo:
            bad += sc.hold_metrics([s["met"][k] for k in sc.MET_NAMES], r, label)
    assert not bad, bad


@pytest.mark.parametrize("shape", sc.STEP_SHAPES + [("fwd",), ("ppo",)], ids=_ids)
def test_float32_stand_in_holds_the_bounds_with_a_quarter_of_the_cap(shape):
    _check_stand_in(shape, True)


@pytest.mark.parametrize("shape", [(2, 3), (8, 20)], ids=_ids)
def test_float32_stand_in_without_rounding_holds_the_fp32_bounds(shape):
    _check_stand_in(shape, False)


SENS = (3, 7)


def _sens():
    flat0, batch = sc.inputs(SENS)
    s, S = sc.stand_in(SENS)
    r = sc.reference(SENS, S, True, key="stand-in")
    W = rs.Weights(flat0, sc.A, True, torch.float32)
    t = {k: torch.from_numpy(v).float() for k, v in S.items()}
    return s, S, r, W, t


def _fails_tensor(name, value, r):
    """a defective float32 evaluation of a bf16 tensor, rounded as the kernel would"""
    got = {name: rs.rne_bf16(value.float()).double().numpy()}
    return bool(sc.hold_tensors(got, r, (name,), True, f"defect {name}"))


def test_defect_weight_gradient_skips_the_last_64_rows():
    _, _, r, W, t = _sens()
    d3 = t["dact3"].clone()
    d3[-4:] = 0  # conv3's rows are (frame, pixel): 64 rows = 4 frames
    _, w3, _ = rs.conv3_bwd(d3, t["act2"], W)
    assert sc.hold_blocks({"w3": w3.double().numpy()}, r, "defect", names=("w3",))
    _, w3, _ = rs.conv3_bwd(t["dact3"], t["act2"], W)  # (and the sound one passes)
    assert not sc.hold_blocks({"w3": w3.double().numpy()}, r, "sound", names=("w3",))


def test_defect_weight_gradient_counts_one_frame_twice():
    _, _, r, W, t = _sens()
    d2 = torch.cat([t["dact2"], t["dact2"][5:6]])
    a1 = torch.cat([t["act1"], t["act1"][5:6]])
    _, w2, b2 = rs.conv2_bwd(d2, a1, W)
    bad = sc.hold_blocks({"w2": w2.double().numpy(), "b2": b2.double().numpy()}, r, "defect",
                         names=("w2", "b2"))
    assert len(bad) == 2, bad


def test_defect_dgrad_with_one_tap_shifted():
    _, _, r, W, t = _sens()
    w3 = W.w3.clone()
    w3[:, :, 0, 0], w3[:, :, 0, 1] = W.w3[:, :, 0, 1], W.w3[:, :, 0, 0]
    dact2, _, _ = rs.conv3_bwd(t["dact3"], t["act2"], W, w3=w3)
    assert _fails_tensor("dact2", dact2, r)
    dact2, _, _ = rs.conv3_bwd(t["dact3"], t["act2"], W)
    assert not _fails_tensor("dact2", dact2, r)


def test_defect_layernorm_backward_from_y():
    _, _, r, W, t = _sens()
    xh = (t["y"] - W.lnb) / W.lng  # the rounded y instead of (act3 - mean) * rstd
    dact3, lng, _ = rs.ln_bwd(t["dy"], t["act3"], t["lnstat"], W, xh=xh)
    assert _fails_tensor("dact3", dact3, r)
    dact3, _, _ = rs.ln_bwd(t["dy"], t["act3"], t["lnstat"], W)
    assert not _fails_tensor("dact3", dact3, r)


def test_defect_head_gradient_left_unrounded():
    s, _, r, W, t = _sens()
    dH = torch.from_numpy(s["t"]["dH"]).float()
    dz, _, _ = rs.head_bwd(dH, t["zg"], t["h"], W)  # no rounding of dH
    assert _fails_tensor("dz", dz, r)
    dz, _, _ = rs.head_bwd(rs.rne_bf16(dH), t["zg"], t["h"], W)
    assert not _fails_tensor("dz", dz, r)


# ------------------------------------------------------------------------------ Ape-X DQN
@pytest.mark.parametrize("A", [15, 1])
def test_dqn_chain_of_stages_is_the_dueling_net(A):
    """Rounding off, run(algo="dqn") is tests/dqn_oracle.train_step in float64: the pre-clip
    gradient, the metrics and the priorities to 1e-10, every bias and the LayerNorm affine away
    from 0 / 1, at A = 15 and at A = 1 (where the advantage head's gradient is exactly zero)."""
    import dqn_oracle as orc
    N = 5
    obs, act, tgt, p = orc.synthetic_batch(N, A, seed=7, probs=True)
    flat = sc._dqn_flat(A)[0].astype(np.float64)
    flat += 0.02 * np.random.default_rng(3).standard_normal(flat.size)
    beta = float(np.float32(sc.DQN_BETA))  # the exponent as the kernel holds it
    net = orc.make_net(flat, A, dtype=torch.float64)
    exp = orc.train_step(net, orc.make_optimizer(net), obs, act, tgt.astype(np.float64),
                         p.astype(np.float64), beta=beta, max_grad_norm=1e30)  # (no clip)
    want = rs.split_flat(exp["grads"], A, "dqn")
    out = rs.run(flat, (obs, act, tgt, p), A, quant=False, algo="dqn", beta=sc.DQN_BETA)
    for k in rs.BLOCKS:
        if A == 1 and k == "wa" or A == 1 and k == "ba":
            assert not np.any(want[k]) and not np.any(out["grads"][k]), k
        else:
            assert rs.rel_l2(out["grads"][k], want[k]) <= 1e-10, k
    for k in sc.DQN_MET_NAMES:
        assert abs(out["met"][k] - exp[k]) <= 1e-10 * abs(exp[k]), k
    assert np.max(np.abs(out["prio"] - exp["prio"])) <= 1e-10 * np.max(exp["prio"])
    norm = np.sqrt(sum(float(np.sum(v * v)) for v in out["grads"].values()))
    assert abs(norm - exp["grad_norm"]) <= 1e-10 * norm


def _check_dqn_stand_in(shape, quant):
    s, S = sc.stand_in(shape, quant)
    _, batch = sc.inputs(shape)
    r = sc.reference(shape, S, quant, key="stand-in" if quant else None)
    label = f"stand-in {'bf16' if quant else 'fp32'} dqn N={shape[1]} A={shape[2]}"
    head = shape == sc.DQN_HEAD
    if quant:
        und = sc.dqn_undecided(r["t"]["dH"], batch[1], shape[2])
        assert not und, f"the seed of {shape} leaves undecided roundings of dH: {und}"
    r, bad = sc.dqn_resolve_head(shape, S, s["grads"], r, quant, label)
    bad += sc.hold_tensors(S, r, ("dz",) if head else sc.DQN_STEP_TENSORS, quant, label,
                           cap=sc.STAND_IN_CAP)
    bounds = {}
    if not head:
        bad += sc.hold_mask(s["mask1"], S["act1"], label)
        if quant:
            bounds = {"w1": sc.w1_bound(shape)[0]}
            print(f"{label} w1: reference fed float32- vs float64-accumulated q(dY1) "
                  f"{sc.w1_bound(shape)[1]:.2e} -> bound {bounds['w1']:.1e}")
    bad += sc.hold_blocks(s["grads"], r, label, bounds, sc.DQN_HEAD_BLOCKS if head else rs.BLOCKS)
    bad += sc.hold_dqn_prio(S["prio"], r, batch, label)
    bad += sc.hold_dqn_metrics([s["met"][k] for k in sc.DQN_MET_NAMES], r, label)
    assert not bad, bad


_dqn_ids = lambda s: "_".join(str(v) for v in s[1:])  # noqa: E731


@pytest.mark.parametrize("quant", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", sc.DQN_CASES + [sc.DQN_HEAD], ids=_dqn_ids)
def test_dqn_float32_stand_in_holds_the_bounds_with_a_quarter_of_the_cap(shape, quant):
    _check_dqn_stand_in(shape, quant)


@pytest.mark.parametrize("quant", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", sc.DQN_FWD_CASES, ids=_dqn_ids)
def test_dqn_forward_stand_in_holds_the_bounds_with_a_quarter_of_the_cap(shape, quant):
    s, S = sc.stand_in(shape, quant)
    r = sc.reference(shape, S, quant)
    label = f"stand-in {'bf16' if quant else 'fp32'} dqn forward n={shape[1]} target={shape[2]}"
    bad = sc.hold_tensors(S, r, rs.FORWARD_TENSORS, quant, label, cap=sc.STAND_IN_CAP)
    bad += sc.hold_mask(s["mask1"], S["act1"], label)
    assert not bad, bad


def _dqn_sens(shape):
    flat0, batch = sc.inputs(shape)
    s, S = sc.stand_in(shape)
    r = sc.reference(shape, S, True, key="stand-in")
    W = rs.Weights(flat0, shape[2], True, torch.float32, 512, "dqn")
    t = {k: torch.from_numpy(np.asarray(v)).float() for k, v in S.items()}
    return s, S, r, W, t, batch


def _dqn_head_defect(shape, **defect):
    """The stand-in's head stage with a defect -> (violations of the priorities / metrics checks,
    violations of dz's check)."""
    s, S, r, W, t, batch = _dqn_sens(shape)
    dH, met, x = rs.dqn_head(t["h"], batch, shape[2], W, sc.DQN_BETA, torch.float32, **defect)
    dz, _, _ = rs.head_bwd(rs.rne_bf16(dH), t["zg"], t["h"], W)
    loss = sc.hold_dqn_prio(x["prio"], r, batch, "defect") + \
        sc.hold_dqn_metrics([met[k] for k in sc.DQN_MET_NAMES], r, "defect")
    return loss, _fails_tensor("dz", dz, r)


def test_dqn_defect_mean_over_15_rows_instead_of_A():
    shape = ("dqn", 32, 6, True)
    loss, dz = _dqn_head_defect(shape, mean_rows=15)
    assert any(m.startswith("priorities") for m in loss) and any("metric q" in m for m in loss), loss
    assert dz
    assert _dqn_head_defect(shape) == ([], False)  # (and the sound one passes)


def test_dqn_defect_weights_normalised_by_max_p():
    shape = ("dqn", 33, 15, True)
    loss, dz = _dqn_head_defect(shape, pnorm=float(sc.inputs(shape)[1][3].max()))
    assert any("metric loss" in m for m in loss) and dz, loss


def test_dqn_defect_pmin_over_the_first_1024_probabilities():
    shape = sc.DQN_HEAD
    p = sc.inputs(shape)[1][3]
    assert int(np.argmin(p)) == 1029
    loss, dz = _dqn_head_defect(shape, pnorm=float(p[:1024].min()))
    assert any("metric loss" in m for m in loss) and dz, loss
    assert _dqn_head_defect(shape) == ([], False)


def test_dqn_defect_row_after_a_ragged_blocks_last_transition_counted():
    shape = ("dqn", 33, 15, True)  # the second block of 32 holds transition 32 alone
    s, _, r, W, t, _ = _dqn_sens(shape)
    qdH = rs.rne_bf16(torch.from_numpy(s["t"]["dH"]).float())
    _, wh, bh = rs.head_bwd(qdH, t["zg"], t["h"], W)
    g = rs._head_grads({"wh": wh, "bh": bh}, 15)
    assert not sc.hold_blocks(g, r, "sound", names=sc.DQN_HEAD_BLOCKS)
    wh = wh + torch.outer(qdH[32], t["h"][32])  # row 33 of the tile: a copy of the last one
    g = rs._head_grads({"wh": wh, "bh": bh}, 15)
    bad = sc.hold_blocks(g, r, "defect", names=("wa", "wc"))
    assert len(bad) == 2, bad


def test_dqn_defect_dz_of_slice_s_times_zg_of_slice_0():
    shape = ("dqn", 33, 15, True)
    s, _, r, W, t, _ = _dqn_sens(shape)
    qdH = rs.rne_bf16(torch.from_numpy(s["t"]["dH"]).float())
    zg = t["zg"][:, :64].repeat(1, 8)  # every 64-column slice reads slice 0's gelu'
    dz, _, _ = rs.head_bwd(qdH, zg, t["h"], W)
    assert _fails_tensor("dz", dz, r)
    dz, _, _ = rs.head_bwd(qdH, t["zg"], t["h"], W)
    assert not _fails_tensor("dz", dz, r)


def test_dqn_defect_bfc_summed_over_the_first_256_columns():
    shape = ("dqn", 33, 15, True)
    _, _, r, W, t, _ = _dqn_sens(shape)
    _, _, bfc = rs.fc_bwd(t["dz"], t["y"], W)
    assert not sc.hold_blocks({"bfc": bfc.double().numpy()}, r, "sound", names=("bfc",))
    bfc[256:] = 0
    assert sc.hold_blocks({"bfc": bfc.double().numpy()}, r, "defect", names=("bfc",))


def test_dqn_undecided_rounding_of_dH_is_resolved_not_tolerated(monkeypatch):
    """A kernel whose fp32 dH rounded the other way at an undecided element: the reference's own
    rounding fails the head blocks at N = 1 (the bounds see it), the assignment search finds the
    kernel's rounding and everything holds under it -- and with more than MAX_UNDECIDED
    undecided decisions the case fails.  (The margin is widened to make elements undecided.)"""
    shape = ("dqn", 1, 15, True)
    s, S, r, W, t, batch = _dqn_sens(shape)
    monkeypatch.setattr(sc, "DQN_U", 2.0 ** -11)
    und, cands = sc.dqn_head_assignments(r["t"]["dH"], batch[1], 15)
    assert 1 <= len(und) <= 3 and len(cands) == 2 ** len(und)
    qdH = torch.from_numpy(cands[-1]).float()  # every undecided decision at its upper rounding
    assert not np.array_equal(cands[-1], cands[0])
    dz, wh, bh = rs.head_bwd(qdH, t["zg"], t["h"], W)
    got = dict(S, dz=rs.rne_bf16(dz).double().numpy())
    blocks = rs._head_grads({"wh": wh, "bh": bh}, 15)
    assert sc.hold_blocks(blocks, r, "other rounding, reference's own", names=sc.DQN_HEAD_BLOCKS)
    r2, bad = sc.dqn_resolve_head(shape, got, blocks, r, True, "other rounding")
    assert not bad
    assert not sc.hold_blocks(blocks, r2, "other rounding, resolved", names=sc.DQN_HEAD_BLOCKS)
    assert not sc.hold_tensors(got, r2, ("dz",), True, "other rounding, resolved")
    # a genuinely wrong dH is not rescued: no assignment holds, and the ordinary checks report it
    dz, wh, bh = rs.head_bwd(qdH * 1.01, t["zg"], t["h"], W)
    got = dict(S, dz=rs.rne_bf16(dz).double().numpy())
    blocks = rs._head_grads({"wh": wh, "bh": bh}, 15)
    r3, bad = sc.dqn_resolve_head(shape, got, blocks, r, True, "wrong dH")
    assert sc.hold_blocks(blocks, r3, "wrong dH", names=sc.DQN_HEAD_BLOCKS)
    # too many undecided decisions: the case fails
    shape = ("dqn", 33, 15, True)
    s, S, r, W, t, batch = _dqn_sens(shape)
    _, bad = sc.dqn_resolve_head(shape, S, s["grads"], r, True, "wide margin")
    assert bad and "undecided" in bad[0], bad


# ------------------------------------------------------------------------------ IQN forward
_iqn_ids = lambda s: "_".join(str(v) for v in s[1:])  # noqa: E731
IQN_ALL = sc.IQN_CASES + [sc.IQN_LARGE]


@pytest.mark.parametrize("shape", sc.IQN_CASES, ids=_iqn_ids)
def test_iqn_chain_of_stages_is_the_quantile_net(shape):
    """Rounding off, run(algo="iqn") in float64 is tests/iqn_oracle.make_net(..., float64) to
    1e-10 at every small case and both nets, with the cosine's argument formed in float32 in both
    (``arg32``: the oracle's own float64 run forms the last product in double, the kernel and the
    reference's float32 run do not).  The argument's rounding moves it by at most 2^-24 of up to
    64 pi = 201, i.e. 1.2e-5 absolute: q of the two oracles differs by that order, also checked."""
    import iqn_oracle as orc
    flat, (obs, taus) = sc.inputs(shape)
    A = shape[3]
    out = rs.run(flat.astype(np.float64), (obs, taus), A, quant=False, algo="iqn")
    net = orc.make_net(flat, A, torch.float64)
    with torch.no_grad():
        want = net(torch.from_numpy(obs), torch.from_numpy(taus), arg32=True).numpy().reshape(-1, A)
        f64 = net(torch.from_numpy(obs), torch.from_numpy(taus)).numpy().reshape(-1, A)
    err = np.max(np.abs(out["q"] - want)) / np.max(np.abs(want))
    d = np.max(np.abs(f64 - want)) / np.max(np.abs(want))
    print(f"{_iqn_ids(shape)} chain vs oracle (float32 argument) {err:.1e}; "
          f"oracle float64 vs float32 argument {d:.1e}")
    assert err <= 1e-10
    assert d <= 1e-4


def test_iqn_seeds_leave_no_undecided_cosine_at_the_small_cases_and_few_at_the_large():
    """On the reference alone: no element of the bf16 cosine tile is undecided at any small case;
    at the large case at most 1 % of the rows hold one (the GPU test allows 2 %) and no row more
    than IQN_MAX_UNDECIDED."""
    for shape in sc.IQN_CASES:
        _, _, und = sc.iqn_undecided_rows(shape)
        assert und.shape == (shape[1] * shape[2], rs.IQN_COS)
        assert not und.any(), (shape, np.argwhere(und))
    cnt = sc.iqn_undecided_rows(sc.IQN_LARGE)[2].sum(1)
    print(f"large case: {int((cnt > 0).sum())} of {len(cnt)} rows undecided, at most {int(cnt.max())} in a row")
    assert len(cnt) == 1953 and 0 < np.mean(cnt > 0) <= 0.01 < sc.IQN_LARGE_UNDECIDED
    assert cnt.max() <= sc.IQN_MAX_UNDECIDED


def test_iqn_edge_taus_hold_the_ends_of_the_interval():
    top = np.nextafter(np.float32(1), np.float32(0))
    for shape in IQN_ALL:
        t = sc.inputs(shape)[1][1].reshape(-1)
        assert t.dtype == np.float32 and t[0] == 0.0 and t.max() < 1.0
        assert len(t) == 1 or t[-1] == top
        assert len(t) <= 2 or t[len(t) // 2] == np.nextafter(top, np.float32(0))


def _iqn_stand_in_holds(shape, quant):
    s, S = sc.stand_in(shape, quant)
    label = f"stand-in {'bf16' if quant else 'fp32'} iqn {_iqn_ids(shape)}"
    q = rs.dueling_q(torch.from_numpy(S["heads"]).float(), shape[3]).numpy()
    return sc.hold_iqn_forward(shape, S, s["mask1"], q, quant, label, cap=sc.STAND_IN_CAP)


@pytest.mark.parametrize("quant", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", IQN_ALL, ids=_iqn_ids)
def test_iqn_float32_stand_in_holds_the_bounds_with_a_quarter_of_the_cap(shape, quant):
    bad = _iqn_stand_in_holds(shape, quant)
    assert not bad, bad


def _iqn_sens(shape):
    flat, (obs, taus) = sc.inputs(shape)
    s, S = sc.stand_in(shape)
    r = sc.reference(shape, S, True, key="stand-in")
    W = rs.IqnWeights(flat, shape[3], True, torch.float32)
    t = {k: torch.from_numpy(np.asarray(v)).float() for k, v in S.items()}
    e = rs.iqn_cos(taus.reshape(-1), torch.float32)
    return S, r, W, t, e, taus.shape[1]


IQN_SENS = ("iqn", 3, 8, 6, False)  # 16-row tiles spanning frames


@pytest.mark.parametrize("defect", ["first_frame", "tanh_gelu", "no_bq", "raw_second_moment"])
def test_iqn_defect_of_the_embed_stage(defect):
    """A tile's rows all reading its first row's frame; tanh-GELU for erf-GELU; bq dropped; the
    variance without the mean subtracted: each fails y's check, and the sound stage passes."""
    _, r, W, t, e, n_tau = _iqn_sens(IQN_SENS)
    assert _fails_tensor("y", rs.iqn_embed_ln(t["act3"], rs.rne_bf16(e), W, n_tau, defect), r)
    assert not _fails_tensor("y", rs.iqn_embed_ln(t["act3"], rs.rne_bf16(e), W, n_tau), r)


def test_iqn_defect_cosine_tile_left_unrounded():
    _, r, W, t, e, n_tau = _iqn_sens(IQN_SENS)
    assert not torch.equal(e, rs.rne_bf16(e))
    assert _fails_tensor("y", rs.iqn_embed_ln(t["act3"], e, W, n_tau), r)


def test_iqn_defect_q_mean_over_W_columns():
    S, _, _, t, _, n_tau = _iqn_sens(IQN_SENS)
    A = IQN_SENS[3]
    assert n_tau != A
    assert sc.hold_dqn_q(rs.dueling_q(t["heads"], A, mean_cols=n_tau).numpy(), S["heads"], A, "defect")
    assert not sc.hold_dqn_q(rs.dueling_q(t["heads"], A).numpy(), S["heads"], A, "sound")


@pytest.mark.parametrize("quant,rows", [(True, 1536), (False, 1920)], ids=["bf16", "fp32"])
def test_iqn_defect_fc_skips_the_row_tiles_past_its_capped_grid(quant, rows):
    """The FC's grid is capped at 3 x 256 CUs = 768 tiles; tile t is (feature tile t % n, row tile
    t / n), so its first pass covers 768 / 16 row tiles of 32 (bf16) or 768 / 32 of 80 (fp32).  A
    loop that stopped there would leave the rows behind unwritten (zero: the workspace starts
    zeroed): the large case reaches them, and h's and zg's checks fail."""
    shape = sc.IQN_LARGE
    s, S = sc.stand_in(shape, quant)
    r = sc.reference(shape, S, quant, key="stand-in" if quant else None)
    assert rows < shape[1] * shape[2]
    got = {k: S[k].copy() for k in ("h", "zg")}
    assert not sc.hold_tensors(got, r, ("h", "zg"), quant, "sound")
    for k in got:
        got[k][rows:] = 0
    bad = sc.hold_tensors(got, r, ("h", "zg"), quant, "defect")
    assert any(b.startswith("h:") for b in bad) and any(b.startswith("zg:") for b in bad), bad


def test_iqn_undecided_cosine_is_resolved_row_by_row_not_tolerated():
    """A kernel whose cosf rounded the other way at the undecided elements of the large case: the
    reference's own rounding fails y (the bounds see it), the row search finds the kernel's
    rounding and y holds under it; a row that is wrong (another frame's act3) is not rescued."""
    shape = sc.IQN_LARGE
    flat, (_, taus) = sc.inputs(shape)
    s, S = sc.stand_in(shape)
    r = sc.reference(shape, S, True, key="stand-in")
    lo, hi, und = sc.iqn_undecided_rows(shape)
    W = rs.IqnWeights(flat, shape[3], True, torch.float32)
    base = rs.rne_bf16(torch.from_numpy(r["e"])).numpy()
    other = np.where(und, np.where(base == lo, hi, lo), base)  # every undecided element flipped
    rows = np.nonzero(und.any(1))[0]
    act3 = torch.from_numpy(S["act3"]).float()
    y = rs.rne_bf16(rs.iqn_embed_ln(act3, torch.from_numpy(other).float(), W, taus.shape[1]))
    got = dict(S, y=y.double().numpy())
    assert sc.hold_tensors(got, r, ("y",), True, "other rounding, reference's own")
    r2, bad = sc.iqn_resolve_embed(shape, got, r, True, "other rounding")
    assert not bad and not sc.hold_tensors(got, r2, ("y",), True, "other rounding, resolved")
    changed = np.nonzero((r2["t"]["y"] != r["t"]["y"]).any(1))[0]
    assert set(changed) <= set(rows) and len(changed) >= len(rows) // 2
    f = int(rows[0]) // taus.shape[1]
    wrong = got["y"].copy()
    wrong[rows[0]] = rs.rne_bf16(rs.iqn_embed_ln_rows(
        act3[(f + 1) % shape[1]][None], torch.from_numpy(other[rows[0]]).float()[None], W)).numpy()[0]
    got = dict(S, y=wrong)
    r3, _ = sc.iqn_resolve_embed(shape, got, r, True, "wrong row")
    assert sc.hold_tensors(got, r3, ("y",), True, "wrong row")
