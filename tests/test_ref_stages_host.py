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
