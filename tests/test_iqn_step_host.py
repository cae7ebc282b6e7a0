"""CPU checks of the IQN training step's reference (tests/iqn_step_oracle.py) and of what the GPU
tests ask of the kernels:

* the reference's loss and its gradient with respect to the heads agree with
  ``iqn_oracle.loss_from_heads`` -- the restatement pinned to the reference's own fixture -- to 1e-10;
* a float32 evaluation of the reference stays within a quarter of each GPU bound at every test
  shape (were it not so, the bound would not be a float32 kernel's to meet);
* the test inputs hold the edge cases they are meant to.
"""
import numpy as np
import pytest
import torch

import iqn_oracle as orc
import iqn_step_oracle as so


@pytest.mark.parametrize("case", so.CASES[:5], ids=str)
def test_loss_and_head_gradients_match_the_pinned_loss_head(case):
    N, W, A, _ = case
    obs, act, taus, tgt, prob = so.batch(case)
    r = so.reference(case)
    with torch.no_grad():
        net = orc.make_net(so.flat0(A), A, torch.float64)
        adv, v = net.heads(torch.as_tensor(obs), torch.as_tensor(taus), arg32=True)
    want = orc.loss_from_heads(adv.numpy(), v.squeeze(-1).numpy(), act, taus.astype(np.float64), tgt, prob,
                               kappa=so.OPT["kappa"], beta=so.OPT["beta"], dtype=torch.float64)
    assert abs(r["met"]["loss"] - want["metrics"][3]) <= 1e-10 * max(1.0, abs(want["metrics"][3]))
    assert np.abs(r["dadv"] - want["dadv"]).max() <= 1e-10
    assert np.abs(r["dv"] - want["dv"]).max() <= 1e-10
    assert np.abs(r["prio"] - want["priorities"]).max() <= 1e-10
    for k, i in (("q", 0), ("target", 1), ("priorities", 2)):
        assert abs(r["met"][k] - want["metrics"][i]) <= 1e-10


def _quarter(case, got, ref, label):
    """Every figure of `got` against `ref` at a quarter of the GPU bounds; prints them."""
    A = case[2]
    bad = []
    for k in so.MET_NAMES:
        err, tol = abs(got["met"][k] - ref["met"][k]), 0.25 * (so.MET_ATOL + so.MET_RTOL * abs(ref["met"][k]))
        print(f"{label} {k}: {got['met'][k]:.9g} vs {ref['met'][k]:.9g}  err {err:.2e} (quarter bound {tol:.2e})")
        if err > tol:
            bad.append(k)
    err = np.abs(got["prio"] - ref["prio"])
    tol = 0.25 * (so.PRIO_ATOL + so.PRIO_RTOL * np.abs(ref["prio"]))
    print(f"{label} priorities: worst err / quarter bound {float((err / tol).max()):.3f}")
    if (err > tol).any():
        bad.append("prio")
    v = so.rel_l2(got["grad"], ref["grad"])
    print(f"{label} grad flat rel-L2 {v:.2e}")
    if v > 0.25 * so.GRAD_RL2:
        bad.append("grad")
    for name, sl in so.tensor_slices(A).items():
        v = so.rel_l2(got["grad"][sl], ref["grad"][sl])
        print(f"{label} grad {name} rel-L2 {v:.2e}")
        if v > 0.25 * so.GRAD_RL2:
            bad.append("grad " + name)
    v = float(np.abs(got["params"] - ref["params"]).max())
    print(f"{label} params max abs {v:.2e}")
    if v > 0.25 * so.PARAM_ABS:
        bad.append("params")
    return bad


@pytest.mark.parametrize("case", so.CASES, ids=str)
def test_float32_evaluation_within_a_quarter_of_the_gpu_bounds(case):
    bad = _quarter(case, so.reference(case, torch.float32), so.reference(case), f"{case}")
    assert not bad, bad


def test_float32_three_steps_within_a_quarter_of_the_gpu_bounds():
    r32, r64 = so.reference_steps(so.MULTI, 3, torch.float32), so.reference_steps(so.MULTI, 3)
    bad = [(i, b) for i in range(3) for b in _quarter(so.MULTI, r32[i], r64[i], f"step {i}")]
    assert not bad, bad


def test_inputs_hold_the_edge_cases():
    for case in so.CASES:
        N, W, A, probs = case
        obs, act, taus, tgt, prob = so.batch(case)
        assert obs.shape == (N, 3, 64, 64) and taus.shape == tgt.shape == (N, W)
        assert taus.reshape(-1)[0] == 0.0
        qa = so.reference(case)["qa"]
        if W > 1:
            assert abs(float(tgt[0, 0]) - qa[0, 0]) <= 2 * np.spacing(np.float32(abs(qa[0, 0])))
        if probs:
            assert prob.argmin() == N - 1  # the largest weight on the last frame
            d = np.abs(tgt.astype(np.float64) - qa[:, :1])
            assert (d > 1.0).any() and (d < 1.0).any()  # both Huber branches
    # the large case: more FC tiles than a persistent grid of 3 per CU on 256 CUs, in both dtypes
    # (fp32 16 x 80 tiles, bf16 32 x 32), and a ragged last split of 64-row chunks
    R = max(N * W for N, W, _, _ in so.CASES)
    assert -(-R // 80) * (512 // 16) > 768 and -(-R // 32) * (512 // 32) > 768 and R % 64
