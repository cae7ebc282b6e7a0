"""Every stage of the IQN training step's backward against float64 computed from that stage's own
exported inputs (teacher-forced, as tests/test_gpu_dqn_stages.py does for the dueling step), at
(N, W) = (3, 8) and (5, 32) in fp32 and bf16, with DESIGN.md §2's stage bounds (tests/stage_checks.py):
an fp32 tensor normwise 1e-5; a bf16 tensor within one bf16 ulp + 1e-5 (|r| + rms r) of the
reference at every element and at most 5e-3 of its elements off the reference's own rounding; a
gradient block 1e-4 rel-L2.

The tensors are the step's own (``IqnEngine.debug_tensor`` after ``compute_grads``); the weights a
kernel holds in the compute type enter the reference rounded as the library rounds them.  Stages:
  dz, the heads' blocks   from the exported heads (the loss's float64 gradient, rounded to the compute
                          type as the kernel stages it), zg and h
  dy, Wfc / bfc           from the exported dz and y
  dpre, dx, gamma / beta  from the exported dy, statistics, cosine tile and act3
  Wq / bq                 from the exported dpre and cosine tile
  dact3                   from the exported dx and act3
  dact2, conv3            from the exported dact3 and act2
  conv2, conv1            from the exported dact2, act1 and the frames; conv1's output gradient never
                          reaches HBM, so in bf16 d w1 is held as tests/stage_checks.py holds the
                          dueling step's: against the reference's own rounding of it, with the bound
                          that rounding's float32 / float64 hazard gives (w1_bound's rule)
"""
import types

import numpy as np
import pytest
import torch

import iqn_oracle as orc
import iqn_step_oracle as so
import stage_checks as sc
from oracle import ref_stages as rs

pytestmark = pytest.mark.gpu
CASES = [so.CASES[1], so.CASES[4]]  # (3, 8), (5, 32)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _canon(t):
    """[.., 1024] in the kernel order p*64 + c -> the canonical order c*16 + p."""
    t = np.asarray(t, np.float64)
    return t.reshape(t.shape[:-1] + (16, 64)).swapaxes(-1, -2).reshape(t.shape)


def _q(x, quant):
    x = torch.as_tensor(np.asarray(x, np.float64))
    return (rs.rne_bf16(x) if quant else x).numpy()


def _hold_t(name, got, ref, quant_out, label):
    g = np.asarray(got, np.float64).reshape(ref.shape)
    if quant_out:
        worst, share, wu = rs.bf16_figures(g, ref)
        print(f"{label} {name:6s} worst |d| / (ulp + 1e-5 (|r| + rms)) {worst:.3f}, share != RNE {share:.2e} "
              f"(worst {wu:.2f} ulp), rel-L2 {rs.rel_l2(g, ref):.2e}")
        return ([f"{name}: element bound x{worst:.3f}"] if worst > 1.0 else []) + \
               ([f"{name}: mismatch share {share:.2e}"] if share > sc.CAP else [])
    w = rs.f32_figures(g, ref)
    print(f"{label} {name:6s} normwise {w:.2e}, rel-L2 {rs.rel_l2(g, ref):.2e}")
    return [f"{name}: normwise {w:.2e}"] if w > sc.F32_NORMWISE else []


def _hold_b(name, got, ref, label):
    v = rs.rel_l2(got, ref)
    print(f"{label} block {name}: rel-L2 {v:.2e}")
    return [f"block {name}: rel-L2 {v:.2e}"] if not v <= sc.BLOCK_RL2 else []


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_iqn_step_stages_vs_float64(case, dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from impala_amd.iqn import DistributionalAtariDQN, IqnEngine
    dev = torch.device("cuda:0")
    N, W, A, _ = case
    R, quant, label = N * W, dtype == "bf16", f"{case} {dtype}"
    obs, act, taus, tgt, prob = so.batch(case)
    flat = so.flat0(A)
    m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
    m.load_flat(flat, flat)
    e = IqnEngine(m, batch_size=N, train=True)
    e.compute_grads(_t(obs, dev), _t(act, dev), _t(tgt, dev), _t(prob, dev), taus=_t(taus, dev))
    T = {k: np.asarray(e.debug_tensor(k), np.float64) for k in
         ("heads", "zg", "h", "y", "lnstat", "cos", "act3", "act2", "act1", "dz", "dy", "dpre", "dx", "dact3", "dact2")}
    sl = so.tensor_slices(A)
    g = m.flat_grad.cpu().numpy().astype(np.float64)
    P = {k: flat[s].astype(np.float64) for k, s in sl.items()}
    G = {k: g[s] for k, s in sl.items()}
    bad = []

    # ---- the head: dH from the exported heads, dz, the heads' blocks
    hd = T["heads"].reshape(N, W, 16)
    lh = orc.loss_from_heads(hd[:, :, :A], hd[:, :, 15], act, taus.astype(np.float64), tgt, prob,
                             kappa=so.OPT["kappa"], beta=so.OPT["beta"], dtype=torch.float64)
    dH = np.zeros((R, 16))
    dH[:, :A] = lh["dadv"].reshape(R, A)
    dH[:, 15] = lh["dv"].reshape(R)
    dH = _q(dH, quant)  # the kernel stages dH in the compute type
    wh = np.zeros((16, 512))
    wh[:A] = _q(P["q.q.weight"].reshape(A, 512), quant)
    wh[15] = _q(P["q.v.weight"], quant)
    bad += _hold_t("dz", T["dz"], (dH @ wh) * T["zg"], quant, label)
    dwh = dH.T @ T["h"]
    bad += _hold_b("q.q.weight", G["q.q.weight"], dwh[:A].reshape(-1), label)
    bad += _hold_b("q.v.weight", G["q.v.weight"], dwh[15], label)
    bad += _hold_b("q.q.bias", G["q.q.bias"], dH[:, :A].sum(0), label)
    bad += _hold_b("q.v.bias", G["q.v.bias"], dH[:, 15:].sum(0), label)

    # ---- the projection: dy, Wfc / bfc (canonical columns c*16 + p)
    wfc = _q(P["q.project.1.weight"].reshape(512, 1024), quant)
    bad += _hold_t("dy", _canon(T["dy"]), T["dz"] @ wfc, False, label)
    bad += _hold_b("q.project.1.weight", G["q.project.1.weight"], (T["dz"].T @ _canon(T["y"])).reshape(-1), label)
    bad += _hold_b("q.project.1.bias", G["q.project.1.bias"], T["dz"].sum(0), label)

    # ---- LayerNorm and modulation: dpre, dx, gamma / beta
    wq = _q(P["q.quantile_layer.output_layer.0.weight"].reshape(1024, 64), quant)
    pre = torch.as_tensor(T["cos"] @ wq.T + P["q.quantile_layer.output_layer.0.bias"])
    phi = (0.5 * pre * (1 + torch.erf(pre / np.sqrt(2.0)))).numpy()
    gp = (0.5 * (1 + torch.erf(pre / np.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / np.sqrt(2 * np.pi)).numpy()
    x = np.repeat(_canon(T["act3"]), W, axis=0)
    mean, rstd = T["lnstat"][:, :1], T["lnstat"][:, 1:]
    xh = (x * phi - mean) * rstd
    dy = _canon(T["dy"])
    gg = dy * P["q.project.0.weight"]
    dm = rstd * (gg - gg.mean(1, keepdims=True) - xh * (gg * xh).mean(1, keepdims=True))
    bad += _hold_t("dpre", _canon(T["dpre"]), dm * x * gp, quant, label)
    dx = (dm * phi).reshape(N, W, 1024).sum(1) * (_canon(T["act3"]) > 0)
    bad += _hold_t("dx", _canon(T["dx"]), dx, False, label)
    bad += _hold_b("q.project.0.weight", G["q.project.0.weight"], (dy * xh).sum(0), label)
    bad += _hold_b("q.project.0.bias", G["q.project.0.bias"], dy.sum(0), label)

    # ---- the quantile layer: Wq / bq from the exported dpre
    dpre = _canon(T["dpre"])
    bad += _hold_b("Wq", G["q.quantile_layer.output_layer.0.weight"], (dpre.T @ T["cos"]).reshape(-1), label)
    bad += _hold_b("bq", G["q.quantile_layer.output_layer.0.bias"], dpre.sum(0), label)

    # ---- the trunk, with the dueling step's own stage references (oracle/ref_stages.py): dact3 from
    # dx; dact2 and conv3's blocks from the exported dact3 and act2; conv2's blocks from the exported
    # dact2 and act1; conv1's from dY1 = [act1 > 0] col2im(dact2 w2), which never reaches HBM: d b1
    # sums it unrounded, d w1 reads it rounded to the compute type.
    bad += _hold_t("dact3", T["dact3"], T["dx"] * (T["act3"] > 0), quant, label)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))

    def weights(dt):
        cast = lambda k, shape: torch.as_tensor(_q(P[k], quant)).reshape(shape).to(dt)
        return types.SimpleNamespace(w1=cast("body.body.0.weight", (32, 3, 8, 8)),
                                     w2=cast("body.body.2.weight", (64, 32, 4, 4)),
                                     w3=cast("body.body.4.weight", (64, 64, 3, 3)))
    Wt = weights(torch.float64)
    dact2, dw3, db3 = rs.conv3_bwd(tt(T["dact3"]), tt(T["act2"]), Wt)
    bad += _hold_t("dact2", T["dact2"], dact2.numpy(), quant, label)
    bad += _hold_b("body.4.weight", G["body.body.4.weight"], dw3.numpy().reshape(-1), label)
    bad += _hold_b("body.4.bias", G["body.body.4.bias"], db3.numpy(), label)
    dY1, dw2, db2 = rs.conv2_bwd(tt(T["dact2"]), tt(T["act1"]), Wt)
    bad += _hold_b("body.2.weight", G["body.body.2.weight"], dw2.numpy().reshape(-1), label)
    bad += _hold_b("body.2.bias", G["body.body.2.bias"], db2.numpy(), label)
    frames = torch.from_numpy(np.ascontiguousarray(obs))
    dw1, db1 = rs.conv1_bwd(dY1, torch.as_tensor(_q(dY1.numpy(), quant)), frames, Wt)
    # d w1's bound where dY1 is rounded (stage_checks.w1_bound's rule): an element of dY1 that the
    # kernel's fp32 accumulation puts on the other side of a bf16 rounding boundary moves d w1 by a
    # whole bf16 ulp of it; 4 x the distance between the reference fed a float32-accumulated q(dY1)
    # and fed the float64-accumulated one, on this stage's own inputs; never below the block bound
    w1_bound = sc.BLOCK_RL2
    if quant:
        W32 = weights(torch.float32)
        dY1_32 = rs.conv2_bwd(tt(T["dact2"]).float(), tt(T["act1"]).float(), W32)[0]
        dw1_32 = rs.conv1_bwd(dY1, rs.rne_bf16(dY1_32).double(), frames, Wt)[0]
        own = rs.rel_l2(dw1_32.numpy(), dw1.numpy())
        w1_bound = max(sc.BLOCK_RL2, 4 * own)
        print(f"{label} block body.0.weight: the reference's own float32 / float64 distance {own:.2e}, bound {w1_bound:.2e}")
    v = rs.rel_l2(G["body.body.0.weight"], dw1.numpy().reshape(-1))
    print(f"{label} block body.0.weight: rel-L2 {v:.2e}")
    if not v <= w1_bound:
        bad.append(f"block body.0.weight: rel-L2 {v:.2e} > {w1_bound:.2e}")
    bad += _hold_b("body.0.bias", G["body.body.0.bias"], db1.numpy(), label)
    assert not bad, bad
