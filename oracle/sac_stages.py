"""ORACLE -- test infrastructure only (never shipped, never on the product path).

The SAC learner step (oracle/sac_cpu.py; impala_amd/csrc/sac.h) as plain torch float64, one
function per launch of the per-layer path (``enqueue_step`` in csrc/sac.hip is the list), so each
kernel stage can be held to a reference evaluated on the tensors THAT stage read (teacher-forced:
``run(..., given=the device's own exports)``).

Rounding (``quant=True``, the bf16 mode): to bf16, ties to even, exactly where a kernel stores a
value of the compute type T (packed operands, kernel-layout weights, hidden activations, dh*, dq,
g_mean, g_u); to float32 where a later stage reads a stored float32 (save, logp*, q1, q2).
Everything else a kernel keeps in registers stays unrounded: the dQ that multiplies W3 is the
float, not the stored bf16; the policy-head backward uses the float g_mean / g_u; heads, W3, the
biases and the critic's action columns are read from the canonical float32 parameters.
``quant=False`` rounds nothing: the chain is then the autograd step of oracle/sac_cpu.py in
float64 (tests/test_sac_stages_host.py: 1e-10).

The step uses three parameter sets: the initial ones (critic phase), the critic after its Adam
step (actor phase), the actor after its Adam step (alpha phase).  ``dtype=torch.float32`` runs the
same chain in float32: the CPU stand-in of the device (as oracle/ref_stages.py's).

Logical tensors (``run(...)["t"]``, padding stripped; q = 0, 1 the two Q networks):
  T     xs xs1 [N,D]; xc xt xp [N,D+K]; hta1 hta2 ha1 ha2 hb1 hb2 hc1_q hc2_q htc1_q htc2_q hp1_q
        hp2_q [N,256]; dh2_q dhc1_q dhp2_q dhp1_q dha2 dha1 [N,256]; dq_q [N]; gm gu [N,K]
  fp32  q1 q2 logp1 logp logp2 prio [N]; save [4,N,K] (std, y, x - mean, tanh u); rowm [6,N]
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from oracle.ref_stages import rne_bf16

H = 256
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
A_BLOCKS = ("w1", "b1", "w2", "b2", "wm", "bm", "wl", "bl")
Q_BLOCKS = ("w1", "b1", "w2", "b2", "w3", "b3")
C_BLOCKS = tuple(f"q{q}.{k}" for q in (0, 1) for k in Q_BLOCKS)
HID = ("hta1", "hta2", "ha1", "ha2", "hb1", "hb2") + tuple(
    f"{n}_{q}" for n in ("hc1", "hc2", "htc1", "htc2", "hp1", "hp2") for q in (0, 1))
T_TENSORS = ("xs", "xs1", "xc", "xt", "xp") + HID + (
    "dh2_0", "dh2_1", "dq_0", "dq_1", "dhc1_0", "dhc1_1", "dhp2_0", "dhp2_1", "dhp1_0", "dhp1_1",
    "gm", "gu", "dha2", "dha1")
F32_TENSORS = ("q1", "q2", "logp1", "logp", "logp2", "save", "rowm", "prio")
DEFECTS = ("ones_row", "swap_head_row", "actor_min_q1", "wrong_n", "clip_off", "polyak_first",
           "w1_shift")


# ------------------------------------------------------------------------------ parameters
def actor_shapes(D: int, K: int):
    return [("w1", (H, D)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)), ("wm", (K, H)), ("bm", (K,)),
            ("wl", (K, H)), ("bl", (K,))]


def q_shapes(D: int, K: int):
    return [("w1", (H, D + K)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)), ("w3", (H,)), ("b3", ())]


def _split(flat, shapes, dtype):
    out, off = {}, 0
    for n, s in shapes:
        k = int(np.prod(s)) if len(s) else 1
        out[n] = torch.as_tensor(np.asarray(flat[off:off + k]), dtype=dtype).reshape(s)
        off += k
    return out, off


def split_actor(flat, D, K, dtype=torch.float64):
    flat = np.asarray(flat)
    out, off = _split(flat, actor_shapes(D, K), dtype)
    assert off == flat.size
    return out


def split_critic(flat, D, K, dtype=torch.float64):
    flat = np.asarray(flat)
    q0, off = _split(flat, q_shapes(D, K), dtype)
    q1, off2 = _split(flat[off:], q_shapes(D, K), dtype)
    assert off + off2 == flat.size
    return [q0, q1]


def actor_blocks(flat, D, K) -> Dict[str, np.ndarray]:
    return {k: v.numpy() for k, v in split_actor(flat, D, K).items()}


def critic_blocks(flat, D, K) -> Dict[str, np.ndarray]:
    qs = split_critic(flat, D, K)
    return {f"q{q}.{k}": v.numpy() for q in (0, 1) for k, v in qs[q].items()}


def _flat(blocks, names) -> torch.Tensor:
    return torch.cat([blocks[k].reshape(-1) for k in names])


# ------------------------------------------------------------------------------ stages
def _q(x, quant):
    return rne_bf16(x) if quant else x


def _f32(x, quant):  # a float32 the kernel stores and a later stage reads
    return x.float().to(x.dtype) if quant else x


def pack(s, a, s1, quant):
    """pack_kernel: the operand rows [s], [s1], [s | a]; xt and xp start as [s1 | .], [s | .]."""
    s, a, s1 = _q(s, quant), _q(a, quant), _q(s1, quant)
    return dict(xs=s, xs1=s1, xc=torch.cat([s, a], 1), xt_obs=s1, xp_obs=s)


def layout(w, quant):
    """adam_net_kernel's kernel-layout copy of a weight: RNE of the fp32 master."""
    return _q(w, quant)


def linear_relu(x, w, b, quant):
    """gemm_jobs E_FWD: relu(W x + b), W and x of type T, the bias fp32, stored as T."""
    return _q(torch.relu(x @ layout(w, quant).T + b), quant)


def policy_head(h, P, eps, defect=None):
    """heads_kernel HK_POLICY (to_action): -> y, logp, and what the backward reads (std, x - mean,
    tanh u), plus std.mean(-1)."""
    wm, wl = P["wm"], P["wl"]
    if defect == "swap_head_row":
        wm, wl = wm.clone(), wl.clone()
        wm[0], wl[0] = P["wl"][0], P["wm"][0]
    mean = h @ wm.T + P["bm"]
    tu = torch.tanh(h @ wl.T + P["bl"])
    ls = -5.0 + 3.5 * (tu + 1.0)
    sd = torch.exp(ls)
    x = mean + eps * sd
    y = torch.tanh(x)
    xm = x - mean
    lp = -(xm * xm) / (2.0 * (sd * sd)) - torch.log(sd) - LOG_SQRT_2PI
    lp = lp - torch.log((1.0 - y * y) + 1e-6)
    return dict(mean=mean, ls=ls, sd=sd, y=y, xm=xm, tu=tu, logp=lp.sum(-1), stdrow=sd.mean(-1))


def q_head(h, Q):
    return h @ Q["w3"] + Q["b3"]


def is_weights(probs, N, prio_exp, dtype):
    if probs is None:
        return torch.ones(N, dtype=dtype)
    w = probs.pow(-prio_exp)
    return w / w.max()


def critic_loss(t1, t2, q1, q2, logp1, r, done, w, alpha, gamma, n_div):
    """critic_loss_kernel up to dQ: -> y, dq [2][N], prio, the four metric rows."""
    mn = torch.minimum(t1, t2) - alpha * logp1
    y = r + torch.where(done, torch.zeros_like(r), torch.full_like(r, gamma)) * mn
    d1, d2 = y - q1, y - q2
    wn = w / n_div
    return dict(y=y, dq=[-(wn * (2.0 * d1)), -(wn * (2.0 * d2))],
                prio=(y - torch.minimum(q1, q2)).abs(),
                rowm=[d1 * d1 * w, d2 * d2 * w, q1, q2])


def dq_to_dh(dq, w3, h2, quant):
    """dh2 = dQ W3 (.) [h2 > 0], stored as T."""
    return _q(torch.where(h2 > 0, dq[:, None] * w3[None, :], torch.zeros_like(h2)), quant)


def dgrad(dy, w, hmask, quant):
    """gemm_jobs E_DGRAD: (dY W) (.) [h > 0] with W the kernel-layout (T) weight, stored as T."""
    return _q(torch.where(hmask > 0, dy @ layout(w, quant), torch.zeros_like(hmask)), quant)


def wgrad(dy, x, ones=None):
    """gemm_jobs E_WGRAD: dW = dY^T X and, from the row of ones after X's last feature, db."""
    ones = torch.ones(dy.shape[0], dtype=dy.dtype) if ones is None else ones
    return dy.T @ x, dy.T @ ones


def actor_loss(q1, q2, logp, alpha, N, assign=None, defect=None):
    """actor_loss_kernel: the loss term and d/dq_i = -1/N to the smaller (halved on a tie).
    assign: {row: 0 | 1} forces which network takes an undecided row's gradient."""
    g = -1.0 / N
    lt, eq = (q1 < q2).to(q1.dtype), (q1 == q2).to(q1.dtype)
    a1 = lt + 0.5 * eq
    if defect == "actor_min_q1":
        a1 = torch.ones_like(q1)
    for n, which in (assign or {}).items():
        a1[n] = 1.0 if which == 0 else 0.0
    mn = q1 if defect == "actor_min_q1" else torch.minimum(q1, q2)
    return dict(term=alpha * logp - mn, dq=[g * a1, g * (1.0 - a1)])


def head_bwd(dhp1, W1act, save, eps, alpha, N, A, ha2, quant):
    """actor_head_bwd_kernel: the closed-form backward of to_action (csrc/sac.h has the formulas);
    W1act [2][256][K] = the action columns of the critic's canonical first layers."""
    sd, y, xm, tu = save
    c = alpha / N
    dpi = dhp1[0] @ W1act[0] + dhp1[1] @ W1act[1]
    var, omy = sd * sd, 1.0 - y * y
    gy = dpi + c * (2.0 * y / (omy + 1e-6))
    gx = gy * omy - c * xm / var
    gs = gx * eps + c * (xm * xm) / (var * sd) - c / sd
    gm = gx + c * xm / var
    gu = gs * sd * (3.5 * (1.0 - tu * tu))
    dha2 = torch.where(ha2 > 0, gm @ A["wm"] + gu @ A["wl"], torch.zeros_like(ha2))
    return dict(gm=_q(gm, quant), gu=_q(gu, quant), dha2=_q(dha2, quant))


def clip_coef(norm, max_norm):
    return 1.0 if max_norm is None or max_norm <= 0 else min(max_norm / (norm + 1e-6), 1.0)


def adam(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-5):
    """torch.optim.Adam's step t (1-based) given the clipped gradient -> (p, m, v)."""
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)), m, v


def polyak(p, tgt, tau):
    return tau * p + (1.0 - tau) * tgt


def alpha_step(logp2, la, m, v, t, target_entropy, lr, eps=1e-5):
    """finalize_kernel's alpha part -> (loss, grad, new la, m, v)."""
    x = logp2 + target_entropy
    g = -x.mean()
    la1, m, v = adam(la, g, m, v, t, lr, eps=eps)
    return -(la * x).mean(), g, la1, m, v


# ------------------------------------------------------------------------------ the chain
def run(D: int, K: int, actor0, critic0, la0: float, batch, probs, eps3, *, tactor0=None,
        tcritic0=None, given: Optional[dict] = None, quant: bool = True, dtype=torch.float64,
        critic_lr=3e-3, actor_lr=3e-4, adam_eps=1e-5, max_grad_norm=40.0, tau=0.005, gamma=0.99,
        tune_alpha=True, prio_exponent=0.4, defect: Optional[str] = None) -> dict:
    """One step from zero Adam state.  given: logical tensors (module doc) and, as "critic1" /
    "actor1", the flat parameters after the critic's / actor's Adam step; a stage whose input is
    given reads it instead of the chain's own.  -> dict(t, cgrads, agrads (unclipped blocks),
    cnorm, anorm, ccoef, acoef, critic1, actor1, tcritic1, tactor1 (flat), la (la, g, m, v), met,
    qpi, undecided)."""
    given = given or {}
    t: Dict[str, torch.Tensor] = {}
    # `done.logical_not() * gamma` is a float32 tensor in the reference (bool x Python float), and
    # the kernel's gamma is a float: the step's discount is the float32 nearest to gamma
    gamma = float(np.float32(gamma))

    def T(x):
        return torch.as_tensor(np.asarray(x), dtype=dtype)

    def G(name):  # the stage input: the device's own when given, else the chain's
        return T(given[name]) if name in given else t[name]

    s, a, r, s1, done = batch
    N = s.shape[0]
    s, a, r, s1 = T(s).reshape(N, D), T(a).reshape(N, K), T(r).reshape(N), T(s1).reshape(N, D)
    done = torch.as_tensor(np.asarray(done)).reshape(N).bool()
    eps3 = T(eps3).reshape(3, N, K)
    pr = None if probs is None else T(probs).reshape(N)
    A0, C0 = split_actor(actor0, D, K, dtype), split_critic(critic0, D, K, dtype)
    TA0 = split_actor(actor0 if tactor0 is None else tactor0, D, K, dtype)
    TC0 = split_critic(critic0 if tcritic0 is None else tcritic0, D, K, dtype)
    alpha = math.exp(float(np.float32(la0))) if dtype == torch.float64 else float(np.exp(np.float32(la0)))
    with torch.no_grad():
        # ---- pack
        p = pack(s, a, s1, quant)
        t.update(xs=p["xs"], xs1=p["xs1"], xc=p["xc"])
        # ---- fwd_l1, fwd_l2: target actor on s1, Q1 / Q2 on [s | a], actor on s
        t["hta1"] = linear_relu(G("xs1"), TA0["w1"], TA0["b1"], quant)
        t["ha1"] = linear_relu(G("xs"), A0["w1"], A0["b1"], quant)
        for q in (0, 1):
            t[f"hc1_{q}"] = linear_relu(G("xc"), C0[q]["w1"], C0[q]["b1"], quant)
        t["hta2"] = linear_relu(G("hta1"), TA0["w2"], TA0["b2"], quant)
        t["ha2"] = linear_relu(G("ha1"), A0["w2"], A0["b2"], quant)
        for q in (0, 1):
            t[f"hc2_{q}"] = linear_relu(G(f"hc1_{q}"), C0[q]["w2"], C0[q]["b2"], quant)
        # ---- heads
        ht = policy_head(G("hta2"), TA0, eps3[0])
        ha = policy_head(G("ha2"), A0, eps3[1], defect)
        t["xt"] = torch.cat([p["xt_obs"], _q(ht["y"], quant)], 1)
        t["xp"] = torch.cat([p["xp_obs"], _q(ha["y"], quant)], 1)
        t["logp1"], t["logp"] = _f32(ht["logp"], quant), _f32(ha["logp"], quant)
        t["save"] = _f32(torch.stack([ha["sd"], ha["y"], ha["xm"], ha["tu"]]), quant)
        t["q1"] = _f32(q_head(G("hc2_0"), C0[0]), quant)
        t["q2"] = _f32(q_head(G("hc2_1"), C0[1]), quant)
        # ---- target critic on [s1 | a1]
        for q in (0, 1):
            t[f"htc1_{q}"] = linear_relu(G("xt"), TC0[q]["w1"], TC0[q]["b1"], quant)
        for q in (0, 1):
            t[f"htc2_{q}"] = linear_relu(G(f"htc1_{q}"), TC0[q]["w2"], TC0[q]["b2"], quant)
        # ---- critic loss
        w = is_weights(pr, N, prio_exponent, dtype)
        cl = critic_loss(q_head(G("htc2_0"), TC0[0]), q_head(G("htc2_1"), TC0[1]), G("q1"), G("q2"),
                         G("logp1"), r, done, w, alpha, gamma, N + 1 if defect == "wrong_n" else N)
        t["prio"] = cl["prio"]
        for q in (0, 1):
            t[f"dq_{q}"] = _q(cl["dq"][q], quant)
            t[f"dh2_{q}"] = dq_to_dh(cl["dq"][q], C0[q]["w3"], G(f"hc2_{q}"), quant)
        # ---- critic backward: dh1, then every weight gradient
        cg = {}
        for q in (0, 1):
            t[f"dhc1_{q}"] = dgrad(G(f"dh2_{q}"), C0[q]["w2"], G(f"hc1_{q}"), quant)
            cg[f"q{q}.w2"], cg[f"q{q}.b2"] = wgrad(G(f"dh2_{q}"), G(f"hc1_{q}"))
            gw3, gb3 = wgrad(G(f"dq_{q}")[:, None], G(f"hc2_{q}"))
            cg[f"q{q}.w3"], cg[f"q{q}.b3"] = gw3.reshape(H), gb3.reshape(())
            ones = torch.zeros(N, dtype=dtype) if defect == "ones_row" else None
            cg[f"q{q}.w1"], cg[f"q{q}.b1"] = wgrad(G(f"dhc1_{q}"), G("xc"), ones)
        # ---- clip + Adam + Polyak of the critic (zero moments, step 1)
        cflat = _flat(cg, C_BLOCKS)
        cnorm = float(cflat.double().norm().to(dtype))  # (the kernels sum per tile, then the slots)
        ccoef = 1.0 if defect == "clip_off" else clip_coef(cnorm, max_grad_norm)
        c_old = T(critic0)
        gclip = T(given["critic_grad"]) if "critic_grad" in given else cflat * ccoef
        z = torch.zeros_like(c_old)
        critic1, cm, cv = adam(c_old, gclip, z, z, 1, critic_lr, eps=adam_eps)
        tc_old = c_old if tcritic0 is None else T(tcritic0)
        tcritic1 = polyak(c_old if defect == "polyak_first" else critic1, tc_old, tau)
        if dtype != torch.float64 or quant:  # the masters are float32 on the device
            critic1f = critic1.float().to(dtype)
        else:
            critic1f = critic1
        C1 = split_critic(given["critic1"] if "critic1" in given else critic1f.numpy(), D, K, dtype)
        # ---- actor loss through the updated critic
        for q in (0, 1):
            t[f"hp1_{q}"] = linear_relu(G("xp"), C1[q]["w1"], C1[q]["b1"], quant)
        for q in (0, 1):
            t[f"hp2_{q}"] = linear_relu(G(f"hp1_{q}"), C1[q]["w2"], C1[q]["b2"], quant)
        qpi = [q_head(G("hp2_0"), C1[0]), q_head(G("hp2_1"), C1[1])]
        und = [int(n) for n in torch.nonzero(
            (qpi[0] - qpi[1]).abs() <= 1e-5 * (qpi[0].abs() + qpi[1].abs())).reshape(-1)]
        assign = {}
        if "dhp2_0" in given:  # an undecided row: the network the device sent the gradient to
            for n in und:
                assign[n] = 0 if np.any(np.asarray(given["dhp2_0"])[n] != 0) else 1
        al = actor_loss(qpi[0], qpi[1], G("logp"), alpha, N, assign, defect)
        for q in (0, 1):
            t[f"dhp2_{q}"] = dq_to_dh(al["dq"][q], C1[q]["w3"], G(f"hp2_{q}"), quant)
        for q in (0, 1):
            t[f"dhp1_{q}"] = dgrad(G(f"dhp2_{q}"), C1[q]["w2"], G(f"hp1_{q}"), quant)
        sh = 1 if defect == "w1_shift" else 0
        W1act = [torch.roll(C1[q]["w1"][:, D:], sh, 1) for q in (0, 1)]
        hb = head_bwd([G("dhp1_0"), G("dhp1_1")], W1act, G("save"), eps3[1], alpha, N, A0, G("ha2"),
                      quant)
        t.update(gm=hb["gm"], gu=hb["gu"], dha2=hb["dha2"])
        t["dha1"] = dgrad(G("dha2"), A0["w2"], G("ha1"), quant)
        ag = {}
        ag["w2"], ag["b2"] = wgrad(G("dha2"), G("ha1"))
        ag["wm"], ag["bm"] = wgrad(G("gm"), G("ha2"))
        ag["wl"], ag["bl"] = wgrad(G("gu"), G("ha2"))
        ag["w1"], ag["b1"] = wgrad(G("dha1"), G("xs"))
        aflat = _flat(ag, A_BLOCKS)
        anorm = float(aflat.double().norm().to(dtype))
        acoef = 1.0 if defect == "clip_off" else clip_coef(anorm, max_grad_norm)
        a_old = T(actor0)
        gclip = T(given["actor_grad"]) if "actor_grad" in given else aflat * acoef
        z = torch.zeros_like(a_old)
        actor1, am, av = adam(a_old, gclip, z, z, 1, actor_lr, eps=adam_eps)
        ta_old = a_old if tactor0 is None else T(tactor0)
        tactor1 = polyak(a_old if defect == "polyak_first" else actor1, ta_old, tau)
        actor1f = actor1.float().to(dtype) if (dtype != torch.float64 or quant) else actor1
        A1 = split_actor(given["actor1"] if "actor1" in given else actor1f.numpy(), D, K, dtype)
        # ---- alpha: a fresh sample from the updated actor
        la = dict(la=float(np.float32(la0)), g=0.0, m=0.0, v=0.0, loss=0.0)
        if tune_alpha:
            t["hb1"] = linear_relu(G("xs"), A1["w1"], A1["b1"], quant)
            t["hb2"] = linear_relu(G("hb1"), A1["w2"], A1["b2"], quant)
            t["logp2"] = _f32(policy_head(G("hb2"), A1, eps3[2])["logp"], quant)
            zero = torch.zeros((), dtype=dtype)
            loss, g, la1, m, v = alpha_step(G("logp2"), torch.tensor(la["la"], dtype=dtype), zero,
                                            zero, 1, -float(K), critic_lr, adam_eps)
            la = dict(la=float(la1), g=float(g), m=float(m), v=float(v), loss=float(loss))
        # ---- the metric rows and their means (finalize_kernel)
        t["rowm"] = torch.stack(cl["rowm"] + [al["term"], ha["stdrow"]])
        mean = G("rowm").mean(1)
        met = {"qf1_loss": float(mean[0]), "qf2_loss": float(mean[1]), "qf1": float(mean[2]),
               "qf2": float(mean[3]), "qf_loss": float((mean[0] + mean[1]) / 2.0),
               "critic_grad_norm": cnorm, "actor_loss": float(mean[4]), "actor_std": float(mean[5]),
               "actor_grad_norm": anorm, "alpha_loss": la["loss"], "alpha": alpha}
    num = lambda d: {k: v.double().numpy() for k, v in d.items()}  # noqa: E731
    return dict(t=num(t), cgrads=num(cg), agrads=num(ag), cnorm=cnorm, anorm=anorm, ccoef=ccoef,
                acoef=acoef, critic1=critic1.double().numpy(), actor1=actor1.double().numpy(),
                tcritic1=tcritic1.double().numpy(), tactor1=tactor1.double().numpy(),
                cm=cm.double().numpy(), cv=cv.double().numpy(), am=am.double().numpy(),
                av=av.double().numpy(), la=la, met=met,
                qpi=[x.double().numpy() for x in qpi], undecided=und, assign=assign)
