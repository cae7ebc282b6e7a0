"""ORACLE -- test infrastructure only.  References of the learner step's stages, one function
each, for teacher-forced checks of the bf16 (and fp32) kernels.

Every function takes the tensors its kernel stage READS (in the layouts ``Engine.debug_tensor``
exports, DESIGN §3: activations channels-last, the 1024 features in p*64+c order) and returns
what the stage WRITES, before any rounding to bf16, evaluated in ``dtype`` (float64 for the
reference, float32 for the CPU stand-in of the kernels).  What each stage reads, from the
kernels:

  conv1      relu(conv(w1, image bytes) * (1/255) + b1): the bytes are exact in bf16, the scale
             and the bias are applied to the fp32 accumulator (conv1.h c1_epi).  mask1 bit c =
             channel c > 0.
  conv2      relu(conv(w2, act1) + b2) on the rounded act1.
  conv3+LN   v = relu(conv(w3, act2) + b3) unrounded in fp32; mean / rstd and y = LN(v) come
             from that unrounded v, act3 is v rounded (lnorm.h ln_frame_epilogue).
  fc         z = wfc y + bfc; zg = gelu'(z) stays fp32, h = gelu(z) is rounded; z is not kept.
  heads      heads = wh h + bh, fp32 [N][16].
  head bwd   dH (d loss / d heads, from the fp32 heads) is rounded in LDS (head.h phase 2c);
             dz = zg * (q(dH) wh); d wh = q(dH)^T h; d bh = sum q(dH).
  fc bwd     dy = dz wfc (fp32); d wfc = dz^T y; d bfc = sum dz -- the rounded dz (the weight-
             gradient GEMM sums the rows it reads, gemm.h gemm_wg_body).
  LN bwd     xh = (act3 - mean) * rstd from the ROUNDED act3 and the fp32 stats; d gamma = sum
             dy xh, d beta = sum dy; dact3 = [act3 > 0] rstd (dy gamma - S1 - xh S2) (lnc3.h).
  conv3 bwd  dact2 = [act2 > 0] col2im(q(dact3) w3); d w3 from (q(dact3), act2); d b3 = sum
             q(dact3).
  conv2 bwd  d w2 from (q(dact2), act1); d b2 = sum q(dact2); dY1 = [mask1] col2im(q(dact2) w2),
             which never reaches HBM.
  conv1 bwd  d b1 = sum of the UNROUNDED fp32 dY1 (conv1.h: bsum adds v before the bf16 store);
             d w1 = q(dY1)^T image bytes * (1/255).

The Ape-X DQN step (algo="dqn": the dueling net, the projection 512 wide) runs the same stages
around its own head, ``dqn_head``; its step kernel keeps the heads in LDS (dqn_head_step.h), so
that stage reads the exported h.  The distributional (IQN) actor path's forward (algo="iqn") has a
section of its own below.

In the bf16 mode every weight is RNE_bf16(master fp32) (kernels.h pack_params, ``(T)p``); biases,
LayerNorm gamma / beta and the statistics stay fp32.  ``quant=False`` switches every rounding off
(the fp32 mode, and the chain identity against ref_cpu).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu

BLOCKS = ("w1", "b1", "w2", "b2", "w3", "b3", "lng", "lnb", "wfc", "bfc", "wa", "ba", "wc", "bc")
T_TENSORS = ("act1", "act2", "act3", "y", "h", "dz", "dact3", "dact2")  # compute type
F32_TENSORS = ("lnstat", "zg", "heads", "dy")
FORWARD_TENSORS = ("act1", "act2", "act3", "lnstat", "y", "zg", "h", "heads")
LN_EPS = 1e-5
VCOL = 15
# export feature j = p*64 + c  ->  canonical (NCHW flatten) feature c*16 + p
_PERM = torch.tensor([(j & 63) * 16 + (j >> 6) for j in range(1024)])


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 (ties to even), returned in x's dtype.  float64 is rounded
    directly (not through float32: a double rounding could land on the other side of a tie)."""
    if x.dtype == torch.float32:
        return x.bfloat16().float()
    _, e = torch.frexp(x)
    ulp = torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-126) - 7)
    return torch.round(x / ulp) * ulp


def ulp_bf16(r: np.ndarray) -> np.ndarray:
    """2^(floor(log2 |r|) - 7): the spacing of bf16 at r (0 at r = 0)."""
    r = np.asarray(r, np.float64)
    _, e = np.frexp(r)
    return np.where(r == 0, 0.0, np.ldexp(1.0, np.maximum(e - 1, -126) - 7))


def block_shapes(A: int, algo: str = "impala"):
    """(block name, shape) of the 14 canonical blocks: the IMPALA / PPO net's, or -- algo "dqn" --
    the dueling net's (impala_amd.dqn.net_specs: the same order, the projection 512 wide, the
    advantage head in the actor's place and the value head in the critic's)."""
    if algo == "dqn":
        from impala_amd.dqn import net_specs
        return [(n, s) for n, (_, s) in zip(BLOCKS, net_specs(A))]
    return [(n, (A,) + s[1:] if k.startswith("model.actor") else s)
            for n, (k, s) in zip(BLOCKS, ref_cpu.PARAM_SPECS)]


def split_flat(flat, A: int, algo: str = "impala") -> Dict[str, np.ndarray]:
    """A flat parameter / gradient vector -> its 14 canonical blocks."""
    out, off = {}, 0
    for n, s in block_shapes(A, algo):
        k = int(np.prod(s))
        out[n] = np.asarray(flat[off:off + k]).reshape(s)
        off += k
    assert off == len(flat)
    return out


class Weights:
    """The weights as the kernels see them: conv / FC / head weights rounded to bf16 when
    ``quant``, the vectors fp32; the 1024-feature axes in the export order p*64+c; the heads as
    one [16][hid] matrix (rows 0..A-1 actor / advantage, row 15 critic / value).  ``hid``: the
    projection's width, 256 (the IMPALA / PPO net) or 512 (the dueling net, algo "dqn")."""

    def __init__(self, flat, A: int, quant: bool, dtype=torch.float64, hid: int = 256,
                 algo: str = "impala"):
        src = np.asarray(flat, np.float32 if quant else np.float64)  # (the master weights are fp32)
        b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
             for k, v in split_flat(src, A, algo).items()}
        assert b["wfc"].shape[0] == hid, (b["wfc"].shape, hid)
        q = rne_bf16 if quant else (lambda t: t)
        self.A, self.hid = A, hid
        self.w1, self.w2, self.w3 = q(b["w1"]), q(b["w2"]), q(b["w3"])
        self.b1, self.b2, self.b3 = b["b1"], b["b2"], b["b3"]
        self.lng, self.lnb = b["lng"][_PERM], b["lnb"][_PERM]
        self.wfc, self.bfc = q(b["wfc"])[:, _PERM], b["bfc"]
        self.wh = torch.zeros(16, hid, dtype=dtype)
        self.wh[:A], self.wh[VCOL] = q(b["wa"]), q(b["wc"])[0]
        self.bh = torch.zeros(16, dtype=dtype)
        self.bh[:A], self.bh[VCOL] = b["ba"], b["bc"][0]


def _nchw(x, H, C):
    return x.reshape(-1, H, H, C).permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------- forward
def conv1_fwd(obs_u8, W: Weights):
    """image bytes [N,3,64,64] -> act1 [N,15,15,32] (unrounded)."""
    x = F.conv2d(obs_u8.to(W.w1.dtype), W.w1, stride=4) * (1.0 / 255.0) + W.b1.view(1, -1, 1, 1)
    return _nhwc(x.clamp_min(0))


def mask_bits(act1) -> np.ndarray:
    """act1 [N,15,15,32] -> mask1 uint32 [N,225], bit c = channel c > 0."""
    b = (np.asarray(act1) > 0).reshape(-1, 225, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def conv2_fwd(act1, W: Weights):
    """act1 [N,15,15,32] -> act2 [N,6,6,64] (unrounded)."""
    x = F.conv2d(_nchw(act1, 15, 32), W.w2, stride=2) + W.b2.view(1, -1, 1, 1)
    return _nhwc(x.clamp_min(0))


def conv3_ln_fwd(act2, W: Weights):
    """act2 [N,6,6,64] -> (act3 [N,1024] unrounded, lnstat [N,2] = (mean, rstd), y [N,1024])."""
    x = F.conv2d(_nchw(act2, 6, 64), W.w3) + W.b3.view(1, -1, 1, 1)
    v = _nhwc(x.clamp_min(0)).reshape(-1, 1024)
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    y = (v - mean) * rstd * W.lng + W.lnb
    return v, torch.cat([mean, rstd], 1), y


def fc_fwd(y, W: Weights):
    """y [N,1024] -> (zg = gelu'(z) [N,256], h = gelu(z) unrounded); exact (erf) GELU."""
    z = y @ W.wfc.T + W.bfc
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi), z * cdf


def heads_fwd(h, W: Weights):
    """h [N,256] -> heads [N,16] (logits 0..A-1, value at 15, the rest 0)."""
    return h @ W.wh.T + W.bh


# ------------------------------------------------------------------------------- loss head
def impala_head(heads, batch, A: int, dtype=torch.float64, entropy_coeff: float = 0.01):
    """The V-trace loss on the exported heads [B*T,16] -> (dH [N,16] unrounded, metrics dict
    with loss / entropy / td / pg / kl / ratio and pg_abs = mean |log pi(a) adv|, the scale of
    train/pg's normwise bound)."""
    _, act, rew, disc, mu = batch
    B, T = act.shape
    hd = np.asarray(heads, np.float64).reshape(B, T, 16)
    o = ref_cpu.loss_from_outputs(hd[..., :A], hd[..., VCOL], act, rew, disc, mu,
                                  entropy_coeff=entropy_coeff, dtype=dtype)
    dH = torch.zeros(B, T, 16, dtype=dtype)
    dH[..., :A] = torch.from_numpy(o["dlogits"]).to(dtype)
    dH[..., VCOL] = torch.from_numpy(o["dvalues"]).to(dtype)
    lg = torch.from_numpy(hd[..., :A])
    logpa = torch.log_softmax(lg, -1).gather(-1, torch.from_numpy(np.asarray(act))[..., None])[..., 0]
    met = {k: o[k] for k in ("loss", "entropy", "td", "pg", "kl", "ratio")}
    met["pg_abs"] = float((logpa[:, :-1] * torch.from_numpy(np.asarray(o["adv"], np.float64))).abs().mean())
    return dH.reshape(B * T, 16), met


def ppo_head(heads, batch, A: int, dtype=torch.float64, entropy_coeff: float = 0.01,
             clip_coeff: float = 0.1):
    """ref_cpu.ppo_loss (the code behind ppo_loss_from_outputs) on the exported heads [N,16], in
    ``dtype`` -> (dH [N,16] unrounded, metrics dict)."""
    _, act, tgt, mu = batch
    hd = torch.from_numpy(np.asarray(heads, np.float64)).to(dtype)
    lg = hd[:, :A].clone().requires_grad_(True)
    v = hd[:, VCOL:VCOL + 1].clone().requires_grad_(True)
    b = (None, torch.from_numpy(np.asarray(act, np.int64)),
         torch.from_numpy(np.asarray(tgt)).to(dtype), torch.from_numpy(np.asarray(mu)).to(dtype))
    loss, met = ref_cpu.ppo_loss(ref_cpu._Outputs(lg, v), b, entropy_cost=entropy_coeff,
                                 clip_coeff=clip_coeff)
    loss.backward()
    dH = torch.zeros(hd.shape[0], 16, dtype=dtype)
    dH[:, :A], dH[:, VCOL] = lg.grad, v.grad[:, 0]
    return dH, {k.split("/")[1]: float(x) for k, x in met.items()}


def dqn_head(h, batch, A: int, W: Weights, beta: float = 0.4, dtype=torch.float64, err_abs=None,
             mean_rows: Optional[int] = None, pnorm=None):
    """The Ape-X loss on the exported h [N,512] (dqn_head_step.h phases 1 and 2; the step kernel
    keeps its heads in LDS, so they are formed here: heads = wh h + bh in ``dtype``):
      q = (v + adv_a) - mean_{k<A} adv_k;  err = target - q;  w = p^-beta / (min p)^-beta (1
      without probabilities; beta as the kernel holds it, a float32);  dq = -err w / N;
      dH[k<A] = [k = a] dq - dq / A, dH[15] = dq, rows A..14 zero.
    ``err_abs`` [N]: the step's own priorities |err| (the kernel stores fabsf(err)); dH then is
    built from that magnitude under the reference's sign.  q, the metrics and the returned
    priorities are always the reference's own.
    ``mean_rows`` / ``pnorm``: a number of rows to average over instead of A, a probability to
    normalise by instead of min p (defects for the sensitivity tests).
    -> (dH [N,16] unrounded, metrics q / target / priorities / loss (means; loss = 1/2 mean err^2
    w) and q_abs = mean |q_a| (the scale of q's normwise bound), {"q": q_a [N], "prio": |err|
    [N], "w": [N]} in ``dtype``)."""
    _, act, tgt, prob = batch
    h = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).to(dtype) \
        if not torch.is_tensor(h) else h.to(dtype)
    N = h.shape[0]
    hd = heads_fwd(h, W)
    a = torch.from_numpy(np.asarray(act, np.int64)).reshape(-1)
    adv_a = hd[:, :A].gather(1, a[:, None])[:, 0]
    R = mean_rows or A
    q = (hd[:, VCOL] + adv_a) - hd[:, :R].sum(1) / R
    t = torch.from_numpy(np.asarray(tgt, np.float32)).reshape(-1).to(dtype)
    err0 = err = t - q  # (the metrics and the returned priorities are the reference's own)
    if err_abs is not None:
        mag = torch.from_numpy(np.asarray(err_abs, np.float64)).reshape(-1).to(dtype)
        err = torch.where(err0 < 0, -mag, mag)
    if prob is None:
        w = torch.ones_like(q)
    else:
        p = torch.from_numpy(np.asarray(prob, np.float32)).reshape(-1).to(dtype)
        b = torch.tensor(float(np.float32(beta)), dtype=dtype)
        pn = p.min() if pnorm is None else torch.as_tensor(float(pnorm), dtype=dtype)
        w = p.pow(-b) / pn.pow(-b)
    dq = -(err * w) / N
    dH = torch.zeros(N, 16, dtype=dtype)
    dH[:, :A] = (-dq / A)[:, None]
    dH[torch.arange(N), a] += dq
    dH[:, VCOL] = dq
    met = {"q": float(q.mean()), "target": float(t.mean()), "priorities": float(err0.abs().mean()),
           "loss": float(0.5 * (err0 * err0 * w).mean()), "q_abs": float(q.abs().mean())}
    return dH, met, {"q": q.double().numpy(), "prio": err0.abs().double().numpy(),
                     "w": w.double().numpy()}


# ------------------------------------------------------------------------------- backward
def head_bwd(qdH, zg, h, W: Weights):
    """q(dH) [N,16], zg, h [N,256] -> (dz unrounded, d wh [16,256], d bh [16])."""
    return zg * (qdH @ W.wh), qdH.T @ h, qdH.sum(0)


def fc_bwd(dz, y, W: Weights):
    """dz [N,256] (rounded), y [N,1024] -> (dy [N,1024], d wfc [256,1024] export order, d bfc)."""
    return dz @ W.wfc, dz.T @ y, dz.sum(0)


def ln_bwd(dy, act3, lnstat, W: Weights, xh=None):
    """dy fp32, act3 (rounded), lnstat -> (dact3 unrounded, d gamma, d beta) (export order).
    ``xh``: a normalised input to use instead of the kernel's (act3 - mean) * rstd."""
    mean, rstd = lnstat[:, :1], lnstat[:, 1:]
    if xh is None:
        xh = (act3 - mean) * rstd
    gd = dy * W.lng
    s1, s2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    dact3 = torch.where(act3 > 0, rstd * (gd - s1 - xh * s2), torch.zeros_like(dy))
    return dact3, (dy * xh).sum(0), dy.sum(0)


def conv3_bwd(dact3, act2, W: Weights, w3=None):
    """dact3 [N,1024] (rounded), act2 -> (dact2 unrounded, d w3 [64,64,3,3], d b3).
    ``w3``: a weight to use in the dgrad instead of W.w3."""
    g = _nchw(dact3, 4, 64).contiguous()
    x = _nchw(act2, 6, 64).contiguous()
    dx = torch.nn.grad.conv2d_input(x.shape, W.w3 if w3 is None else w3, g)
    dact2 = torch.where(x > 0, dx, torch.zeros_like(dx))
    return _nhwc(dact2), torch.nn.grad.conv2d_weight(x, W.w3.shape, g), g.sum((0, 2, 3))


def conv2_bwd(dact2, act1, W: Weights):
    """dact2 [N,6,6,64] (rounded), act1 (its sign = mask1) -> (dY1 [N,15,15,32] unrounded,
    d w2 [64,32,4,4], d b2)."""
    g = _nchw(dact2, 6, 64).contiguous()
    x = _nchw(act1, 15, 32).contiguous()
    dx = torch.nn.grad.conv2d_input(x.shape, W.w2, g, stride=2)
    dY1 = torch.where(x > 0, dx, torch.zeros_like(dx))
    return _nhwc(dY1), torch.nn.grad.conv2d_weight(x, W.w2.shape, g, stride=2), g.sum((0, 2, 3))


def conv1_bwd(dY1, qdY1, obs_u8, W: Weights):
    """dY1 unrounded (the bias sum), q(dY1) (the weight gradient), image bytes ->
    (d w1 [32,3,8,8], d b1)."""
    x = obs_u8.to(W.w1.dtype)
    dw = torch.nn.grad.conv2d_weight(x, W.w1.shape, _nchw(qdY1, 15, 32).contiguous(), stride=4)
    return dw * (1.0 / 255.0), dY1.sum((0, 1, 2))


def _head_grads(g: Dict[str, torch.Tensor], A: int) -> Dict[str, np.ndarray]:
    """(d wh [16,hid], d bh [16]) -> the four canonical head blocks."""
    return {"wa": g["wh"][:A].double().numpy(), "ba": g["bh"][:A].double().numpy(),
            "wc": g["wh"][VCOL:VCOL + 1].double().numpy(),
            "bc": g["bh"][VCOL:VCOL + 1].double().numpy()}


def _canon_grads(g: Dict[str, torch.Tensor], A: int) -> Dict[str, np.ndarray]:
    """Stage gradients (export order) -> the 14 canonical blocks."""
    inv = torch.empty_like(_PERM)
    inv[_PERM] = torch.arange(1024)
    out = {k: g[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "bfc")}
    out["lng"], out["lnb"], out["wfc"] = g["lng"][inv], g["lnb"][inv], g["wfc"][:, inv]
    out["wa"], out["ba"] = g["wh"][:A], g["bh"][:A]
    out["wc"], out["bc"] = g["wh"][VCOL:VCOL + 1], g["bh"][VCOL:VCOL + 1]
    return {k: out[k].double().numpy() for k in BLOCKS}


def run(flat, batch, A: int, given: Optional[dict] = None, quant: bool = True,
        dtype=torch.float64, algo: str = "impala", forward_only: bool = False,
        hid: int = 256, beta: float = 0.4, head_only: bool = False) -> dict:
    """Every stage of one step.  ``given`` = the tensors of a real step (teacher forcing: each
    stage reads ITS inputs from there, so the outputs are references for that step's tensors);
    None chains the stages on their own outputs, rounded to bf16 where the kernels round when
    ``quant`` (dtype float32: the CPU stand-in of the bf16 kernels; quant False, float64: the
    network itself).  -> {"t": name -> tensor before rounding (numpy float64), "grads": the 14
    canonical blocks, "met": metrics, "mask1": uint32}.  ``given`` may also carry "dY1" (an
    unrounded conv2 input gradient to round and use instead of the run's own).

    ``algo="dqn"``: the dueling net (``hid`` 512 whatever is passed; blocks of
    impala_amd.dqn.net_specs), batch = (obs, act, target, prob-or-None), the head stage
    ``dqn_head`` with importance exponent ``beta``; ``given`` may carry "prio", the step's own
    priorities (dqn_head's ``err_abs``), and "qdH", a rounded dH to use instead of the run's own.
    The output also has "prio" [N] and "q" [N] (q_a).  ``head_only``: with ``given``, the head
    stage and its backward alone ("t" holds heads, dH, dz; "grads" the four head blocks).

    ``algo="iqn"``: the distributional actor path's forward (``run_iqn``), batch = (obs, taus);
    ``head_only``: with ``given``, without the trunk."""
    if algo == "iqn":
        return run_iqn(flat, batch, A, given, quant, dtype,
                       trunk=not (head_only and given is not None))
    dqn = algo == "dqn"
    if dqn:
        hid = 512
    W = Weights(flat, A, quant, dtype, hid, "dqn" if dqn else "impala")
    q = rne_bf16 if quant else (lambda t: t)
    t: Dict[str, torch.Tensor] = {}

    def inp(name):  # the tensor a stage reads
        if given is not None:
            return torch.from_numpy(np.ascontiguousarray(given[name], dtype=np.float64)).to(dtype)
        return q(t[name]) if name in T_TENSORS or name in ("dH", "dY1") else t[name]

    obs = torch.from_numpy(np.ascontiguousarray(batch[0])).reshape(-1, 3, 64, 64)
    out = {}
    if not (head_only and given is not None):
        with torch.no_grad():
            t["act1"] = conv1_fwd(obs, W)
            t["act2"] = conv2_fwd(inp("act1"), W)
            t["act3"], t["lnstat"], t["y"] = conv3_ln_fwd(inp("act2"), W)
            t["zg"], t["h"] = fc_fwd(inp("y"), W)
        out["mask1"] = mask_bits(inp("act1").numpy())
    with torch.no_grad():
        t["heads"] = heads_fwd(inp("h"), W)
    if not forward_only:
        if dqn:
            with torch.no_grad():
                t["dH"], out["met"], x = dqn_head(
                    inp("h"), batch, A, W, beta, dtype,
                    err_abs=None if given is None else given.get("prio"))
            out["prio"], out["q"] = x["prio"], x["q"]
        else:
            head = impala_head if algo == "impala" else ppo_head
            t["dH"], out["met"] = head(inp("heads").double().numpy(), batch, A, dtype=dtype)
        with torch.no_grad():
            qdH = q(t["dH"])  # (never exported: always the run's own)
            if given is not None and "qdH" in given:
                qdH = torch.from_numpy(np.asarray(given["qdH"], np.float64)).to(dtype)
            g = {}
            t["dz"], g["wh"], g["bh"] = head_bwd(qdH, inp("zg"), inp("h"), W)
            if head_only:
                out["grads"] = _head_grads(g, A)
                out["t"] = {k: v.double().numpy() for k, v in t.items()}
                return out
            t["dy"], g["wfc"], g["bfc"] = fc_bwd(inp("dz"), inp("y"), W)
            t["dact3"], g["lng"], g["lnb"] = ln_bwd(inp("dy"), inp("act3"), inp("lnstat"), W)
            t["dact2"], g["w3"], g["b3"] = conv3_bwd(inp("dact3"), inp("act2"), W)
            t["dY1"], g["w2"], g["b2"] = conv2_bwd(inp("dact2"), inp("act1"), W)
            qdY1 = q(t["dY1"])
            if given is not None and "dY1" in given:
                qdY1 = q(torch.from_numpy(np.asarray(given["dY1"], np.float64)).to(dtype))
            g["w1"], g["b1"] = conv1_bwd(t["dY1"], qdY1, obs, W)
        out["grads"] = _canon_grads(g, A)
    out["t"] = {k: v.double().numpy() for k, v in t.items()}
    return out


# ------------------------------------------------------------------------------- IQN forward
# The distributional actor path (csrc/iqn.hip; algo="iqn", forward only).  R = n W rows, row
# r = f W + k.  What each stage reads, from the kernels:
#   trunk     conv1, conv2 as above; conv3 WITHOUT the LayerNorm: the handle runs the forward in
#             trunk-only mode, act3 = relu(conv(w3, act2) + b3) rounded is all the head reads.
#   embed_ln  iqn_embed_ln_kernel: e[r][i] = cos(fl(fl(pi) (i + 1)) tau_r), i = 0..63, the argument
#             formed in float32 (two roundings, as torch forms torch.pi * embedding_range * tau);
#             the tile is of the compute type, so e is ROUNDED in the bf16 mode; pre = Wq e + bq
#             (Wq rounded as packed), phi = erf-GELU(pre), z = act3[r // W] phi, y = LN(z) gamma +
#             beta with the two-pass variance and eps 1e-5, all fp32; y stored in the compute type.
#   fc/heads  FcFwd / HeadsFwd (the 512-wide projection's) over the R rows: fc_fwd, heads_fwd.
#   q         iqn_q_kernel: the dueling formula on the heads (dueling_q).
IQN_COS = 64
IQN_HEAD_TENSORS = ("y", "zg", "h", "heads")
IQN_FORWARD_TENSORS = ("act1", "act2", "act3") + IQN_HEAD_TENSORS
# The maximum error of the device cosf in fp32 ulps.  ASSUMED: the HIP programming guide's table
# of device math functions (which the DQN stage test took powf's 1 ULP from) is not at hand; 4 is
# taken in its place, so the margin of iqn_undecided is 8 fp32 ulps of the cosine.
COSF_ULPS = 4


def iqn_split(flat, A: int):
    """One IQN net's flat parameters (impala_amd.iqn.net_specs) -> (the dueling net's flat vector
    without the quantile layer's segment, Wq [1024,64], bq [1024])."""
    from impala_amd.iqn import net_specs
    flat = np.asarray(flat)
    off, parts = 0, {}
    for k, s in net_specs(A):
        n = int(np.prod(s))
        parts[k] = (off, n)
        off += n
    assert off == flat.size, (off, flat.size)
    (ow, nw), (ob, nb) = (parts["q.quantile_layer.output_layer.0." + x] for x in ("weight", "bias"))
    assert ob == ow + nw
    return (np.concatenate([flat[:ow], flat[ob + nb:]]), flat[ow:ow + nw].reshape(1024, IQN_COS),
            flat[ob:ob + nb])


class IqnWeights(Weights):
    """``Weights`` of the dueling net plus the quantile layer's: wq [1024,64] (rounded to bf16
    when ``quant``: iqn_pack_kernel's ``(T)src``) and bq [1024] fp32, the features in the export
    order p*64+c (the pack kernel's permutation)."""

    def __init__(self, flat, A: int, quant: bool, dtype=torch.float64):
        dflat, wq, bq = iqn_split(np.asarray(flat, np.float32 if quant else np.float64), A)
        super().__init__(dflat, A, quant, dtype, 512, "dqn")
        wq = torch.from_numpy(np.ascontiguousarray(wq)).to(dtype)
        self.wq = (rne_bf16(wq) if quant else wq)[_PERM]
        self.bq = torch.from_numpy(np.ascontiguousarray(bq)).to(dtype)[_PERM]


def iqn_cos_arg(taus) -> np.ndarray:
    """taus [R] -> the cosine's argument [R,64] exactly as the kernel (and torch) form it in
    float32: fl(fl(fl(pi) i) tau), i = 1..64."""
    pi_i = np.float32(np.pi) * np.arange(1, IQN_COS + 1, dtype=np.float32)
    assert pi_i.dtype == np.float32
    return pi_i[None, :] * np.asarray(taus, np.float32).reshape(-1, 1)


def iqn_cos(taus, dtype=torch.float64):
    """-> e [R,64] unrounded: the cosine of the float32 argument taken in ``dtype``."""
    return torch.cos(torch.from_numpy(iqn_cos_arg(taus)).to(dtype))


def ulp_f32(r: np.ndarray) -> np.ndarray:
    """2^(floor(log2 |r|) - 23): the spacing of float32 at r (0 at r = 0)."""
    r = np.asarray(r, np.float64)
    _, e = np.frexp(r)
    return np.where(r == 0, 0.0, np.ldexp(1.0, np.maximum(e - 1, -126) - 23))


def iqn_undecided(taus):
    """The elements of the bf16 cosine tile whose rounding the float64 cosine cannot decide: the
    kernel rounds the device cosf, which may differ from the float64 value c by COSF_ULPS fp32
    ulps; the margin is twice that, and an element is undecided when c - margin and c + margin
    round to different bf16.  -> (lower rounding [R,64], upper rounding, mask of the undecided)."""
    c = np.cos(iqn_cos_arg(taus).astype(np.float64))
    m = 2 * COSF_ULPS * ulp_f32(c)
    lo = rne_bf16(torch.from_numpy(c - m)).numpy()
    hi = rne_bf16(torch.from_numpy(c + m)).numpy()
    return lo, hi, lo != hi


def iqn_embed_ln_rows(x, e, W: "IqnWeights", defect: Optional[str] = None):
    """x [R,1024] (the frame's act3 of every row), e [R,64] (the cosine tile as the MFMA reads
    it) -> y [R,1024] unrounded.  ``defect`` (for the sensitivity tests): "tanh_gelu", "no_bq",
    "raw_second_moment" (the variance without the mean subtracted)."""
    pre = e @ W.wq.T
    if defect != "no_bq":
        pre = pre + W.bq
    if defect == "tanh_gelu":
        phi = 0.5 * pre * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (pre + 0.044715 * pre ** 3)))
    else:
        phi = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    z = x * phi
    mean = z.mean(1, keepdim=True)
    var = (z * z).mean(1, keepdim=True) if defect == "raw_second_moment" else \
        ((z - mean) ** 2).mean(1, keepdim=True)
    return (z - mean) / torch.sqrt(var + LN_EPS) * W.lng + W.lnb


def iqn_embed_ln(act3, e, W: "IqnWeights", n_tau: int, defect: Optional[str] = None):
    """act3 [n,1024] (rounded), e [n n_tau, 64] -> y [R,1024] unrounded: row r reads frame
    r // n_tau.  ``defect`` "first_frame": every row of a 16-row tile reads the frame of the
    tile's first row; the others as iqn_embed_ln_rows."""
    r = torch.arange(e.shape[0])
    if defect == "first_frame":
        r = r // 16 * 16
    return iqn_embed_ln_rows(act3[r // n_tau], e, W, None if defect == "first_frame" else defect)


def dueling_q(heads, A: int, mean_cols: Optional[int] = None):
    """heads [R,16] -> q [R,A] = (v + adv_k) - mean_{k<A} adv (``mean_cols``: columns to average
    over instead of A, a defect)."""
    M = mean_cols or A
    return (heads[:, VCOL:VCOL + 1] + heads[:, :A]) - heads[:, :M].sum(1, keepdim=True) / M


def run_iqn(flat, batch, A: int, given: Optional[dict] = None, quant: bool = True,
            dtype=torch.float64, trunk: bool = True) -> dict:
    """``run`` for algo "iqn": batch = (obs u8 [n,3,64,64], taus float32 [n,W]); flat = one IQN
    net's parameters.  ``trunk`` False: the head stages alone, on given["act3"].  -> {"t": the
    tensors before rounding, "mask1" (with the trunk), "q" [R,A], "e": the unrounded cosine tile}."""
    obs, taus = batch
    taus = np.asarray(taus, np.float32)
    n_tau = taus.shape[1]
    W = IqnWeights(flat, A, quant, dtype)
    q = rne_bf16 if quant else (lambda t: t)
    t: Dict[str, torch.Tensor] = {}

    def inp(name):
        if given is not None:
            return torch.from_numpy(np.ascontiguousarray(given[name], dtype=np.float64)).to(dtype)
        return q(t[name]) if name in T_TENSORS else t[name]

    out = {}
    with torch.no_grad():
        if trunk:
            t["act1"] = conv1_fwd(torch.from_numpy(np.ascontiguousarray(obs)).reshape(-1, 3, 64, 64), W)
            t["act2"] = conv2_fwd(inp("act1"), W)
            t["act3"] = conv3_ln_fwd(inp("act2"), W)[0]
            out["mask1"] = mask_bits(inp("act1").numpy())
        e = iqn_cos(taus.reshape(-1), dtype)
        t["y"] = iqn_embed_ln(inp("act3"), q(e), W, n_tau)
        t["zg"], t["h"] = fc_fwd(inp("y"), W)
        t["heads"] = heads_fwd(inp("h"), W)
        out["q"] = dueling_q(inp("heads"), A).double().numpy()
    out["e"] = e.double().numpy()
    out["t"] = {k: v.double().numpy() for k, v in t.items()}
    return out


def stand_in_tensors(run_out: dict, quant: bool = True) -> dict:
    """What the kernels would export after a chained run: the workspace tensors alone (dH and
    dY1 never leave LDS), those of the compute type rounded."""
    return {k: (rne_bf16(torch.from_numpy(v).float()).double().numpy()
                if quant and k in T_TENSORS else v)
            for k, v in run_out["t"].items() if k in T_TENSORS + F32_TENSORS}


# ------------------------------------------------------------------------------- figures
def f32_figures(got, r):
    """-> worst |got - r| / (|r| + rms r) (the normwise measure of test_gpu_parity_full.py)."""
    got, r = np.asarray(got, np.float64), np.asarray(r, np.float64)
    rms = float(np.sqrt(np.mean(r * r)))
    return float(np.max(np.abs(got - r) / (np.abs(r) + rms + 1e-300)))


def bf16_figures(got, r):
    """got: a bf16 tensor (as float), r: its float64 reference before rounding ->
    (worst |got - r| / (ulp(r) + 1e-5 (|r| + rms r)), share of elements with got != RNE_bf16(r),
    worst |got - r| in ulp(r) over the mismatching elements)."""
    got, r = np.asarray(got, np.float64), np.asarray(r, np.float64)
    rms = float(np.sqrt(np.mean(r * r)))
    d = np.abs(got - r)
    tol = ulp_bf16(r) + 1e-5 * (np.abs(r) + rms)
    worst = float(np.max(d / (tol + 1e-300)))
    want = rne_bf16(torch.from_numpy(np.ascontiguousarray(r))).numpy()
    miss = got != want
    u = ulp_bf16(r)
    wu = float(np.max(d[miss] / np.maximum(u[miss], 1e-300))) if miss.any() else 0.0
    return worst, float(np.mean(miss)), wu


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
