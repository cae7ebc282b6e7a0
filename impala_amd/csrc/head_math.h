// The per-lane loss arithmetic of the fused head (head.h) and of the standalone loss-head kernels
// (kernels.h): the V-trace lane and its gradient, the PPO clipped-surrogate term.  Device inline
// functions only, so a translation unit that instantiates head_step_kernel alone need not take
// kernels.h's kernels with it.
#pragma once
#include "common.h"
#include "net.h"

using namespace net;

// =========================================================================================
// V-trace (rlax/rlego vtrace_td_error_and_advantage as called through
// agents/impala/learning.py:15-26,150-153), one lane per (trajectory, t) of a wavefront segment
// of S lanes, L = T - 1 live lanes.
//
// Forward order.  Every operation rounds once, in the order of the fp32 restatement
// (oracle/vtrace.py: td = rho' * ((r + g v_t) - v_tm1); acc = td + (g c) * acc; target = acc +
// v_tm1; ...): floating-point contraction is off in these functions, so on identical inputs the
// outputs are bit-identical to the sequential fp32 loop.  The reverse recurrence
// e_t = b_t + a_t e_{t+1} runs as L sweeps over the segment, each lane recomputing its e from
// its neighbour's value of the previous sweep (DPP wave shift): after sweep k the lanes
// t >= L - k hold their final value, computed from the final e_{t+1} -- the sequential loop's
// own operations, so its own rounding (a log-depth composition of the affine maps would sum in
// tree order instead).  L <= 63 sweeps of 3 VALU operations.
//
// Return order (pg_advantage, td_error, q_estimate): taken from the reference's unpacking
// `adv, err, _ =` (learning.py:150); rlax's published VTraceOutput lists (errors,
// pg_advantage, q_estimate).  rlego itself is absent, so this order is an unpinned assumption
// pinned only by the reference's own call sites.
//
// Gradient semantics (IMPALA_VTRACE_SG_*, include/impala_hip.h).  learning.py:148-155 detaches
// neither rho nor the advantage; what is constant depends on rlego:
//   SG_ADVANTAGE (0)  targets and pg advantages constant (the IMPALA paper's estimator)
//   SG_TARGETS   (1)  rlax stop_target_gradients=True: targets constant, the advantage
//                     rho_pg (q - v_tm1) live -- through min(rho_pg, rho) into log pi(a), into
//                     v_tm1 and, via q's bootstrap, into v_t[L-1] ((1 - lambda) v_tm1[t+1])
//   SG_NONE      (2)  stop_target_gradients=False: also through the targets, i.e. the scan
// =========================================================================================
enum : int { VT_SG_ADVANTAGE = 0, VT_SG_TARGETS = 1, VT_SG_NONE = 2 };

DEV float seq_rev_scan(float a, float b, int t, int L) {
#pragma clang fp contract(off)
  const bool live = t < L, nxt = t + 1 < L;
  float e = 0.f;
  for (int k = 0; k < L; ++k) {
    const float en = shift_down1(e);
    e = live ? b + a * (nxt ? en : 0.f) : 0.f;
  }
  return e;
}
// the adjoint of seq_rev_scan: E_t = b_t + a_{t-1} E_{t-1}, E_0 = b_0 (forward in t)
DEV float seq_fwd_scan(float a, float b, int t, int L) {
  const bool live = t < L, prv = t >= 1;
  float E = 0.f;
  for (int k = 0; k < L; ++k) {
    const float p = shift_up1(a * E);
    E = live ? b + (prv ? p : 0.f) : 0.f;
  }
  return E;
}

struct VtLane {
  float a, td, e, tgt, err, q, adv;
};
// v = v_tm1[t], vt = v_t[t], vnx = v_tm1[t + 1] (only read for t < L - 1); lanes t >= L
// produce zeros.  In the learner v_t = values[:, 1:], so vt == vnx == the next lane's v.
DEV VtLane vtrace_lane(float v, float vt, float vnx, float r, float g, float rho, int t, int L,
                       float lam, float crho, float cpg) {
#pragma clang fp contract(off)
  const bool in = t < L;
  VtLane o;
  o.td = in ? fminf(crho, rho) * (r + g * vt - v) : 0.f;
  o.a = in ? g * (fminf(1.f, rho) * lam) : 0.f;
  o.e = seq_rev_scan(o.a, o.td, t, L);
  o.tgt = o.e + v;
  o.err = o.tgt - v;
  const float tgt_n = shift_down1(o.tgt);
  const float boot = (t < L - 1) ? lam * tgt_n + (1.f - lam) * vnx : vt;
  o.q = r + g * boot;
  o.adv = fminf(cpg, rho) * (o.q - v);
  return o;
}

// d loss / d log pi(a_t) and d loss / d v_t of the lane's frame t (t = 0 .. L, the last frame
// only through the bootstrap) for
//   loss = -c_pg sum_t log pi(a_t) adv_t + c_pg sum_t err_t^2 + (entropy term, elsewhere),
// c_pg = 1 / (B (T - 1)) (learning.py:155-159).  Every lane of the wavefront calls it.
struct VtGrad {
  float dlogpa, dv;
};
DEV VtGrad vtrace_grad_lane(const VtLane& o, int mode, float v, float vt, float r, float g,
                            float rho, float logpa, int t, int L, float lam, float crho,
                            float cpg, float c_pg) {
  const bool in = t < L;
  VtGrad d;
  d.dlogpa = in ? -c_pg * o.adv : 0.f;
  float dv = 0.f, dv_nx = 0.f, rbar = 0.f;  // -> v_t, -> v_{t+1}, -> rho_t
  if (mode != VT_SG_NONE) dv = in ? -2.f * c_pg * o.err : 0.f;  // err = sg(target) - v
  if (mode != VT_SG_ADVANTAGE) {
    const float abar = in ? -c_pg * logpa : 0.f;  // d loss / d adv_t
    const float qbar = fminf(cpg, rho) * abar;    // d loss / d q_t
    if (rho <= cpg) rbar += abar * (o.q - v);     // adv = min(cpg, rho) (q - v)
    dv -= qbar;
    dv_nx += (t < L - 1) ? (1.f - lam) * g * qbar : g * qbar;  // q's bootstrap
    if (mode == VT_SG_NONE) {
      // target_t = e_t + v_t enters err_t (whose own -v_t cancels target's +v_t) and q_{t-1}
      const float tq = shift_up1((t < L - 1) ? lam * g * qbar : 0.f);  // from q_{t-1}
      dv += (in && t >= 1) ? tq : 0.f;
      const float ebar = in ? 2.f * c_pg * o.err + (t >= 1 ? tq : 0.f) : 0.f;
      const float E = seq_fwd_scan(o.a, ebar, t, L);  // total adjoint of e_t
      // e_t = td_t + a_t e_{t+1};  td_t = min(crho, rho) (r + g v_{t+1} - v_t);
      // a_t = g min(1, rho) lambda
      const float rc = fminf(crho, rho);
      dv -= rc * E;
      dv_nx += rc * g * E;
      if (rho <= crho) rbar += E * (r + g * vt - v);
      const float e_n = shift_down1(o.e);
      if (rho <= 1.f) rbar += E * ((t + 1 < L) ? e_n : 0.f) * g * lam;
    }
    d.dlogpa += in ? rbar * rho : 0.f;  // rho = exp(log pi(a) - log mu(a))
  }
  const float from_prev = shift_up1(in ? dv_nx : 0.f);
  d.dv = (in ? dv : 0.f) + (t >= 1 && t <= L ? from_prev : 0.f);
  return d;
}

// =========================================================================================
// PPO clipped surrogate (losses.py:131-155), per transition:
//   ratio r = exp(log pi(a) - log pi_ref(a)),  adv = v_target - v
//   pg_l = max(-adv r, -clamp(r, 1-eps, 1+eps) adv),  loss = mean(pg_l) + 0.5 mean(adv^2)
//                                                           - c_ent mean(H(pi))
// adv is detached in pg_l.  d pg_l / d r = -adv w, w = 1 where the unclipped term is the max,
// clamp'(r) (1 inside [lo, hi], bounds included, else 0) where the clipped term is, and their
// mean on a tie (torch.max splits the gradient evenly between equal inputs).
// =========================================================================================
struct PpoFrame {
  float adv, pgl, dr;  // advantage, surrogate term, d pg_l / d r
};
DEV PpoFrame ppo_frame(float r, float v, float tgt, float lo, float hi) {
  const float adv = tgt - v;
  const float l1 = -adv * r, l2 = -fminf(fmaxf(r, lo), hi) * adv;
  const float inside = (r >= lo && r <= hi) ? 1.f : 0.f;
  const float w = l1 > l2 ? 1.f : (l1 < l2 ? inside : 0.5f * (1.f + inside));
  return PpoFrame{adv, fmaxf(l1, l2), -adv * w};
}
