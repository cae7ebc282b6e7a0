// The IMPALA ResNet learner step's own kernels (included by resnet.hip inside its
// unnamed namespace, after resnet_bwd.h).  Between resnet_forward_train and the backward:
//   resnet_vtrace_head_kernel  heads [n][16] -> d loss / d logits, d loss / d values, straight into the
//                              buffers resnet_head_bwd_kernel reads, and a row of metric sums per
//                              trajectory.  One wave per trajectory, lane = t; no LDS, no atomics.
// behind the backward:
//   resnet_sumsq_kernel        the flat gradient's sum of squares, one partial per workgroup of a fixed grid
//   resnet_adam_kernel         every wave re-adds the partials (the same bits everywhere), then torch's
//                              clip coefficient and Adam on four parameters a thread, a scalar tail;
//                              workgroup 0 writes the metrics vector and advances the step count
// The flat order is uniform for Adam (no kernel-layout weights are written here: the handle's
// resnet_refresh_weights launches follow), so there is no segment table.
#pragma once
#include "head_math.h"

// head.h's exponential and logarithm (the hardware's v_exp_f32 / v_log_f32)
DEV float rs_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
DEV float rs_log(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }
// four sums of four terms each, as a quad of head.h's threads adds them (quad_sum's order)
DEV float sum_q4(const float (&q)[4]) { return (q[0] + q[1]) + (q[2] + q[3]); }

struct VtHeadArgs {
  const float* heads;  // [B T][16]: logits 0..A-1, the value at 15 (resnet_heads_kernel)
  const int64_t* act;
  const float *rew, *disc, *mu;
  int B, T, A, vt_mode;
  float lam, crho, cpg, ent_coef;
  float *dl, *dv;  // [B T][A], [B T]
  float* tpart;    // [B][RN_TPART]
  float* vt_dbg;   // or null: adv, err, q [3][B][T-1], then rho [B][T] (resnet_set_debug_vtrace)
};

// learning.py:144-170 on the heads of B trajectories: wave w of workgroup g takes trajectory 4 g + w,
// lane t its frame t.  A lane holds its frame's 64-byte head row (four 16-byte loads) and the A behaviour
// logits in registers: both log-softmaxes, log pi(a), rho, the entropy and the KL term are lane-local,
// summed in the order head.h's quads sum them.  The V-trace and its gradient are head_math.h's, lanes
// talking by DPP shifts.  Waves past B leave at once (a wave-uniform branch); lanes t >= T load frame
// T - 1 again, are masked to zeros and t = 64 (dead in the scans) before the first shift, and store nothing.
__global__ __launch_bounds__(256) void resnet_vtrace_head_kernel(const VtHeadArgs a) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= a.B) return;
  const int T = a.T, A = a.A, L = T - 1;
  const bool live = lane < T, inL = lane < L;
  const size_t n = (size_t)b * T + min(lane, T - 1);
  // ---- every load, unconditionally (clamped indices); the action as the low word of the int64
  const f32x4* hr = reinterpret_cast<const f32x4*>(a.heads + n * HEADS);
  const f32x4 hv[4] = {hr[0], hr[1], hr[2], hr[3]};
  float mu[HEADS];
#pragma unroll
  for (int j = 0; j < HEADS; ++j) mu[j] = a.mu[n * A + min(j, A - 1)];
  const int aa = min(max(reinterpret_cast<const int*>(a.act)[2 * n], 0), A - 1);
  float r = a.rew[n], g = a.disc[n];
  // ---- the frame's statistics
  float lg[HEADS], ex[HEADS], m = -INFINITY, mm = -INFINITY;
#pragma unroll
  for (int j = 0; j < HEADS; ++j) {
    lg[j] = hv[j >> 2][j & 3];
    if (j < A) {
      m = fmaxf(m, lg[j]);
      mm = fmaxf(mm, mu[j]);
    }
  }
  float qs[4], qm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    qs[q] = qm[q] = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * q + u;
      ex[j] = j < A ? rs_exp(lg[j] - m) : 0.f;
      qs[q] += ex[j];
      qm[q] += j < A ? rs_exp(mu[j] - mm) : 0.f;
    }
  }
  const float s = sum_q4(qs), sm = sum_q4(qm);
  const float lse = m + rs_log(s), lse_mu = mm + rs_log(sm), inv = 1.f / s;
  float p[MAX_A], logp[MAX_A], qh[4], qk[4], logpa = 0.f, logmua = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    qh[q] = qk[q] = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * q + u;
      if (j < MAX_A) {
        const float lmu = mu[j] - lse_mu;
        logp[j] = lg[j] - lse;
        p[j] = ex[j] * inv;
        if (j < A) {
          qh[q] -= p[j] * logp[j];
          qk[q] += p[j] * (logp[j] - lmu);
        }
        logpa = j == aa ? logp[j] : logpa;
        logmua = j == aa ? lmu : logmua;
      }
    }
  }
  float H = sum_q4(qh), kld = sum_q4(qk), rho = rs_exp(logpa - logmua), v = hv[3][3];
  if (!live) { H = 0.f; kld = 0.f; logpa = 0.f; rho = 0.f; v = 0.f; r = 0.f; g = 0.f; }
  // ---- V-trace over the first T - 1 frames, its gradient under the mode (every lane calls both)
  const int tv = live ? lane : 64;
  const float v_n = shift_down1(v);  // values[:, 1:]
  const VtLane o = vtrace_lane(v, v_n, v_n, r, g, rho, tv, L, a.lam, a.crho, a.cpg);
  const float c_pg = 1.f / (float)(a.B * L);
  const VtGrad gr = vtrace_grad_lane(o, a.vt_mode, v, v_n, r, g, rho, logpa, tv, L, a.lam, a.crho, a.cpg, c_pg);
  if (live) {
    // dlogit_j = ke p_j (log p_j + H) + kappa ([j == a] - p_j), ke = d(-ent_coef mean H) / d H
    const float ke = a.ent_coef * (1.f / (float)(a.B * T)), kappa = gr.dlogpa;
    float* dl = a.dl + n * A;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j)
      if (j < A) dl[j] = ke * p[j] * (logp[j] + H) + kappa * ((j == aa ? 1.f : 0.f) - p[j]);
    a.dv[n] = gr.dv;
    if (a.vt_dbg) {
      const size_t BL = (size_t)a.B * L, ob = (size_t)b * L + lane;
      if (inL) {
        a.vt_dbg[ob] = o.adv;
        a.vt_dbg[BL + ob] = o.err;
        a.vt_dbg[2 * BL + ob] = o.q;
      }
      a.vt_dbg[3 * BL + n] = rho;
    }
  }
  // ---- the trajectory's metric sums, the lanes in wave_sum's order
  const float s0 = wave_sum(inL ? logpa * o.adv : 0.f), s1 = wave_sum(inL ? o.err * o.err : 0.f);
  const float s2 = wave_sum(H), s3 = wave_sum(kld), s4 = wave_sum(rho);
  if (lane == 0) {
    f32x4* tp = reinterpret_cast<f32x4*>(a.tpart + (size_t)b * RN_TPART);
    tp[0] = f32x4{s0, s1, s2, s3};
    tp[1] = f32x4{s4, 0.f, 0.f, 0.f};
  }
}

// Sum of squares of grad [n]: workgroup w takes the w-th of RN_SUMSQ_WGS equal contiguous slices of the
// buffer's 16-byte vectors, a thread every 256th vector of the slice; the last workgroup's thread 0 also
// takes the n % 4 floats behind the last whole vector.  Lanes by wave_sum, then the four waves in order.
// Workgroup 0 also forms the bias corrections of the step under way, t = step + 1 (adam.h's
// adam_step_scalars: torch's python doubles, rounded to fp32 once).
__global__ __launch_bounds__(256) void resnet_sumsq_kernel(const float* __restrict__ grad, int n, float* __restrict__ part,
                                                           const int64_t* __restrict__ step, float* __restrict__ sc,
                                                           double lr, double b1, double b2) {
  __shared__ float red[4];
  const int nv = n >> 2, per = (nv + RN_SUMSQ_WGS - 1) / RN_SUMSQ_WGS;
  const int lo = blockIdx.x * per, hi = min(lo + per, nv);
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const f32x4 x = reinterpret_cast<const f32x4*>(grad)[i];
    acc += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
  }
  if (blockIdx.x == RN_SUMSQ_WGS - 1 && threadIdx.x == 0)
    for (int i = 4 * nv; i < n; ++i) acc += grad[i] * grad[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if (blockIdx.x == 0 && threadIdx.x == 64) {
    const double t = (double)(step[0] + 1);
    sc[0] = (float)(lr / (1.0 - pow(b1, t)));
    sc[1] = (float)sqrt(1.0 - pow(b2, t));
  }
}

struct RsAdamArgs {
  float *params, *grads, *m, *v, *metrics;
  const float *sqpart, *sc, *tpart;
  int64_t* step;
  int n, B, T;
  double b1, b2;
  float eps, max_norm, ent_coef;
};

// clip_grad_norm_(max_norm) and torch.optim.Adam (no weight decay, no amsgrad) on the flat buffers: thread
// i of the grid takes the 16-byte vector i, thread n / 4 the n % 4 floats behind the last one.  Every
// wave adds the RN_SUMSQ_WGS partial sums itself -- lane l < 32 the four of vector l, the lanes by
// wave_sum: one order, so one norm for the whole grid with no launch between -- and forms torch's
// coefficient min(1, max_norm / (norm + 1e-6)).  grads is left clipped, as p.grad is.  An element's
// update is adam.h's adam_elem term for term (lerp form of exp_avg, sqrt(v) / sqrt(bc2) + eps; every
// operation rounded on its own).
// Wave 0 of workgroup 0: the IMPALA_M_* vector from the trajectories' sums (kernels.h's
// finalize_loss_metrics: lane l adds trajectories l, l + 64, .. in order, then the lanes), the norm and
// the step; it alone reads and writes the step count here (the bias corrections come from sc).
__global__ __launch_bounds__(256) void resnet_adam_kernel(const RsAdamArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, nv = a.n >> 2, i = blockIdx.x * 256 + threadIdx.x;
  const int cnt = i < nv ? 4 : i == nv ? (a.n & 3) : 0;
  const size_t i0 = (size_t)4 * i;
  float g[4], m[4], v[4], p[4];
  if (cnt == 4) {
    const f32x4 G = *reinterpret_cast<const f32x4*>(a.grads + i0), M = *reinterpret_cast<const f32x4*>(a.m + i0);
    const f32x4 V = *reinterpret_cast<const f32x4*>(a.v + i0), P = *reinterpret_cast<const f32x4*>(a.params + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { g[k] = G[k]; m[k] = M[k]; v[k] = V[k]; p[k] = P[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = k < cnt;
      g[k] = ok ? a.grads[i0 + k] : 0.f; m[k] = ok ? a.m[i0 + k] : 0.f;
      v[k] = ok ? a.v[i0 + k] : 0.f;     p[k] = ok ? a.params[i0 + k] : 0.f;
    }
  }
  const float step_size = a.sc[0], bc2s = a.sc[1];
  const f32x4 q = *reinterpret_cast<const f32x4*>(a.sqpart + 4 * (lane & 31));
  static_assert(RN_SUMSQ_WGS == 128, "32 lanes x one vector of partials");
  const float norm = sqrtf(wave_sum(lane < 32 ? (q[0] + q[1]) + (q[2] + q[3]) : 0.f));
  const float coef = fminf(a.max_norm / (norm + 1e-6f), 1.f);
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = lane; b < a.B; b += 64) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a.tpart + (size_t)b * RN_TPART);
      s[0] += x[0]; s[1] += x[1]; s[2] += x[2]; s[3] += x[3];
      s[4] += a.tpart[(size_t)b * RN_TPART + 4];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
      const float c_pg = 1.f / (float)(a.B * (a.T - 1)), c_ent = 1.f / (float)(a.B * a.T);
      const float pg = s[0] * c_pg, td = s[1] * c_pg, ent = s[2] * c_ent;
      const int64_t t = a.step[0] + 1;
      a.metrics[IMPALA_M_LOSS] = -pg + td - a.ent_coef * ent;
      a.metrics[IMPALA_M_ENTROPY] = ent;
      a.metrics[IMPALA_M_TD] = td;
      a.metrics[IMPALA_M_PG] = pg;
      a.metrics[IMPALA_M_KL] = s[3] * c_ent;
      a.metrics[IMPALA_M_RATIO] = s[4] * c_ent;
      a.metrics[IMPALA_M_GRAD_NORM] = norm;
      a.metrics[IMPALA_M_STEP] = (float)t;
      a.metrics[IMPALA_M_TARGET] = 0.f;
      a.step[0] = t;
    }
  }
  if (cnt == 0) return;
  const float w1 = (float)(1.0 - a.b1), b2f = (float)a.b2, w2 = (float)(1.0 - a.b2);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g[k] = g[k] * coef;
    m[k] = m[k] + w1 * (g[k] - m[k]);
    v[k] = v[k] * b2f + w2 * g[k] * g[k];
    const float denom = sqrtf(v[k]) / bc2s + a.eps;
    p[k] = p[k] - step_size * (m[k] / denom);
  }
  if (cnt == 4) {
    *reinterpret_cast<f32x4*>(a.grads + i0) = f32x4{g[0], g[1], g[2], g[3]};
    *reinterpret_cast<f32x4*>(a.m + i0) = f32x4{m[0], m[1], m[2], m[3]};
    *reinterpret_cast<f32x4*>(a.v + i0) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(a.params + i0) = f32x4{p[0], p[1], p[2], p[3]};
  } else {
    for (int k = 0; k < cnt; ++k) {
      a.grads[i0 + k] = g[k]; a.m[i0 + k] = m[k]; a.v[i0 + k] = v[k]; a.params[i0 + k] = p[k];
    }
  }
}
