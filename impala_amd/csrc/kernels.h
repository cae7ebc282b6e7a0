// Non-GEMM kernels of the learner step: fused log-softmax / V-trace / loss head, LayerNorm
// forward and backward, gradient-slab reduction, global-norm clip + Adam, weight repacking.
#pragma once
#include "adam.h"
#include "common.h"
#include "conv1.h"
#include "net.h"
#include "ops.h"

using namespace net;

// (the V-trace lane, its gradient and the PPO surrogate term: head_math.h)
#include "head_math.h"

// Standalone batched V-trace on [B][L] inputs (impala_vtrace).
__global__ __launch_bounds__(256) void vtrace_kernel(const float* __restrict__ v_tm1,
                                                     const float* __restrict__ v_t,
                                                     const float* __restrict__ r_t,
                                                     const float* __restrict__ g_t,
                                                     const float* __restrict__ rho_t, int B,
                                                     int L, int S, float lam, float crho,
                                                     float cpg, float* __restrict__ adv,
                                                     float* __restrict__ err,
                                                     float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int traj = gw * (64 / S) + lane / S;
  const int t = lane % S;
  const bool in = traj < B && t < L;
  const size_t i = (size_t)traj * L + t;
  const float v = in ? v_tm1[i] : 0.f, vt = in ? v_t[i] : 0.f, r = in ? r_t[i] : 0.f,
              g = in ? g_t[i] : 0.f, rho = in ? rho_t[i] : 0.f;
  const VtLane o = vtrace_lane(v, vt, shift_down1(v), r, g, rho, in ? t : L, L, lam, crho, cpg);
  if (in) {
    err[i] = o.err;
    q[i] = o.q;
    adv[i] = o.adv;
  }
}

// =========================================================================================
// Fused loss head (agents/impala/learning.py:144-170): per (b,t) lane: log-softmax of the
// policy and behaviour logits, log pi(a), rho, entropy, KL; per trajectory: V-trace scan over
// T-1 (the last step is dropped from pg/value, kept for entropy/KL/ratio, learning.py:150-157);
// analytic d loss / d logits and d loss / d value under the V-trace gradient mode vt_mode
// (VT_SG_*, vtrace_grad_lane):
//   loss = -mean_{B,T-1}(log pi(a) adv) + mean_{B,T-1}(err^2) - c_ent * mean_{B,T} H(pi)
//   dlogit_j = c_ent/(BT) pi_j (log pi_j + H)  +  kappa_t (1[j=a] - pi_j),
//   kappa_t = d loss / d log pi(a_t)  (= -[t<T-1] adv/(B(T-1)) with the advantage constant)
// Per-workgroup partial sums of (log pi(a) adv, err^2, H, KL, rho) go to `partials`.
// =========================================================================================
struct LossArgs {
  const float* logits; int lg_ld;
  const float* values; int v_ld;
  const int64_t* act; const float* rew; const float* disc; const float* mu;
  int B, T, A, S, vt_mode;
  float lam, crho, cpg, ent_coef;
  float* partials;  // [gridDim.x][8]
  float* dbg_adv; float* dbg_err; float* dbg_q; float* dbg_rho;
};

template <typename TO>
__global__ __launch_bounds__(256) void loss_head_kernel(const LossArgs a, TO* __restrict__ dl,
                                                        int dl_ld, TO* __restrict__ dv,
                                                        int dv_ld, int zero_to) {
  __shared__ float red[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * 4 + wave;
  const int S = a.S, T = a.T, A = a.A, L = T - 1;
  const int traj = gw * (64 / S) + lane / S;
  const int t = lane % S;
  const bool valid = traj < a.B && t < T;
  const bool inL = valid && t < L;
  const size_t n = (size_t)(valid ? traj : 0) * T + (valid ? t : 0);

  float lg[MAX_A], logp[MAX_A];
  float H = 0.f, kl = 0.f, logpa = 0.f, rho = 0.f, v = 0.f, r = 0.f, g = 0.f;
  int act = 0;
  if (valid) {
    // all loads are issued unconditionally (clamped index) and masked afterwards: a
    // "load or constant" select per element would make the compiler wait on each load
    float m = -INFINITY, mu[MAX_A];
    const float* lrow = a.logits + n * a.lg_ld;
    const float* mrow = a.mu + n * A;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) {
      const int jj = j < A ? j : A - 1;
      lg[j] = lrow[jj];
      mu[j] = mrow[jj];
    }
    act = (int)a.act[n];
    v = a.values[n * a.v_ld];
    r = a.rew[n];
    g = a.disc[n];
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) {
      if (j >= A) lg[j] = -INFINITY;
      m = fmaxf(m, lg[j]);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) s += j < A ? expf(lg[j] - m) : 0.f;
    const float lse = m + logf(s);
    float mm = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) {
      if (j >= A) mu[j] = -INFINITY;
      mm = fmaxf(mm, mu[j]);
    }
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) sm += j < A ? expf(mu[j] - mm) : 0.f;
    const float lse_mu = mm + logf(sm);
    float logmua = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) {
      if (j < A) {
        logp[j] = lg[j] - lse;
        const float p = expf(logp[j]);
        const float lmu = mu[j] - lse_mu;
        H -= p * logp[j];
        kl += p * (logp[j] - lmu);
        if (j == act) { logpa = logp[j]; logmua = lmu; }
      } else {
        logp[j] = 0.f;
      }
    }
    rho = expf(logpa - logmua);
  }
  // ---- V-trace over the first T-1 steps of each trajectory segment ----
  const int tv = valid ? t : 64;     // lanes of missing trajectories are dead in the scans
  const float v_n = shift_down1(v);  // values[:, 1:]
  const VtLane o = vtrace_lane(v, v_n, v_n, r, g, rho, tv, L, a.lam, a.crho, a.cpg);
  const float err = o.err, qq = o.q, adv = o.adv;
  const float c_pg = 1.f / (float)(a.B * L), c_ent = 1.f / (float)(a.B * T);
  const VtGrad gr = vtrace_grad_lane(o, a.vt_mode, v, v_n, r, g, rho, logpa, tv, L, a.lam,
                                     a.crho, a.cpg, c_pg);

  if (valid) {
    const float ke = a.ent_coef * c_ent, kp = gr.dlogpa;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j) {
      if (j < A) {
        const float p = expf(logp[j]);
        const float d = ke * p * (logp[j] + H) + kp * ((j == act ? 1.f : 0.f) - p);
        dl[n * dl_ld + j] = (TO)d;
      } else if (j < zero_to) {
        dl[n * dl_ld + j] = (TO)0.f;
      }
    }
    dv[n * dv_ld] = (TO)gr.dv;
    if (a.dbg_rho) a.dbg_rho[n] = rho;
    if (inL && a.dbg_adv) {
      const size_t k = (size_t)traj * L + t;
      a.dbg_adv[k] = adv;
      a.dbg_err[k] = err;
      a.dbg_q[k] = qq;
    }
  }
  float s0 = inL ? logpa * adv : 0.f, s1 = inL ? err * err : 0.f;
  float s2 = valid ? H : 0.f, s3 = valid ? kl : 0.f, s4 = valid ? rho : 0.f;
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; red[wave][4] = s4;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    a.partials[blockIdx.x * 8 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// metrics[0..5] = loss, entropy, td, pg, kl, ratio from the loss-head partial sums
// Sum the per-workgroup partials [nparts][8] (first K values) across one wavefront: lane l
// sums partials l, l + 64, ... in order, then a fixed butterfly over the lanes -- every lane
// ends with the same totals (a one-thread load-add loop would be one L2 round trip per partial).
template <int K>
DEV void sum_partials(const float* part, int nparts, int lane, float (&s)[K]) {
  for (int p = lane; p < nparts; p += 64) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(part + (size_t)p * 8);
    const f32x4 b = *reinterpret_cast<const f32x4*>(part + (size_t)p * 8 + 4);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += k < 4 ? a[k] : b[k - 4];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
}

// (called by a whole wavefront; lane 0 writes the metrics)
DEV void finalize_loss_metrics(const float* part, int nparts, int B, int T, float ent_coef,
                               float* metrics, int lane) {
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  sum_partials<5>(part, nparts, lane, s);
  if (lane != 0) return;
  const float c_pg = 1.f / (float)(B * (T - 1)), c_ent = 1.f / (float)(B * T);
  const float pg = s[0] * c_pg, td = s[1] * c_pg, ent = s[2] * c_ent;
  metrics[0] = -pg + td - ent_coef * ent;
  metrics[1] = ent;
  metrics[2] = td;
  metrics[3] = pg;
  metrics[4] = s[3] * c_ent;
  metrics[5] = s[4] * c_ent;
  metrics[8] = 0.f;  // (PPO's train/target slot) every slot is written each step
}

__global__ void finalize_loss_kernel(const float* part, int nparts, int B, int T, float ent_coef,
                                     float* metrics) {
  if (threadIdx.x < 64) finalize_loss_metrics(part, nparts, B, T, ent_coef, metrics, (int)threadIdx.x);
}

// metrics from PPO partial sums (pg_l, adv^2, H, KL, r, target): slots 0..5 as IMPALA
// (loss, entropy, td, pg, kl, ratio) and slot 8 = train/target; kl is clamp_min(0)'d
DEV void finalize_ppo_metrics(const float* part, int nparts, int N, float ent_coef,
                              float* metrics, int lane) {
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  sum_partials<6>(part, nparts, lane, s);
  if (lane != 0) return;
  const float c = 1.f / (float)N;
  const float pg = s[0] * c, td = 0.5f * (s[1] * c), ent = s[2] * c;
  metrics[0] = pg + td - ent_coef * ent;
  metrics[1] = ent;
  metrics[2] = td;
  metrics[3] = pg;
  metrics[4] = fmaxf(s[3] * c, 0.f);
  metrics[5] = s[4] * c;
  metrics[8] = s[5] * c;
}

// metrics from the DQN head's (dqn_head.h) partial sums (q[a], target, |err|, err^2 w): the reference's
// train_step/{q, target, priorities, loss}; the slots Adam does not write are zeroed.
// (called by a whole wavefront; lane 0 writes)
DEV void finalize_dqn_metrics(const float* part, int nparts, int N, float* metrics, int lane,
                              bool step_vector = true) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  sum_partials<4>(part, nparts, lane, s);
  if (lane != 0) return;
  const float c = 1.f / (float)N;
  metrics[0] = s[0] * c;
  metrics[1] = s[1] * c;
  metrics[2] = s[2] * c;
  metrics[3] = 0.5f * (s[3] * c);
  if (step_vector) metrics[4] = metrics[5] = metrics[8] = 0.f;
}
// Standalone PPO loss head on given outputs, one lane per transition (test / reuse entry).
__global__ __launch_bounds__(256) void ppo_loss_head_kernel(
    const float* __restrict__ logits, const float* __restrict__ values,
    const int64_t* __restrict__ act, const float* __restrict__ tgt,
    const float* __restrict__ mu, int N, int A, float ent_coef, float lo, float hi,
    float* __restrict__ dl, float* __restrict__ dv, float* __restrict__ partials) {
  __shared__ float red[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 256 + threadIdx.x;
  const bool valid = n0 < N;
  const int n = valid ? n0 : 0;
  float lg[MAX_A], mv[MAX_A], p[MAX_A], logp[MAX_A];
#pragma unroll
  for (int j = 0; j < MAX_A; ++j) {
    const int jj = j < A ? j : A - 1;
    lg[j] = logits[(size_t)n * A + jj];
    mv[j] = mu[(size_t)n * A + jj];
  }
  const int a = (int)act[n];
  const float v = values[n], t = tgt[n];
  float m = -INFINITY, mm = -INFINITY;
#pragma unroll
  for (int j = 0; j < MAX_A; ++j) {
    lg[j] = j < A ? lg[j] : -INFINITY;
    mv[j] = j < A ? mv[j] : -INFINITY;
    m = fmaxf(m, lg[j]);
    mm = fmaxf(mm, mv[j]);
  }
  float s = 0.f, sm = 0.f;
#pragma unroll
  for (int j = 0; j < MAX_A; ++j) {
    p[j] = j < A ? expf(lg[j] - m) : 0.f;
    s += p[j];
    sm += j < A ? expf(mv[j] - mm) : 0.f;
  }
  const float lse = m + logf(s), lse_mu = mm + logf(sm), inv_s = 1.f / s;
  float H = 0.f, kl = 0.f, logpa = 0.f, logmua = 0.f;
#pragma unroll
  for (int j = 0; j < MAX_A; ++j) {
    const bool on = j < A;
    logp[j] = on ? lg[j] - lse : 0.f;
    p[j] *= inv_s;
    const float lmu = on ? mv[j] - lse_mu : 0.f;
    H -= p[j] * logp[j];
    kl += p[j] * (logp[j] - lmu);
    logpa = j == a ? logp[j] : logpa;
    logmua = j == a ? lmu : logmua;
  }
  const float r = expf(logpa - logmua);
  const PpoFrame pf = ppo_frame(r, v, t, lo, hi);
  if (valid) {
    const float c = 1.f / (float)N, ke = ent_coef * c, kr = c * pf.dr * r;
#pragma unroll
    for (int j = 0; j < MAX_A; ++j)
      if (j < A) dl[(size_t)n * A + j] = ke * p[j] * (logp[j] + H) + kr * ((j == a ? 1.f : 0.f) - p[j]);
    dv[n] = -pf.adv * c;
  }
  float q[6] = {valid ? pf.pgl : 0.f, valid ? pf.adv * pf.adv : 0.f, valid ? H : 0.f,
                valid ? kl : 0.f, valid ? r : 0.f, valid ? t : 0.f};
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = wave_sum(q[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) red[wave][k] = q[k];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    partials[blockIdx.x * 8 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

__global__ void finalize_ppo_kernel(const float* part, int nparts, int N, float ent_coef,
                                    float* metrics9) {
  if (threadIdx.x < 64) finalize_ppo_metrics(part, nparts, N, ent_coef, metrics9, (int)threadIdx.x);
}


// (shadow-weight emission, write_shadow: adam.h)
template <typename T, int HID>
__global__ __launch_bounds__(256) void pack_params_kernel(const float* __restrict__ params,
                                                          ShadowPtrs sp, Canon cn, Shadow sh) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cn.total) write_shadow<T, HID>(sp, cn, sh, i, params[i]);
}

// =========================================================================================
// Gradient-slab reduction into the canonical (state_dict) gradient buffer.  Work is laid out
// in KERNEL order (slab-contiguous: one float4 per thread, coalesced across the wave, all
// splits summed in a fixed order -> deterministic); the canonical index of each element is
// computed on the write side.  Also: per-block sum of squares (clip norm), loss-metric
// finalisation and the Adam step counter increment (block 0).
// =========================================================================================
enum RedKind { RK_ID = 0, RK_CONV2, RK_CONV3, RK_LN, RK_FC, RK_HEADS_W, RK_HEADS_B, RK_CONV1 };
constexpr int MAX_RED_SEGS = 12;
struct RedSeg {
  const float* slab;  // [S][count]
  int S, count, kind;
  long long canon;    // canonical offset (for RK_LN: lng offset; lnb follows)
  int sg;             // split groups per workgroup (power of two, <= 16)
};
struct RedArgs {
  RedSeg seg[MAX_RED_SEGS];
  int wg_start[MAX_RED_SEGS + 1];  // first workgroup of each segment
  float* grads;
  Canon cn;
  float* sumsq_part;
  const float* loss_part;
  int n_loss_part, B, T, A;
  int algo;  // IMPALA_ALGO_*: which loss the partial sums belong to
  float ent_coef;
  float* metrics;
  int64_t* step;
  double lr, b1, b2;  // Adam bias corrections for the step this reduction completes
  float* adam_sc;     // [2]: lr / (1 - b1^t), sqrt(1 - b2^t)
};

template <int HID> DEV long long canon_index(const RedArgs& a, const RedSeg& sg, int k) {
  switch (sg.kind) {
    case RK_CONV1: {  // k = oc*192 + k' (s2d order)  ->  oc*192 + ci*64 + kh*8 + kw
      const int oc = k / K1;
      return sg.canon + oc * K1 + c1_canon_k(k - oc * K1);
    }
    case RK_CONV2: {  // k = oc*512 + tap*32 + ci  ->  oc*512 + ci*16 + tap
      const int oc = k >> 9, rem = k & 511, tap = rem >> 5, ci = rem & 31;
      return sg.canon + oc * K2 + ci * 16 + tap;
    }
    case RK_CONV3: {  // k = oc*576 + tap*64 + ci  ->  oc*576 + ci*9 + tap
      const int oc = k / K3, rem = k - oc * K3, tap = rem >> 6, ci = rem & 63;
      return sg.canon + oc * K3 + ci * 9 + tap;
    }
    case RK_LN: {  // k = which*1024 + p*64 + c  ->  lng/lnb + c*16 + p
      const int which = k >> 10, j = k & 1023, p = j >> 6, c = j & 63;
      return sg.canon + which * FLAT + c * 16 + p;
    }
    case RK_FC: {  // k = o*1024 + p*64 + c  ->  o*1024 + c*16 + p
      const int o = k >> 10, j = k & 1023, p = j >> 6, c = j & 63;
      return sg.canon + (long long)o * FLAT + c * 16 + p;
    }
    case RK_HEADS_W: {  // k = row*HID + j; rows 0..A-1 actor, row 15 critic, else padding
      const int row = k >> hid_log2<HID>(), j = k & (HID - 1);
      if (row < a.A) return (long long)a.cn.wa + row * HID + j;
      if (row == VCOL) return (long long)a.cn.wc + j;
      return -1;
    }
    case RK_HEADS_B: {
      if (k < a.A) return (long long)a.cn.ba + k;
      if (k == VCOL) return (long long)a.cn.bc;
      return -1;
    }
    default:
      return sg.canon + k;
  }
}

// Sum of splits grp, grp + SG, ... of one float4 column of a slab, in split order.  The loads
// are unconditional (split index clamped to S - 1) and out-of-range splits are dropped by a
// value select after them (a select, not a multiply by 0: an Inf in the clamped split must not
// become a NaN); a "load or zero" select per element compiles to a branch and a vmcnt(0) wait
// per load.
template <int R>
DEV f32x4 sum_splits(const float* p, int grp, int SG, int S, int count) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = grp; q < S; q += R * SG) {
    f32x4 v[R];
#pragma unroll
    for (int j = 0; j < R; ++j)
      v[j] = *reinterpret_cast<const f32x4*>(p + (size_t)min(q + j * SG, S - 1) * count);
#pragma unroll
    for (int j = 0; j < R; ++j) acc += q + j * SG < S ? v[j] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  return acc;
}

// the bias corrections of step t from the reduction's arguments (adam.h)
DEV void adam_scalars(const RedArgs& a, int64_t t, float& step_size, float& bc2s) {
  adam_step_scalars(a.lr, a.b1, a.b2, t, step_size, bc2s);
}

// One reduction unit = one workgroup of reduce_grads_kernel (global index `u`), on 256 threads
// (`tid`): reduce_unit_sum gives each thread the sum of its split group, which the caller puts
// in part[tid]; after a barrier reduce_unit_finish combines the SG split groups from LDS --
// threads of split group 0 whose column is in range get the 4 reduced values and their
// canonical indices (-1: padding / out of range) -- and returns the thread's sum of squares.
struct RedUnit {
  int s, SG, cols, col, grp, v4;
  bool in;
};
DEV RedUnit reduce_unit_at(const RedArgs& a, int u, int tid) {
  RedUnit r;
  r.s = 0;
  while (u >= a.wg_start[r.s + 1]) ++r.s;
  const RedSeg& sg = a.seg[r.s];
  r.SG = sg.sg;
  r.cols = 256 / r.SG;
  r.col = tid % r.cols;
  r.grp = tid / r.cols;
  r.v4 = (u - a.wg_start[r.s]) * r.cols + r.col;  // float4 index in the segment
  r.in = r.v4 * 4 < sg.count;
  return r;
}
DEV f32x4 reduce_unit_sum(const RedArgs& a, const RedUnit& r) {
  const RedSeg& sg = a.seg[r.s];
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (r.in) {
    // R split loads in flight per round, R = 8 or 16 by the splits this thread sums (one
    // round for every segment at the default split-group rule)
    const float* p = sg.slab + (size_t)r.v4 * 4;
    acc = (sg.S + r.SG - 1) / r.SG <= 8 ? sum_splits<8>(p, r.grp, r.SG, sg.S, sg.count)
                                        : sum_splits<16>(p, r.grp, r.SG, sg.S, sg.count);
  }
  return acc;
}
template <int HID>
DEV float reduce_unit_finish(const RedArgs& a, const RedUnit& r, const f32x4* part, f32x4& acc,
                             long long (&ci)[4]) {
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) ci[i] = -1;
  if (r.grp == 0 && r.in) {
    for (int g2 = 1; g2 < r.SG; ++g2) acc += part[g2 * r.cols + r.col];
    const int k = r.v4 * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ci[i] = canon_index<HID>(a, a.seg[r.s], k + i);
      if (ci[i] >= 0) sq += acc[i] * acc[i];
    }
  }
  return sq;
}
template <int HID>
DEV float reduce_unit(const RedArgs& a, int wg, f32x4* part, f32x4& acc, long long (&ci)[4]) {
  const RedUnit r = reduce_unit_at(a, wg, (int)threadIdx.x);
  acc = reduce_unit_sum(a, r);
  part[threadIdx.x] = acc;
  __syncthreads();
  return reduce_unit_finish<HID>(a, r, part, acc, ci);
}

// Each segment is processed by workgroups of 256 threads = (256/SG) float4 columns x SG
// split groups; split group g sums splits g, g+SG, ... and the SG partials are combined in
// LDS in a fixed order (deterministic for a given SG).  wg_start[] holds each segment's
// first workgroup.  One launch reduces segments [s_lo, s_hi) (grid = their workgroups), so
// each weight-gradient branch can be reduced as soon as its slab is complete; the workgroup's
// global index (wg_start[s_lo] + blockIdx.x) names its sum-of-squares partial, so the partial
// order -- and the norm -- does not depend on how the segments were grouped into launches.
template <int HID>
__global__ __launch_bounds__(256) void reduce_grads_kernel(const RedArgs a, int s_lo, int fin) {
  __shared__ f32x4 part[256];
  __shared__ float red[4];
  const int wg = a.wg_start[s_lo] + (int)blockIdx.x;
  f32x4 acc;
  long long ci[4];
  float sq = reduce_unit<HID>(a, wg, part, acc, ci);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (ci[i] >= 0) a.grads[ci[i]] = acc[i];
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) a.sumsq_part[wg] = red[0] + red[1] + red[2] + red[3];
  if (fin && blockIdx.x == 0 && (threadIdx.x >> 6) == 1) {  // wave 1
    if constexpr (HID == HID_DQN)  // (the 512-wide instantiation serves the DQN handle alone)
      finalize_dqn_metrics(a.loss_part, a.n_loss_part, a.B * a.T, a.metrics, threadIdx.x & 63);
    else if (a.algo == 1)
      finalize_ppo_metrics(a.loss_part, a.n_loss_part, a.B * a.T, a.ent_coef, a.metrics, threadIdx.x & 63);
    else
      finalize_loss_metrics(a.loss_part, a.n_loss_part, a.B, a.T, a.ent_coef, a.metrics, threadIdx.x & 63);
  }
  if (fin && blockIdx.x == 0 && threadIdx.x == 128) {  // step += 1 and its bias corrections
    const int64_t t = *a.step + 1;
    *a.step = t;
    adam_scalars(a, t, a.adam_sc[0], a.adam_sc[1]);
  }
}

// per-block sum of squares of an (all-reduced) gradient buffer
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n,
                                                    float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    acc += g[i] * g[i];
  const float q = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// clip + Adam + re-emission of the kernel-layout weights on buffers in Canon order (adam.h)
template <typename T, int HID>
__global__ __launch_bounds__(256) void adam_kernel(const AdamArgs a) {
  adam_body<T, HID>(a, FlatId{});
}

// heads output [n][16] -> logits [n][A], values [n]
__global__ void split_heads_kernel(const float* __restrict__ heads, int n, int A,
                                   float* __restrict__ logits, float* __restrict__ values) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * HEADS) return;
  const int f = i / HEADS, j = i % HEADS;
  if (j < A) logits[(size_t)f * A + j] = heads[i];
  else if (j == VCOL) values[f] = heads[i];
}

// Actor inference head (models/distributed_models.py:21-32 AtariPPOModel.act): one thread per
// frame splits the heads row into logits / value and picks the action -- argmax (first maximal
// index, as torch.argmax) where the frame's deterministic flag is set, else a draw from
// softmax(logits) by inverse CDF on a counter-based uniform (seed, counter, frame), the
// distribution torch's softmax(-1).multinomial(1) samples from.
// (the counter-based uniform's mixer is act_mix64, common.h)
__global__ __launch_bounds__(256) void act_heads_kernel(const float* __restrict__ heads, int n, int A,
                                                        const uint8_t* __restrict__ det, int det_all,
                                                        uint64_t seed, uint64_t counter,
                                                        int64_t* __restrict__ actions,
                                                        float* __restrict__ logits,
                                                        float* __restrict__ values) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  float l[HEADS];
#pragma unroll
  for (int j = 0; j < HEADS; j += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(heads + (size_t)f * HEADS + j);
    l[j] = x[0]; l[j + 1] = x[1]; l[j + 2] = x[2]; l[j + 3] = x[3];
  }
  values[f] = l[VCOL];
  float mx = l[0];
  int am = 0;
  for (int j = 0; j < A; ++j) {
    logits[(size_t)f * A + j] = l[j];
    if (l[j] > mx) { mx = l[j]; am = j; }
  }
  int a = am;
  if (!(det ? det[f] != 0 : det_all != 0)) {
    float sum = 0.f;
    for (int j = 0; j < A; ++j) sum += expf(l[j] - mx);
    const uint64_t r = act_mix64(act_mix64(seed ^ act_mix64(counter)) + (uint64_t)f);
    const float u = (float)(uint32_t)(r >> 40) * (1.f / 16777216.f) * sum;  // [0, sum)
    float c = 0.f;
    a = A - 1;
    for (int j = 0; j < A; ++j) {
      c += expf(l[j] - mx);
      if (u < c) { a = j; break; }
    }
  }
  actions[f] = a;
}

// =========================================================================================
// Replay gather: dst_f[i] = src_f[idx[i]] for up to 8 fields of fixed row size (bytes, multiple
// of 4).  One workgroup per (row, field); 16-byte vector copies for the aligned bulk.
// =========================================================================================
// A row is copied in pieces of GATHER_PIECE bytes, one workgroup per (field, row, piece), so a
// 245 KB obs row is spread over 15 workgroups.  Indices come from device memory (idx) or, for
// up to GATHER_HIDX rows, from the launch's own arguments (hidx: no index upload).
constexpr int GATHER_PIECE = 16384;
constexpr int GATHER_HIDX = 256;
static_assert(GATHER_PIECE % (16 * 256) == 0, "whole 16-byte vectors per thread");
struct GatherArgs {
  const char* src[8];
  char* dst[8];
  long long row_bytes[8];
  int pieces[8];     // pieces per row of each field
  int unit0[9];      // first workgroup of each field: unit0[f] + row * pieces[f] + piece
  int nfields;
  const int64_t* idx;
  int n;
  int hidx[GATHER_HIDX];
};

// Host -> HBM pull copy for the staging ring (impala_stage's four small fields): a few
// workgroups read page-locked host memory over PCIe with 4 x 16-byte loads in flight per lane
// (PCIe latency x bandwidth needs ~128 KB outstanding), on the copy stream beside the step.
struct PullArgs {
  const char* src[5];
  char* dst[5];
  long long bytes[5];
  int nf;
};
__global__ __launch_bounds__(1024) void h2d_pull_kernel(const PullArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (int f = 0; f < a.nf; ++f) {
    const long long nv = a.bytes[f] >> 4;
    const f32x4* s = reinterpret_cast<const f32x4*>(a.src[f]);
    f32x4* d = reinterpret_cast<f32x4*>(a.dst[f]);
    long long i = t;
    for (; i + 3 * stride < nv; i += 4 * stride) {
      const f32x4 v0 = __builtin_nontemporal_load(s + i), v1 = __builtin_nontemporal_load(s + i + stride);
      const f32x4 v2 = __builtin_nontemporal_load(s + i + 2 * stride);
      const f32x4 v3 = __builtin_nontemporal_load(s + i + 3 * stride);
      d[i] = v0;
      d[i + stride] = v1;
      d[i + 2 * stride] = v2;
      d[i + 3 * stride] = v3;
    }
    for (; i < nv; i += stride) d[i] = s[i];
    for (long long b = (nv << 4) + t; b < a.bytes[f]; b += stride) a.dst[f][b] = a.src[f][b];
  }
}

// Stands in for a learner step while impala_stage_init primes the copy path: one lane waits
// `ticks` of the 100 MHz real-time counter (bounded: at most 2^20 sleep rounds).
__global__ __launch_bounds__(64) void stage_prime_spin_kernel(long long ticks) {
  if (threadIdx.x != 0) return;
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < (1 << 20); ++i) {
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 >= ticks) break;
    __builtin_amdgcn_s_sleep(8);
  }
}

// the device step clock's closing stamp (impala_step_clock_end): one thread, one vector store
__global__ __launch_bounds__(64) void clock_stamp_kernel(unsigned long long* __restrict__ out) {
  if (threadIdx.x == 0) *out = __builtin_amdgcn_s_memrealtime();
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgs a) {
  const int u = blockIdx.x;
  int f = 0;
  while (f + 1 < a.nfields && u >= a.unit0[f + 1]) ++f;
  const int r = u - a.unit0[f];
  const int i = r / a.pieces[f], piece = r - i * a.pieces[f];
  if (f >= a.nfields || i >= a.n) return;
  const long long rb = a.row_bytes[f];
  const long long o0 = (long long)piece * GATHER_PIECE;
  const long long len = min((long long)GATHER_PIECE, rb - o0);
  const long long row = a.idx ? a.idx[i] : a.hidx[i];
  const char* s = a.src[f] + (size_t)row * rb + o0;
  char* d = a.dst[f] + (size_t)i * rb + o0;
  const bool al16 = ((((uintptr_t)s) | ((uintptr_t)d) | (uintptr_t)len) & 15) == 0;
  if (al16) {
    // every load of the piece issued before any store (a load-store pair per iteration waited
    // out one memory round trip each: source and destination may alias as far as the compiler
    // knows); the replay rows are read once (nontemporal)
    constexpr int NVT = GATHER_PIECE / 16 / 256;
    const int nv = (int)(len >> 4);
    const f32x4* s4 = reinterpret_cast<const f32x4*>(s);
    f32x4* d4 = reinterpret_cast<f32x4*>(d);
    f32x4 v[NVT];
#pragma unroll
    for (int k = 0; k < NVT; ++k) {
      const int e = (int)threadIdx.x + k * 256;
      if (e < nv) v[k] = __builtin_nontemporal_load(s4 + e);
    }
#pragma unroll
    for (int k = 0; k < NVT; ++k) {
      const int e = (int)threadIdx.x + k * 256;
      if (e < nv) d4[e] = v[k];
    }
  } else {
    const long long nw = len >> 2;
    for (long long v = threadIdx.x; v < nw; v += 256)
      reinterpret_cast<float*>(d)[v] = reinterpret_cast<const float*>(s)[v];
  }
}
