// Kernels of the distributional (IQN) Ape-X agent (include/iqn_hip.h) -- the actor path and, further
// down, the learner's training step -- and their launchers (csrc/iqn_launch.h).  A translation unit
// of its own, so the code object of impala.hip -- the learner steps' kernels and where they sit in
// it -- is the same with or without it; the host side is csrc/iqn.h, included at the end of impala.hip.
//
// One forward of R = n W rows (row r = f W + k) after the conv trunk wrote act3 [n][1024]:
//   iqn_embed_ln_kernel  16 rows per workgroup.  The cosine tile e[16][64] = cos((pi i) tau_r) is
//                        computed into LDS; Wq e (K = 64) runs on the MFMAs with the tile as the B
//                        operand held in registers and Wq's rows read straight from L2 (every
//                        workgroup streams all of Wq: 256 KB fp32, 128 KB bf16); bias, GELU and the
//                        product with act3[f] in fp32; two-pass LayerNorm statistics in fp32 (row
//                        sums over the lanes' 4 row groups by permlane swaps, over the 4 waves
//                        through LDS, in a fixed order); y stored in T at the trunk's YLD pitch.
//   FcFwd / HeadsFwd     the dueling net's own functors (ops.h) over R rows
//   iqn_q_kernel         heads [R][16] -> q [R][A]
// Rows of one frame are consecutive, so a 16-row tile may span frames (W = 8) or half of one
// (W = 32); rows >= R are clamped on load and masked on store.
#include "common.h"

#include "../../include/iqn_hip.h"
#include "adam.h"
#include "dqn_head_step.h"
#include "iqn_launch.h"
#include "lnc3.h"
#include "ops.h"

namespace {

constexpr int IQN_TILE = 16;  // rows per workgroup of iqn_embed_ln_kernel
constexpr int NCOS = IQN_COS;

template <typename T>
__global__ __launch_bounds__(256) void iqn_pack_kernel(const float* __restrict__ src, T* __restrict__ wq,
                                                       float* __restrict__ bq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < FLAT * NCOS) {
    const int j = i >> 6, k = i & 63;
    wq[((j & 15) * OC3 + (j >> 4)) * NCOS + k] = (T)src[i];
  } else if (i < FLAT * NCOS + FLAT) {
    const int j = i - FLAT * NCOS;
    bq[(j & 15) * OC3 + (j >> 4)] = src[i];
  }
}

__global__ __launch_bounds__(256) void iqn_tau_kernel(uint64_t seed, uint64_t counter, int which, int R,
                                                      float* __restrict__ taus) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const uint64_t x = act_mix64(act_mix64(seed ^ act_mix64(counter)) + ((uint64_t)(1 + which) << 32) + (uint64_t)r);
  taus[r] = (float)(uint32_t)(x >> 40) * (1.f / 16777216.f);  // [0, 1)
}

// pre-activation tile of the quantile layer: rows j0 .. j0 + 15 of Wq against the cosine fragments b
// (K = 64); the training step's backward recomputes it with the same instructions
template <typename T, int NK>
DEV f32x4 iqn_wq_tile(const T* __restrict__ wq, int j0, int col, int kl, const typename Frag<T>::vec (&b)[NK]) {
  using F = Frag<T>;
  const T* arow = wq + (size_t)(j0 + col) * NCOS;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NK; ++s) acc = F::mma(F::load(arow + s * F::KSTEP + kl), b[s], acc);
  return acc;
}

// TRAIN: also keeps what the backward reads per row -- the LayerNorm statistics (mean, rstd) and
// the cosine tile in T, e [R][64] -- and recomputes the rest (iqn_ln_mod_bwd_kernel)
template <typename T, bool TRAIN>
DEV void iqn_embed_ln_body(const float* __restrict__ taus, const T* __restrict__ act3, const T* __restrict__ wq,
                           const float* __restrict__ bq, const float* __restrict__ gam,
                           const float* __restrict__ bet, T* __restrict__ y, int R, int W,
                           float* __restrict__ stats, T* __restrict__ e_out) {
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int LDE = NCOS + 16 / (int)sizeof(T);  // tile row (elements): rows stay 16-byte aligned
  constexpr int NK = NCOS / F::KSTEP;
  constexpr int TPW = FLAT / 16 / 4;  // 16-feature tiles per wave
  __shared__ __attribute__((aligned(16))) T es[IQN_TILE * LDE];
  __shared__ float red[2][4][IQN_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * IQN_TILE;
  {  // the cosine tile: thread -> row tid >> 4, features 4 (tid & 15) .. + 3
    const int rr = tid >> 4, i0 = (tid & 15) * 4;
    const float tau = taus[min(r0 + rr, R - 1)];
    T c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // torch's order for torch.pi * embedding_range * tau: (fl(pi) * i) * tau, two roundings
      const float pi_i = 3.14159274101257324f * (float)(i0 + q + 1);
      c[q] = (T)cosf(pi_i * tau);
      es[rr * LDE + i0 + q] = c[q];
    }
    if constexpr (TRAIN)  // the same four T values, copied as they are
      if (r0 + rr < R) {
        T* eo = e_out + (size_t)(r0 + rr) * NCOS + i0;
#pragma unroll
        for (int q = 0; q < 4; ++q) eo[q] = c[q];
      }
  }
  __syncthreads();
  const int col = lane & 15, grp = lane >> 4, kl = F::KPL * grp;
  V b[NK];
#pragma unroll
  for (int s = 0; s < NK; ++s) b[s] = *reinterpret_cast<const V*>(es + col * LDE + s * F::KSTEP + kl);
  const int r = min(r0 + col, R - 1);
  const T* xrow = act3 + (size_t)(r / W) * FLAT;
  float z[TPW][4];
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int j0 = (wave * TPW + t) * 16;
    const f32x4 acc = iqn_wq_tile<T, NK>(wq, j0, col, kl, b);
    const int j = j0 + 4 * grp;
    float x[4], bb[4];
    load4(xrow + j, x);
    load4(bq + j, bb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pre = acc[e] + bb[e];
      const float phi = 0.5f * pre * (1.f + erff(pre * 0.70710678118654752440f));
      z[t][e] = x[e] * phi;
      sum += z[t][e];
    }
  }
  // row statistics: this lane's row is col; its 1024 features lie on 4 row groups x 4 waves
  sum = xor32_sum(xor16_sum(sum));
  if (grp == 0) red[0][wave][col] = sum;
  __syncthreads();
  const float mean = (((red[0][0][col] + red[0][1][col]) + red[0][2][col]) + red[0][3][col]) * (1.f / FLAT);
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      z[t][e] -= mean;
      sq += z[t][e] * z[t][e];
    }
  sq = xor32_sum(xor16_sum(sq));
  if (grp == 0) red[1][wave][col] = sq;
  __syncthreads();
  const float var = (((red[1][0][col] + red[1][1][col]) + red[1][2][col]) + red[1][3][col]) * (1.f / FLAT);
  const float rstd = 1.f / sqrtf(var + LN_EPS);
  if (r0 + col >= R) return;
  if constexpr (TRAIN)
    if (wave == 0 && grp == 0) {
      stats[2 * r] = mean;
      stats[2 * r + 1] = rstd;
    }
  T* yrow = y + (size_t)r * YLD;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int j = (wave * TPW + t) * 16 + 4 * grp;
    float g[4], be[4], o[4];
    load4(gam + j, g);
    load4(bet + j, be);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = z[t][e] * rstd * g[e] + be[e];
    store4(yrow + j, o);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void iqn_embed_ln_kernel(const float* __restrict__ taus,
                                                           const T* __restrict__ act3, const T* __restrict__ wq,
                                                           const float* __restrict__ bq,
                                                           const float* __restrict__ gam,
                                                           const float* __restrict__ bet, T* __restrict__ y, int R,
                                                           int W) {
  iqn_embed_ln_body<T, false>(taus, act3, wq, bq, gam, bet, y, R, W, nullptr, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void iqn_embed_ln_train_kernel(
    const float* __restrict__ taus, const T* __restrict__ act3, const T* __restrict__ wq,
    const float* __restrict__ bq, const float* __restrict__ gam, const float* __restrict__ bet,
    T* __restrict__ y, int R, int W, float* __restrict__ stats, T* __restrict__ e_out) {
  iqn_embed_ln_body<T, true>(taus, act3, wq, bq, gam, bet, y, R, W, stats, e_out);
}

// heads output [R][16] (adv rows, v at 15) -> q [R][A]
__global__ __launch_bounds__(256) void iqn_q_kernel(const float* __restrict__ heads, int R, int A,
                                                    float* __restrict__ q) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float l[HEADS];
#pragma unroll
  for (int j = 0; j < HEADS; j += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(heads + (size_t)r * HEADS + j);
    l[j] = x[0]; l[j + 1] = x[1]; l[j + 2] = x[2]; l[j + 3] = x[3];
  }
  float s = 0.f;
  for (int k = 0; k < A; ++k) s += l[k];
  const float mean = s / (float)A;
  for (int k = 0; k < A; ++k) q[(size_t)r * A + k] = (l[VCOL] + l[k]) - mean;
}

// DistributionalAtariDQN.act (models/distributed_models.py:47-66), one wave per frame (four frames
// per workgroup), on the two nets' q [n][W][A]: lane a < A sums q_online[f][k][a] over k = 0..W-1 in
// order (the lanes read a row of A together) and divides by W: qbar.  Through LDS every lane then
// holds all of qbar and repeats what dqn_act_kernel does per frame: greedy = argmax qbar (first
// maximal index), the action drawn by inverse CDF on the counter-based uniform keyed by
// (seed, counter, frame), q_pi = qbar[action]; lane k < W stores q_star[k] = q_target[k][greedy].
// Frames >= n are clamped on load and masked on store.  A >= 2, W <= 64.
__global__ __launch_bounds__(256) void iqn_act_kernel(const float* __restrict__ q_on, const float* __restrict__ q_tg,
                                                      int n, int W, int A, const float* __restrict__ eps_f,
                                                      float eps_all, uint64_t seed, uint64_t counter,
                                                      int64_t* __restrict__ actions, float* __restrict__ q_pi,
                                                      float* __restrict__ q_star, int64_t* __restrict__ greedy_out) {
  __shared__ float qbs[4][HEADS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.x * 4 + wave;
  const bool valid = f0 < n;
  const int f = valid ? f0 : n - 1;
  const float* qo = q_on + (size_t)f * W * A + min(lane, A - 1);
  float s = 0.f;
#pragma unroll 8
  for (int k = 0; k < W; ++k) s += qo[k * A];
  if (lane < HEADS) qbs[wave][lane] = s / (float)W;
  __syncthreads();
  float qb[MAX_A];
#pragma unroll
  for (int a = 0; a < MAX_A; ++a) qb[a] = qbs[wave][a];
  float best = qb[0];
  int g = 0;
#pragma unroll
  for (int a = 1; a < MAX_A; ++a)
    if (a < A && qb[a] > best) { best = qb[a]; g = a; }
  const float eps = eps_f ? eps_f[f] : eps_all;
  const float pg = 1.f - eps, po = eps / (float)(A - 1);
  const uint64_t x = act_mix64(act_mix64(seed ^ act_mix64(counter)) + (uint64_t)f);
  const float u = (float)(uint32_t)(x >> 40) * (1.f / 16777216.f);  // [0, 1)
  // a draw past the rounded total falls on the last action of nonzero probability
  int act = pg > 0.f ? g : (g == A - 1 ? A - 2 : A - 1);
  float c = 0.f;
  bool done = false;
#pragma unroll
  for (int a = 0; a < MAX_A; ++a) {
    if (a < A && !done) {
      c += a == g ? pg : po;
      if (u < c) { act = a; done = true; }
    }
  }
  float qa = qb[0];
#pragma unroll
  for (int a = 0; a < MAX_A; ++a) qa = a == act ? qb[a] : qa;
  if (!valid) return;
  if (lane == 0) {
    actions[f] = act;
    q_pi[f] = qa;
    if (greedy_out) greedy_out[f] = g;
  }
  if (lane < W) q_star[(size_t)f * W + lane] = q_tg[((size_t)f * W + lane) * A + g];
}

// ApexDistributionalActor._make_replay's targets: one thread per (transition t, quantile k), the
// n-step return of replay_rollout_kernel (dqn_replay.hip) on column k of q_star [L][W]
__global__ __launch_bounds__(256) void iqn_nstep_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                        const float* __restrict__ q_star, long long K, int W,
                                                        int n_step, float gamma, float* __restrict__ targets) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * W) return;
  const long long t = i / W;
  const int k = (int)(i - t * W);
  const long long mm = min((long long)n_step, K - t);
  float acc = q_star[(t + mm) * W + k];  // v_{t+m-1}
  for (long long s = t + mm - 1; s >= t; --s) {
    const float d = done[s] ? 0.f : gamma;  // gamma (1 - done), exactly
    acc = fmaf(d, acc, rew[s]);             // one rounding per step
  }
  targets[i] = acc;
}
// priorities[t] = |mean_k target[t][k] - q_pi[t]|, the sum in k order
__global__ __launch_bounds__(256) void iqn_nstep_prio_kernel(const float* __restrict__ targets,
                                                             const float* __restrict__ q_pi, long long K, int W,
                                                             float* __restrict__ prio) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= K) return;
  float s = 0.f;
  for (int k = 0; k < W; ++k) s += targets[t * W + k];
  prio[t] = fabsf(s / (float)W - q_pi[t]);
}

// One source quantile's terms against the Wt targets of its transition, in j order: li = sum_j
// rho H_kappa(delta), gi = sum_j rho H_kappa'(delta), delta = target_j - q, rho = |tau - 1{delta < 0}|.
// The terms are fp32, their sums float64.  Shared by iqn_loss_head_kernel and iqn_head_step_kernel.
DEV void iqn_quantile_terms(const float* __restrict__ tg, int Wt, float q, float tau, float kappa, double& li,
                            double& gi) {
  li = 0.0;
  gi = 0.0;
  for (int j = 0; j < Wt; ++j) {
    const float d = tg[j] - q, ad = fabsf(d);
    const float rho = fabsf(tau - (d < 0.f ? 1.f : 0.f));
    float hub, g;
    if (kappa == 0.f) {  // (uniform branch)
      hub = ad;
      g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else {
      const float m = fminf(ad, kappa);
      hub = 0.5f * m * m + kappa * (ad - m);
      g = fminf(fmaxf(d, -kappa), kappa);
    }
    li += (double)(rho * hub);
    gi += (double)(rho * g);
  }
}

// DistributionalApex._train_step's loss on given heads (agents/dqn/learning.py:203-216,
// models/quantile_layers.py:83-93), one thread per transition; per quantile i the sum over the
// targets j in order, the quantiles' sums added in order.  The terms are fp32; their sums run in
// float64 and are rounded once, so a quantile's gradient does not carry the cancellation error of
// up to 32 fp32 additions of terms of either sign.  partials [gridDim.x][4]: sums of mean_i q,
// mean_j target, the priorities, w L.
__global__ __launch_bounds__(256) void iqn_loss_head_kernel(
    const float* __restrict__ adv, const float* __restrict__ v, const int64_t* __restrict__ act,
    const float* __restrict__ taus, const float* __restrict__ tgt, const float* __restrict__ prob, int N,
    int Ws, int Wt, int A, float kappa, float beta, float* __restrict__ dadv, float* __restrict__ dv,
    float* __restrict__ prio, float* __restrict__ partials) {
  __shared__ float red[4][4];
  __shared__ float pred[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 256 + threadIdx.x;
  const bool valid = n0 < N;
  const int n = valid ? n0 : N - 1;
  const int a = min(max((int)act[n], 0), A - 1);
  float w = 1.f;
  if (prob) {  // (uniform branch)
    const float p = prob[n];
    w = dqn_weight(p, dqn_batch_pmin(prob, N, pred), beta);
  }
  const float* tg = tgt + (size_t)n * Wt;
  float st = 0.f;
  for (int j = 0; j < Wt; ++j) st += tg[j];
  const float tmean = st / (float)Wt;
  const float gsc = -(w / (float)N) / (float)Wt;
  float sq = 0.f;
  double loss = 0.0;
  for (int i = 0; i < Ws; ++i) {
    const float* ar = adv + ((size_t)n * Ws + i) * A;
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += ar[k];
    const float q = (v[(size_t)n * Ws + i] + ar[a]) - s / (float)A;
    const float tau = taus[(size_t)n * Ws + i];
    double li, gi;
    iqn_quantile_terms(tg, Wt, q, tau, kappa, li, gi);
    loss += li;
    sq += q;
    if (valid) {
      const float dq = gsc * (float)gi, da = -dq / (float)A;
      float* dr = dadv + ((size_t)n * Ws + i) * A;
      for (int k = 0; k < A; ++k) dr[k] = k == a ? dq + da : da;
      dv[(size_t)n * Ws + i] = dq;
    }
  }
  const float qmean = sq / (float)Ws;
  const float pr = fabsf(tmean - qmean);
  if (valid) prio[n] = pr;
  float s[4] = {valid ? qmean : 0.f, valid ? tmean : 0.f, valid ? pr : 0.f,
                valid ? w * (float)(loss / (double)Wt) : 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partials[blockIdx.x * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}
// metrics4 = the workgroups' partial sums added in order, over N
__global__ void iqn_finalize_kernel(const float* __restrict__ part, int nparts, int N, float* __restrict__ metrics4) {
  const int k = threadIdx.x;
  if (k >= 4) return;
  float s = 0.f;
  for (int p = 0; p < nparts; ++p) s += part[p * 4 + k];
  metrics4[k] = s / (float)N;
}

// =========================================================================================
// The training step (DistributionalApex._train_step, agents/dqn/learning.py:197-237) past the conv
// trunk.  After the training forward (iqn_embed_ln_train_kernel, FcFwd over R rows):
//   iqn_head_step_kernel    heads forward over R rows, the loss, dz, the heads' weight-gradient slabs
//   fc_bwd_kernel           the dueling net's own FC weight / input gradient launch with M = R
//   iqn_ln_mod_bwd_kernel   per-row LayerNorm backward, dpre, dx_f (fixed-order sum over k), gamma / beta slabs
//   gemm_wg<IqnWqWgrad>     dWq, dbq slabs: the split weight-gradient GEMM over K = R rows
//   lnc3_conv12_bwd_dx      the trunk's per-frame backward from dx (lnc3.h, LNC3_DX)
//   wgrad23_kernel          the core's conv3 / conv2 weight gradients (ops.h), instantiated here too
//   iqn_reduce_ins_kernel   the Wq / bq slabs into the flat gradient's inserted segment
//   iqn_adam_kernel, iqn_adam_ins_kernel   clip + Adam on the IQN flat order
// =========================================================================================

// Rows per workgroup of iqn_head_step_kernel: whole frames, at most DQN_F rows.
__host__ DEV int iqn_head_rows(int W) { return (DQN_F / W) * W; }

// dqn_head_step_kernel (dqn_head_step.h) over quantile rows: the same four phases and wave maps on
// a block of whole frames (iqn_head_rows(W) <= 32 rows), with the quantile-regression loss in
// phase 2.  Phase 2 runs on wave 0, one lane per row (f, i): q_i at the frame's action, the sums
// over the frame's targets j (iqn_quantile_terms), d loss / d heads of the row = iqn_loss_head's
// dadv, dv, which already carry w_f / N; the frame's first lane then adds the W rows' terms in
// i order for the priority and the loss partials.
template <typename T>
__global__ __launch_bounds__(256) void iqn_head_step_kernel(const iqn_dev::HeadStepArgs a) {
  constexpr int HID = HID_DQN, FR = DQN_F;
  constexpr int JC = HID / DQN_SPLIT;
  static_assert(JC == 64 && FR == 32, "phase 1 / 3 / 4 wave maps: 4 column tiles, 2 frame tiles");
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int LDH = HID + VEC;
  constexpr int LDD = HPAD + VEC;
  constexpr int LDZ = JC + 4;
  __shared__ __attribute__((aligned(16))) T hs[FR * LDH];
  __shared__ __attribute__((aligned(16))) T whs[HEADS * LDH];
  __shared__ __attribute__((aligned(16))) T dHs[FR * LDD];
  __shared__ __attribute__((aligned(16))) float zs[FR * LDZ];
  __shared__ float lg_s[FR][HEADS + 1];
  __shared__ f32x4 hp[2][64];
  __shared__ float bred[4][HEADS];
  __shared__ float pred[4];
  __shared__ double li_s[FR];  // phase 2: the rows' loss sums and q, for the frame's first lane
  __shared__ float q_s[FR];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = a.W, A = a.A;
  const int rpb = iqn_head_rows(W);
  const int r0 = blockIdx.x * rpb;
  const int nf = min(rpb, a.R - r0);  // valid rows of this workgroup (>= 1, whole frames)
  const int jw = blockIdx.y * JC;
  const bool lead = blockIdx.y == 0;
  const T* hg = reinterpret_cast<const T*>(a.h);
  // ---- every global load, up front and unconditional (rows past the block's are copies of its
  // last one, which only meet zero dH rows or outputs nobody stores) ----
  const int rl = min(lane, nf - 1);  // phase 2: this lane's row (wave 0)
  const int fr_l = (r0 + rl) / W;    // its frame
  const int act_l = reinterpret_cast<const int*>(a.act)[2 * (size_t)fr_l];  // low word: in [0, A)
  const float tau_l = a.taus[r0 + rl];
  const float* pp = a.prob ? a.prob : a.taus;  // (an unused value without probabilities)
  const float p_l = pp[a.prob ? fr_l : 0];
  const float* tg_l = a.tgt + (size_t)fr_l * W;
  constexpr int NHV = FR * (HID / VEC) / 256, NZV = FR * (JC / 4) / 256;
  constexpr int NWV = HEADS * (HID / VEC) / 256;
  constexpr int NKH = HID / F::KSTEP / 2, NKT = HPAD / F::KSTEP;
  const int kl = F::KPL * (lane >> 4);
  V hv[NHV], whv[NWV], wtf[NKT];
  f32x4 zv[NZV];
#pragma unroll
  for (int i = 0; i < NHV; ++i) {
    const int e = tid + i * 256, f = min(e / (HID / VEC), nf - 1), c = (e % (HID / VEC)) * VEC;
    hv[i] = *reinterpret_cast<const V*>(hg + (size_t)(r0 + f) * HID + c);
  }
#pragma unroll
  for (int i = 0; i < NZV; ++i) {
    const int e = tid + i * 256, f = min(e / (JC / 4), nf - 1), c = (e % (JC / 4)) * 4;
    zv[i] = *reinterpret_cast<const f32x4*>(a.zg + (size_t)(r0 + f) * HID + jw + c);
  }
  {
    const T* wh = reinterpret_cast<const T*>(a.wh);
    const T* wht = reinterpret_cast<const T*>(a.wht);
#pragma unroll
    for (int i = 0; i < NWV; ++i) whv[i] = F::load(wh + (size_t)(tid + i * 256) * VEC);
#pragma unroll
    for (int ks = 0; ks < NKT; ++ks)
      wtf[ks] = F::load(wht + (size_t)(jw + wave * 16 + (lane & 15)) * HPAD + ks * F::KSTEP + kl);
  }
  float bhv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bhv[q] = a.bh[4 * (lane >> 4) + q];
  float pmin = 1.f;
  if (a.prob) pmin = dqn_batch_pmin(a.prob, a.N, pred);  // (uniform branch)
  // ---- phase 1: stage h, z and Wh, zero dH, heads forward ----
#pragma unroll
  for (int i = 0; i < NHV; ++i) {
    const int e = tid + i * 256, f = e / (HID / VEC), c = (e % (HID / VEC)) * VEC;
    *reinterpret_cast<V*>(hs + f * LDH + c) = hv[i];
  }
#pragma unroll
  for (int i = 0; i < NZV; ++i) {
    const int e = tid + i * 256, f = e / (JC / 4), c = (e % (JC / 4)) * 4;
    *reinterpret_cast<f32x4*>(zs + f * LDZ + c) = zv[i];
  }
#pragma unroll
  for (int i = 0; i < NWV; ++i) {
    const int e = tid + i * 256, r = e / (HID / VEC), c = (e % (HID / VEC)) * VEC;
    *reinterpret_cast<V*>(whs + r * LDH + c) = whv[i];
  }
  for (int e = tid; e < FR * LDD / VEC; e += 256) *reinterpret_cast<V*>(dHs + e * VEC) = F::zero();
  __syncthreads();
  {
    const int f = (wave & 1) * 16 + (lane & 15);
    const int kb = (wave >> 1) * NKH;
    static_assert(NKH % 4 == 0, "four accumulators");
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k4 = 0; k4 < NKH; k4 += 4) {
      V w[4], hf[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        w[u] = *reinterpret_cast<const V*>(whs + (lane & 15) * LDH + (kb + k4 + u) * F::KSTEP + kl);
        hf[u] = *reinterpret_cast<const V*>(hs + f * LDH + (kb + k4 + u) * F::KSTEP + kl);
      }
#pragma unroll
      for (int e = 0; e < F::NE; ++e)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = F::mma_e(e, w[u], hf[u], acc[u]);
    }
    f32x4 hsum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (wave >= 2) hp[wave - 2][lane] = hsum;
    __syncthreads();
    if (wave < 2) {
      hsum += hp[wave][lane];
#pragma unroll
      for (int q = 0; q < 4; ++q) lg_s[f][4 * (lane >> 4) + q] = hsum[q] + bhv[q];
    }
  }
  __syncthreads();
  // ---- phase 2: wave 0, one lane per row ----
  const bool valid = lane < nf;
  const int aa = min(act_l, A - 1);
  const float w_l = a.prob ? dqn_weight(p_l, pmin, a.beta) : 1.f;
  if (wave == 0) {
    float hd[HEADS];
#pragma unroll
    for (int k = 0; k < HEADS; ++k) hd[k] = lg_s[rl][k];
    float s = 0.f, adv_a = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_A; ++k) {  // padded rows A..14 stay out of the mean
      s += k < A ? hd[k] : 0.f;
      adv_a = k == aa ? hd[k] : adv_a;
    }
    const float q = (hd[VCOL] + adv_a) - s / (float)A;
    double li, gi;
    iqn_quantile_terms(tg_l, W, q, tau_l, a.kappa, li, gi);
    if (valid) {
      const float gsc = -(w_l / (float)a.N) / (float)W;
      const float dq = gsc * (float)gi, da = -dq / (float)A;
#pragma unroll
      for (int k = 0; k < MAX_A; ++k)
        if (k < A) dHs[lane * LDD + k] = (T)(k == aa ? dq + da : da);
      dHs[lane * LDD + VCOL] = (T)dq;
      li_s[lane] = li;
      q_s[lane] = q;
      if (lead) {  // the heads as the loss read them (iqn_debug_read)
        float* ho = a.heads + (size_t)(r0 + lane) * HEADS;
#pragma unroll
        for (int k = 0; k < HEADS; k += 4)
          *reinterpret_cast<f32x4*>(ho + k) = f32x4{hd[k], hd[k + 1], hd[k + 2], hd[k + 3]};
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    const bool first = valid && lane % W == 0;  // the frame's first row: the frame's terms, in i order
    float sq = 0.f, st = 0.f;
    double loss = 0.0;
    if (first) {
      for (int i = 0; i < W; ++i) {
        loss += li_s[lane + i];
        sq += q_s[lane + i];
      }
      for (int j = 0; j < W; ++j) st += tg_l[j];
    }
    const float qmean = sq / (float)W, tmean = st / (float)W, pr = fabsf(tmean - qmean);
    if (first && lead) a.prio[fr_l] = pr;
    float s4[4] = {first ? qmean : 0.f, first ? tmean : 0.f, first ? pr : 0.f,
                   first ? w_l * (float)(loss / (double)W) : 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) s4[k] = wave_sum(s4[k]);
    if (lane == 0 && lead) {
      float* po = a.partials + (size_t)blockIdx.x * 8;
#pragma unroll
      for (int k = 0; k < 4; ++k) po[k] = s4[k];
    }
  }
  // ---- phase 3: dz = gelu'(z) * (dH . Wh): wave -> column tile, both row tiles ----
  {
    T* dz = reinterpret_cast<T*>(a.dz);
    const int j0 = jw + wave * 16;
#pragma unroll
    for (int ct = 0; ct < FR / 16; ++ct) {
      if (ct * 16 >= nf) break;  // a row tile past the block's rows (uniform)
      const int f = ct * 16 + (lane & 15);
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKT; ++ks)
        acc = F::mma(wtf[ks], *reinterpret_cast<const V*>(dHs + f * LDD + ks * F::KSTEP + kl), acc);
      if (f < nf) {
        const int j = j0 + 4 * (lane >> 4);
        const f32x4 zz = *reinterpret_cast<const f32x4*>(zs + f * LDZ + j - jw);
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = acc[q] * zz[q];
        store4(dz + (size_t)(r0 + f) * HID + j, o);
      }
    }
  }
  // ---- phase 4: dWh partial = dH^T . h over the block's rows (the dH rows past them are zero) ----
  {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = jw + wave * 16;
#pragma unroll
    for (int kk = 0; kk < FR; kk += F::KSTEP)
      acc = F::mma(lds_frag_k(dHs + kk * LDD, LDD, lane), lds_frag_k(hs + kk * LDH + c0, LDH, lane), acc);
    float* sl = a.slab_h + (size_t)blockIdx.x * HEADS * HID;
#pragma unroll
    for (int q = 0; q < 4; ++q) sl[(4 * (lane >> 4) + q) * HID + c0 + (lane & 15)] = acc[q];
    if (lead) {  // bias = sum over rows of dH: 16 groups x 16 heads, fixed-order tree
      const int o = tid & 15, fg = tid >> 4;
      float b = 0.f;
      for (int f = fg; f < nf; f += 16) b += (float)dHs[f * LDD + o];
      b = xor32_sum(xor16_sum(b));
      if ((lane >> 4) == 0) bred[wave][o] = b;
      __syncthreads();
      if (tid < HEADS)
        a.slab_bh[(size_t)blockIdx.x * HEADS + tid] = bred[0][tid] + bred[1][tid] + bred[2][tid] + bred[3][tid];
    }
  }
}

// Backward of y_r = LayerNorm(x_f * phi_r) for the rows of whole frames [f0, f1) per workgroup, in
// 16-row tiles as the forward (8 waves: wave w owns features 128 w .. 128 w + 127, a lane four
// consecutive features of eight 16-feature tiles for row `col`).  pre / phi are recomputed from the
// stored cosine tile with the forward's own MFMAs (iqn_wq_tile) and x-hat from the stored
// statistics; with g = dy * gamma:
//   dm = rstd (g - mean(g) - x-hat mean(g x-hat)), dpre = dm x gelu'(pre)  (stored in T),
//   dx_f = relu'(x_f) sum_k dm phi.
// The sum over k: the tile's dm phi goes to LDS, and each thread adds its two features' rows in row
// order into a running sum that starts at a frame's first row and is stored at its last -- the plain
// left-to-right sum over k = 0..W-1 wherever the 16-row tiles cut the frame.  The gamma / beta partials
// of a tile are summed over its 16 rows' lanes by DPP in a fixed order and added, tile after tile, to
// the workgroup's slab [2][1024] in LDS (every feature has one owning lane), which is written out at
// the end; 64 more accumulators per lane did not fit the 256 registers beside the 128 values a
// lane keeps across the row sums.  Rows past the workgroup's last are clamped on load and masked on
// store.
constexpr int IQN_BWD_WAVES = 8;
template <typename T>
__global__ __launch_bounds__(64 * IQN_BWD_WAVES) void iqn_ln_mod_bwd_kernel(const iqn_dev::LnModBwdArgs a) {
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int NK = NCOS / F::KSTEP;
  constexpr int NWV = IQN_BWD_WAVES, NT = 64 * NWV;
  constexpr int TPW = FLAT / 16 / NWV;  // 16-feature tiles per wave
  constexpr int LDC = FLAT + 4;
  constexpr int FPT = FLAT / NT;  // features per thread of the sum over k
  static_assert(FPT == 2, "the sum over k: two features per thread");
  __shared__ __attribute__((aligned(16))) float cs[IQN_TILE * LDC];
  __shared__ __attribute__((aligned(16))) float xgs[IQN_TILE * LDC];  // x gelu'(pre) of the tile
  __shared__ float red[2][NWV][IQN_TILE];
  __shared__ __attribute__((aligned(16))) float gs[2 * FLAT];  // the gamma / beta slab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, grp = lane >> 4, kl = F::KPL * grp;
  const int W = a.W;
  const int f0 = blockIdx.x * a.fpw, f1 = min(a.N, f0 + a.fpw);
  const int rb = f0 * W, re = f1 * W;  // this workgroup's rows
  const T* e = reinterpret_cast<const T*>(a.e);
  const T* act3 = reinterpret_cast<const T*>(a.act3);
  const T* wq = reinterpret_cast<const T*>(a.wq);
  T* dpre = reinterpret_cast<T*>(a.dpre);
  static_assert(2 * FLAT == 4 * NT, "the slab: one float4 per thread");
  *reinterpret_cast<f32x4*>(gs + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  float xs[FPT] = {0.f, 0.f};  // the running sum over k of features FPT tid ..
  int k_run = 0;               // the quantile index of the tile's first row
  for (int t0 = rb; t0 < re; t0 += IQN_TILE) {
    const bool valid = t0 + col < re;
    const int r = min(t0 + col, re - 1);
    const int f = r / W;
    V b[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) b[s] = F::load(e + (size_t)r * NCOS + s * F::KSTEP + kl);
    const float mean = a.stats[2 * r], rstd = a.stats[2 * r + 1];
    const T* xrow = act3 + (size_t)f * FLAT;
    const float* dyrow = a.dy + (size_t)r * FLAT;
    // kept across the row sums: g and x-hat in registers; phi and x gelu'(pre) in this lane's own
    // slots of two LDS tiles (dm phi then replaces phi).  All four in registers, 128 values beside
    // the GELU's temporaries, spilled at 256 registers per lane.
    float G[TPW][4], XH[TPW][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int j0 = (wave * TPW + t) * 16;
      const f32x4 acc = iqn_wq_tile<T, NK>(wq, j0, col, kl, b);
      const int j = j0 + 4 * grp;
      float x[4], bb[4], gm[4];
      load4(xrow + j, x);
      load4(a.bq + j, bb);
      load4(a.gam + j, gm);
      const f32x4 dyv = *reinterpret_cast<const f32x4*>(dyrow + j);
      float ph[4], xg[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float phi, gp;
        gelu_fwd_grad(acc[q] + bb[q], phi, gp);
        ph[q] = phi;
        xg[q] = x[q] * gp;
        const float xh = (x[q] * phi - mean) * rstd;
        const float g = dyv[q] * gm[q];
        s1 += g;
        s2 += g * xh;
        const float cg = row16_sum(valid ? dyv[q] * xh : 0.f), cb = row16_sum(valid ? dyv[q] : 0.f);
        if (col == 0) {
          gs[j + q] += cg;
          gs[FLAT + j + q] += cb;
        }
        G[t][q] = g; XH[t][q] = xh;
      }
      *reinterpret_cast<f32x4*>(cs + col * LDC + j) = f32x4{ph[0], ph[1], ph[2], ph[3]};
      *reinterpret_cast<f32x4*>(xgs + col * LDC + j) = f32x4{xg[0], xg[1], xg[2], xg[3]};
      __builtin_amdgcn_sched_barrier(0);  // one feature tile's loads in flight at a time
    }
    // the row's two sums: over the lanes' 4 row groups, then the 8 waves in order
    s1 = xor32_sum(xor16_sum(s1));
    s2 = xor32_sum(xor16_sum(s2));
    if (grp == 0) { red[0][wave][col] = s1; red[1][wave][col] = s2; }
    __syncthreads();
    float S1 = 0.f, S2 = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) { S1 += red[0][w][col]; S2 += red[1][w][col]; }
    S1 *= 1.f / FLAT;
    S2 *= 1.f / FLAT;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int j = (wave * TPW + t) * 16 + 4 * grp;
      const f32x4 ph = *reinterpret_cast<const f32x4*>(cs + col * LDC + j);
      const f32x4 xg = *reinterpret_cast<const f32x4*>(xgs + col * LDC + j);
      float dp[4], c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dm = rstd * (G[t][q] - S1 - XH[t][q] * S2);
        dp[q] = dm * xg[q];
        c[q] = dm * ph[q];
      }
      if (valid) store4(dpre + (size_t)r * FLAT + j, dp);
      *reinterpret_cast<f32x4*>(cs + col * LDC + j) = f32x4{c[0], c[1], c[2], c[3]};
    }
    __syncthreads();
    {  // the sum over k, rows in order
      const int nrow = min(IQN_TILE, re - t0);
      int k = k_run, fr = t0 / W;
      for (int rr = 0; rr < nrow; ++rr) {
        const float c0 = cs[rr * LDC + FPT * tid], c1 = cs[rr * LDC + FPT * tid + 1];
        xs[0] = k == 0 ? c0 : xs[0] + c0;
        xs[1] = k == 0 ? c1 : xs[1] + c1;
        if (++k == W) {
          const T* xr = act3 + (size_t)fr * FLAT + FPT * tid;
          float* o = a.dx + (size_t)fr * FLAT + FPT * tid;
          o[0] = (float)xr[0] > 0.f ? xs[0] : 0.f;
          o[1] = (float)xr[1] > 0.f ? xs[1] : 0.f;
          k = 0;
          ++fr;
        }
      }
      k_run = k;
    }
    __syncthreads();  // cs and red are rewritten by the next tile
  }
  // ---- the gamma / beta slab of this workgroup (the tile loop ended on a barrier) ----
  *reinterpret_cast<f32x4*>(a.slab + (size_t)blockIdx.x * 2 * FLAT + 4 * tid) =
      *reinterpret_cast<const f32x4*>(gs + 4 * tid);
}

// dWq[j][i] = sum_r dpre[r][j] e[r][i], dbq[j] = sum_r dpre[r][j]: the weight-gradient GEMM's operand
// (gemm_wg: rows j in the kernel order p*64 + c, columns i, K = R split over blockIdx.z).  Y is the
// cosine tile the training forward stored in T -- the values the forward's MFMAs read.
template <typename T> struct IqnWqWgrad {
  static constexpr int R = FLAT, C = NCOS;
  int M;
  float out_scale = 1.f;
  const T* x;  // dpre
  int x_ld = FLAT;
  const T* e;
  DEV int y_roff(int m) const { return m * NCOS; }
  DEV int y_coff(int c) const { return c; }
  DEV int y_bytes() const { return M * NCOS * (int)sizeof(T); }
  DEV const T* ybase() const { return e; }
  template <int D> static constexpr int y_stride() { return D * NCOS; }
};

// The Wq / bq slabs [S][1024][64], [S][1024] (kernel rows p*64 + c) summed in split order into the
// flat gradient's inserted segment at the canonical row c*16 + p (the inverse of iqn_pack_kernel):
// workgroups 0..63 a float4 of Wq per thread, workgroup 64 four rows of bq per thread.  Each
// workgroup's sum of squares is one clip-norm partial behind the core's.  fin: the loss metrics
// from the head's partials and the Adam step counter, as reduce_grads_kernel's block 0 does.
constexpr int IQN_INS_WGS = FLAT * NCOS / 4 / 256 + 1;
__global__ __launch_bounds__(256) void iqn_reduce_ins_kernel(const iqn_dev::RedInsArgs a, int fin) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float sq = 0.f;
  if (blockIdx.x < IQN_INS_WGS - 1) {
    const int v4 = blockIdx.x * 256 + tid, jk = v4 >> 4, i = (v4 & 15) * 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.S; ++s)
      acc += *reinterpret_cast<const f32x4*>(a.s_wq + ((size_t)s * FLAT + jk) * NCOS + i);
    const int jc = (jk & 63) * 16 + (jk >> 6);
    *reinterpret_cast<f32x4*>(a.grads_ins + (size_t)jc * NCOS + i) = acc;
    sq = (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
  } else {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.S; ++s) acc += *reinterpret_cast<const f32x4*>(a.s_bq + (size_t)s * FLAT + 4 * tid);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jk = 4 * tid + q;
      a.grads_ins[(size_t)FLAT * NCOS + (jk & 63) * 16 + (jk >> 6)] = acc[q];
    }
    sq = (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
  }
  sq = wave_sum(sq);
  if ((tid & 63) == 0) red[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) a.sumsq[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  if (fin && blockIdx.x == 0 && tid == 64) {  // mean q, mean target, mean priorities, loss
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < a.n_loss_part; ++p)
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += a.loss_part[p * 8 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) a.metrics[k] = s[k] / (float)a.N;
    a.metrics[4] = a.metrics[5] = a.metrics[8] = 0.f;
  }
  if (fin && blockIdx.x == 0 && tid == 128) {  // step += 1 and its bias corrections
    const int64_t t = *a.step + 1;
    *a.step = t;
    adam_step_scalars(a.lr, a.b1, a.b2, t, a.adam_sc[0], a.adam_sc[1]);
  }
}

// adam_kernel's body (adam.h) on the IQN flat order: the handle's Canon index i lies at i, or past
// the inserted segment at i + ins
template <typename T>
__global__ __launch_bounds__(256) void iqn_adam_kernel(const AdamArgs a, const FlatGap fm) {
  adam_body<T, HID_DQN>(a, fm);
}
// ... and the inserted segment itself, one parameter per thread: the same norm, clip and update,
// then Wq / bq re-emitted in kernel layout (iqn_pack_kernel's map)
template <typename T>
__global__ __launch_bounds__(256) void iqn_adam_ins_kernel(const AdamArgs a, size_t gap, T* __restrict__ wq,
                                                           float* __restrict__ bq) {
  __shared__ float red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;  // < FLAT * NCOS + FLAT (a multiple of 256)
  const size_t x = gap + (size_t)i;
  float g = a.grads[x], m = a.m[x], v = a.v[x], p = a.params[x];
  const float step_size = a.sc[0], bc2s = a.sc[1];
  const float norm = adam_grad_norm(a, red);
  const float coef = fminf(a.max_norm / (norm + 1e-6f), 1.f);
  adam_elem(a, a.inv_world * coef, step_size, bc2s, g, m, v, p);
  a.grads[x] = g; a.m[x] = m; a.v[x] = v; a.params[x] = p;
  if (i < FLAT * NCOS) {
    const int j = i >> 6, k = i & 63;
    wq[((j & 15) * OC3 + (j >> 4)) * NCOS + k] = (T)p;
  } else {
    const int j = i - FLAT * NCOS;
    bq[(j & 15) * OC3 + (j >> 4)] = p;
  }
}
static_assert((FLAT * NCOS + FLAT) % 256 == 0, "iqn_adam_ins_kernel: whole workgroups");

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// the training step past act3 (iqn_launch.h launch_step), one compute type
template <typename T>
hipError_t step_t(const iqn_dev::StepWork& s, const iqn_dev::TrunkBwd& tb, const float* taus, const int64_t* act,
                  const float* tgt, const float* prob, float* prio, int N, int W, int A, float beta, float kappa,
                  int n_cu, hipStream_t st) {
  const int R = N * W;
  hipError_t e;
  iqn_embed_ln_train_kernel<T><<<blocks(R, IQN_TILE), 256, 0, st>>>(
      taus, (const T*)tb.act3, (const T*)s.w.wq, s.w.bq, s.w.gam, s.w.bet, (T*)s.fw.y, R, W, s.stats, (T*)s.e);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    FcFwd<T, HID_DQN> op{R, (const T*)s.w.wfc, s.w.bfc, (const T*)s.fw.y, s.fw.zg, (T*)s.fw.h};
    using C = FcFwdCfg<T>;
    const long tiles = (long)blocks(R, C::BC) * (HID_DQN / C::BR), cap = (long)n_cu * 3;
    gemm_tile<T, C::BR, C::BC, C::BK, 2, C::NW / 2, FcFwd<T, HID_DQN>, C::PF, C::KW>
        <<<(unsigned)(tiles < cap ? tiles : cap), 64 * C::NW, 0, st>>>(op, HID_DQN / C::BR);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    iqn_dev::HeadStepArgs ha{};
    ha.h = s.fw.h; ha.zg = s.fw.zg; ha.wh = s.w.wh; ha.wht = s.wht; ha.bh = s.w.bh;
    ha.act = act; ha.taus = taus; ha.tgt = tgt; ha.prob = prob;
    ha.N = N; ha.W = W; ha.R = R; ha.A = A; ha.beta = beta; ha.kappa = kappa;
    ha.dz = s.dz; ha.heads = s.fw.heads; ha.partials = s.loss_part; ha.slab_h = s.s_h; ha.slab_bh = s.s_bh;
    ha.prio = prio;
    iqn_head_step_kernel<T><<<dim3(iqn_dev::head_step_wgs(N, W), DQN_SPLIT), 256, 0, st>>>(ha);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {  // the dueling net's FC backward launch with M = R; the input-gradient tiles on a persistent grid
    constexpr int WG2 = sizeof(T) == 2 ? 2 : 1;
    FcWgrad<T, HID_DQN> ow{};
    ow.M = R; ow.x = (const T*)s.dz; ow.y = (const T*)s.fw.y;
    FcDgrad<T, HID_DQN> od{R, (const T*)s.w.wfc, (const T*)s.dz, s.dy};
    using C = FcBwdCfg<T, WG2, HID_DQN>;
    const int gx = FLAT / C::WBC, gy = HID_DQN / 64, gz = s.fc_S;
    const int n_rt = FLAT / C::DR;
    const long n_dt = (long)n_rt * blocks(R, C::DC), cap = (long)n_cu * 3;
    fc_bwd_kernel<T, WG2, HID_DQN><<<gx * gy * gz + (unsigned)(n_dt < cap ? n_dt : cap), 256 * WG2, 0, st>>>(
        ow, s.s_fc, s.s_bfc, s.fc_mps, gx, gy, gz, od, n_rt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    iqn_dev::LnModBwdArgs la{};
    la.e = s.e; la.act3 = tb.act3; la.wq = s.w.wq; la.bq = s.w.bq; la.gam = s.w.gam; la.stats = s.stats;
    la.dy = s.dy; la.dpre = s.dpre; la.dx = s.dx; la.slab = s.s_ln; la.N = N; la.W = W; la.fpw = s.ln_fpw;
    iqn_ln_mod_bwd_kernel<T><<<s.ln_wgs, 64 * IQN_BWD_WAVES, 0, st>>>(la);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    constexpr int WG4 = sizeof(T) == 2 ? 2 : 1;
    IqnWqWgrad<T> ow{};
    ow.M = R; ow.x = (const T*)s.dpre; ow.e = (const T*)s.e;
    gemm_wg<T, 64, 64, 2, 2, 32, WG4, IqnWqWgrad<T>>
        <<<dim3(NCOS / 64, FLAT / 64, s.wq_S), 256 * WG4, 0, st>>>(ow, s.s_wq, s.s_bq, s.wq_mps);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  lnc3_conv12_bwd_dx<T><<<tb.wgs, lnc3_threads<T>(), 0, st>>>(
      s.dx, (const T*)tb.act3, (const T*)tb.w3, (const T*)tb.w3t, (const T*)tb.act2, (T*)tb.dact3, (T*)tb.dact2,
      tb.obs, (const T*)tb.w2, (const T*)tb.w2t, tb.mask1, tb.s_w1, tb.s_b1, N, tb.fpw);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {  // conv3 + conv2 weight gradients from the dact3 / dact2 just written: the core's merged launch
     // (impala.hip launch_backward, wg23) on this translation unit's own instantiation of the kernel
    constexpr int WG4 = sizeof(T) == 2 ? 2 : 1;
    Conv3Wgrad<T> o3{};
    o3.M = N * P3; o3.x = (const T*)tb.dact3; o3.in = (const T*)tb.act2;
    Conv2Wgrad<T> o2{};
    o2.M = N * P2; o2.x = (const T*)tb.dact2; o2.in = (const T*)tb.act1;
    const int g3x = K3 / 64, g3z = tb.S3, g2x = K2 / Wg2Tile<T>::BC, g2z = tb.S2;
    wgrad23_kernel<T, WG4><<<g3x * g3z + g2x * g2z, 256 * WG4, 0, st>>>(o3, tb.s_w3, tb.s_b3, tb.mps3, g3x, g3z, o2,
                                                                      tb.s_w2, tb.s_b2, tb.mps2, g2x, g2z);
  }
  return hipGetLastError();
}

template <typename T>
hipError_t head_t(const iqn_dev::HeadWeights& w, const iqn_dev::HeadWork& ws, const void* act3, const float* taus,
                  int R, int W, int A, int n_cu, float* q, hipStream_t st) {
  iqn_embed_ln_kernel<T><<<blocks(R, IQN_TILE), 256, 0, st>>>(taus, (const T*)act3, (const T*)w.wq, w.bq, w.gam,
                                                              w.bet, (T*)ws.y, R, W);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  {
    FcFwd<T, HID_DQN> op{R, (const T*)w.wfc, w.bfc, (const T*)ws.y, ws.zg, (T*)ws.h};
    using C = FcFwdCfg<T>;
    const long tiles = (long)blocks(R, C::BC) * (HID_DQN / C::BR), cap = (long)n_cu * 3;
    gemm_tile<T, C::BR, C::BC, C::BK, 2, C::NW / 2, FcFwd<T, HID_DQN>, C::PF, C::KW>
        <<<(unsigned)(tiles < cap ? tiles : cap), 64 * C::NW, 0, st>>>(op, HID_DQN / C::BR);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    HeadsFwd<T, HID_DQN> op{R, (const T*)w.wh, w.bh, (const T*)ws.h, ws.heads};
    gemm_rc<T, 1, 1, HeadsFwd<T, HID_DQN>><<<dim3(blocks(R, 64), 1), 256, 0, st>>>(op);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  iqn_q_kernel<<<blocks(R, 256), 256, 0, st>>>(ws.heads, R, A, q);
  return hipGetLastError();
}

}  // namespace

namespace iqn_dev {

hipError_t launch_pack(bool bf16, const float* wq_bq, void* wq, float* bq, hipStream_t st) {
  const unsigned g = blocks(FLAT * NCOS + FLAT, 256);
  if (bf16)
    iqn_pack_kernel<__bf16><<<g, 256, 0, st>>>(wq_bq, (__bf16*)wq, bq);
  else
    iqn_pack_kernel<float><<<g, 256, 0, st>>>(wq_bq, (float*)wq, bq);
  return hipGetLastError();
}

hipError_t launch_taus(uint64_t seed, uint64_t counter, int which, int R, float* taus, hipStream_t st) {
  iqn_tau_kernel<<<blocks(R, 256), 256, 0, st>>>(seed, counter, which, R, taus);
  return hipGetLastError();
}

hipError_t launch_head(bool bf16, const HeadWeights& w, const HeadWork& ws, const void* act3, const float* taus,
                       int R, int W, int A, int n_cu, float* q, hipStream_t st) {
  return bf16 ? head_t<__bf16>(w, ws, act3, taus, R, W, A, n_cu, q, st)
              : head_t<float>(w, ws, act3, taus, R, W, A, n_cu, q, st);
}

hipError_t launch_act(const float* q_on, const float* q_tg, int n, int W, int A, const float* eps, float eps_all,
                      uint64_t seed, uint64_t counter, int64_t* actions, float* q_pi, float* q_star,
                      int64_t* greedy, hipStream_t st) {
  iqn_act_kernel<<<blocks(n, 4), 256, 0, st>>>(q_on, q_tg, n, W, A, eps, eps_all, seed, counter, actions, q_pi,
                                                 q_star, greedy);
  return hipGetLastError();
}

hipError_t launch_nstep(const float* rew, const uint8_t* done, const float* q_pi, const float* q_star, long long K,
                        int W, int n_step, float gamma, float* targets, float* prio, hipStream_t st) {
  iqn_nstep_kernel<<<blocks(K * W, 256), 256, 0, st>>>(rew, done, q_star, K, W, n_step, gamma, targets);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  iqn_nstep_prio_kernel<<<blocks(K, 256), 256, 0, st>>>(targets, q_pi, K, W, prio);
  return hipGetLastError();
}

hipError_t launch_loss_head(const float* adv, const float* v, const int64_t* act, const float* taus,
                            const float* tgt, const float* prob, int N, int Ws, int Wt, int A, float kappa,
                            float beta, float* dadv, float* dv, float* prio, float* part, float* metrics4,
                            hipStream_t st) {
  const unsigned wgs = blocks(N, 256);
  iqn_loss_head_kernel<<<wgs, 256, 0, st>>>(adv, v, act, taus, tgt, prob, N, Ws, Wt, A, kappa, beta, dadv, dv,
                                            prio, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  iqn_finalize_kernel<<<1, 64, 0, st>>>(part, (int)wgs, N, metrics4);
  return hipGetLastError();
}

int head_step_wgs(int N, int W) { return (int)blocks(N, DQN_F / W); }
int ins_wgs() { return IQN_INS_WGS; }

hipError_t launch_step(bool bf16, const StepWork& s, const TrunkBwd& tb, const float* taus, const int64_t* act,
                       const float* tgt, const float* prob, float* prio, int N, int W, int A, float beta,
                       float kappa, int n_cu, hipStream_t st) {
  return bf16 ? step_t<__bf16>(s, tb, taus, act, tgt, prob, prio, N, W, A, beta, kappa, n_cu, st)
              : step_t<float>(s, tb, taus, act, tgt, prob, prio, N, W, A, beta, kappa, n_cu, st);
}

hipError_t launch_reduce_ins(const RedInsArgs& a, int fin, hipStream_t st) {
  iqn_reduce_ins_kernel<<<IQN_INS_WGS, 256, 0, st>>>(a, fin);
  return hipGetLastError();
}

hipError_t launch_adam(bool bf16, const AdamIns& a, hipStream_t st) {
  const unsigned gi = (FLAT * NCOS + FLAT) / 256;
  if (bf16) {
    iqn_adam_kernel<__bf16><<<a.grid, 256, 0, st>>>(a.a, a.fm);
    iqn_adam_ins_kernel<__bf16><<<gi, 256, 0, st>>>(a.a, a.fm.gap, (__bf16*)a.wq, a.bq);
  } else {
    iqn_adam_kernel<float><<<a.grid, 256, 0, st>>>(a.a, a.fm);
    iqn_adam_ins_kernel<float><<<gi, 256, 0, st>>>(a.a, a.fm.gap, (float*)a.wq, a.bq);
  }
  return hipGetLastError();
}

}  // namespace iqn_dev
