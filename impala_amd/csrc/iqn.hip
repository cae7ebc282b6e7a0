// Kernels of the distributional (IQN) Ape-X actor path (include/iqn_hip.h) and their launchers
// (csrc/iqn_launch.h).  A translation unit of its own, so the code object of impala.hip -- the
// learner steps' kernels and where they sit in it -- is the same with or without it; the host
// side is csrc/iqn.h, included at the end of impala.hip.
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
#include "dqn_head_step.h"
#include "iqn_launch.h"
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

template <typename T>
__global__ __launch_bounds__(256) void iqn_embed_ln_kernel(const float* __restrict__ taus,
                                                           const T* __restrict__ act3, const T* __restrict__ wq,
                                                           const float* __restrict__ bq,
                                                           const float* __restrict__ gam,
                                                           const float* __restrict__ bet, T* __restrict__ y, int R,
                                                           int W) {
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
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // torch's order for torch.pi * embedding_range * tau: (fl(pi) * i) * tau, two roundings
      const float pi_i = 3.14159274101257324f * (float)(i0 + q + 1);
      es[rr * LDE + i0 + q] = (T)cosf(pi_i * tau);
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
    const T* arow = wq + (size_t)(j0 + col) * NCOS;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NK; ++s) acc = F::mma(F::load(arow + s * F::KSTEP + kl), b[s], acc);
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
    double li = 0.0, gi = 0.0;
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

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

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

}  // namespace iqn_dev
