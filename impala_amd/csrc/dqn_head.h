// Ape-X DQN head (agents/dqn/learning.py:159-176, models/models.py:44-58 DuelingHead) on the
// 512-wide projection: the dueling heads forward, the importance-weighted squared TD error on
// flat transitions, the heads' input gradient through GELU (dz) and the heads' weight-gradient
// partial -- one launch in the slot head_step_kernel (head.h) fills for IMPALA / PPO, one
// workgroup per block of DQN_F transitions.
//
//   q[n][k] = v[n] + adv[n][k] - mean_k adv[n][k]            (mean over the A real rows only)
//   err = target - q[a],  w = p^-beta / max_batch(p^-beta)   (w = 1 without probabilities)
//   loss = 1/2 mean(err^2 w);  new priority = |err|
//   d loss / d q[a] = dq = -err w / N;  d / d v = dq;  d / d adv_k = dq ([k == a] - 1 / A)
//
//   phase 1  stage h[F][512] and Wh[16][512] in LDS; heads = Wh . h + bh (MFMA; the four waves
//            split the two frame tiles and the two halves of K, halves summed in order)
//   phase 2  wave 0, one lane per transition: mean, q[a], err, w, the priorities, dH[F][32] in
//            LDS, the loss partial sums (fixed-order wave sums)
//   phase 3  dz[f][j] = gelu'(z[f][j]) * sum_o' dH[f][o'] Wh[o'][j]      (MFMA, K = 32)
//   phase 4  dWh[o'][j] partial = sum_f dH[f][o'] h[f][j]                (MFMA over transitions)
//            -> fp32 slab per workgroup (+ bias sums), reduced by reduce_grads
//
// Rows 0..A-1 of the 16-row heads packing are the advantage head, row 15 is v (net.h).  As in
// head.h: every global load is issued up front, unconditionally, with clamped rows; control flow
// is wave-uniform; reductions run in a fixed order and there are no float atomics, so a step is
// bitwise reproducible.
//
// The step kernel itself is csrc/dqn_head_step.h (it needs none of kernels.h, so a second
// translation unit can instantiate it: dqn_inplace.hip); the kernels below are the head's other
// entries.
#pragma once
#include "dqn_head_step.h"
#include "kernels.h"

__global__ void finalize_dqn_kernel(const float* part, int nparts, int N, float* metrics4) {
  if (threadIdx.x < 64) finalize_dqn_metrics(part, nparts, N, metrics4, (int)threadIdx.x, false);
}

// Standalone DQN loss head on given adv [N][A], v [N], one lane per transition (test / reuse
// entry; the counterpart of ppo_loss_head_kernel).
__global__ __launch_bounds__(256) void dqn_loss_head_kernel(
    const float* __restrict__ adv, const float* __restrict__ v, const int64_t* __restrict__ act,
    const float* __restrict__ tgt, const float* __restrict__ prob, int N, int A, float beta,
    float* __restrict__ dadv, float* __restrict__ dv, float* __restrict__ prio,
    float* __restrict__ partials) {
  __shared__ float red[4][4];
  __shared__ float pred[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 256 + threadIdx.x;
  const bool valid = n0 < N;
  const int n = valid ? n0 : N - 1;
  float hd[HEADS];
#pragma unroll
  for (int k = 0; k < MAX_A; ++k) hd[k] = adv[(size_t)n * A + min(k, A - 1)];
  hd[VCOL] = v[n];
  const int a = min((int)act[n], A - 1);
  const float t = tgt[n];
  float w = 1.f;
  if (prob) {  // (uniform branch)
    const float p = prob[n];
    w = dqn_weight(p, dqn_batch_pmin(prob, N, pred), beta);
  }
  const DqnTerm d = dqn_term(hd, a, A, t, w, 1.f / (float)N);
  if (valid) {
    const float da = -d.dq / (float)A;
#pragma unroll
    for (int k = 0; k < MAX_A; ++k)
      if (k < A) dadv[(size_t)n * A + k] = k == a ? d.dq + da : da;
    dv[n] = d.dq;
    prio[n] = fabsf(d.err);
  }
  float s[4] = {valid ? d.q : 0.f, valid ? t : 0.f, valid ? fabsf(d.err) : 0.f,
                valid ? d.err * d.err * d.w : 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partials[blockIdx.x * 8 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// heads output [n][16] (adv rows, v at 15) -> q [n][A]
__global__ void dqn_q_kernel(const float* __restrict__ heads, int n, int A, float* __restrict__ q) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  float l[HEADS];
#pragma unroll
  for (int j = 0; j < HEADS; j += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(heads + (size_t)f * HEADS + j);
    l[j] = x[0]; l[j + 1] = x[1]; l[j + 2] = x[2]; l[j + 3] = x[3];
  }
  float s = 0.f;
  for (int k = 0; k < A; ++k) s += l[k];
  const float mean = s / (float)A;
  for (int k = 0; k < A; ++k) q[(size_t)f * A + k] = (l[VCOL] + l[k]) - mean;
}

// AtariDQNModel.act (models/distributed_models.py:84-101), one thread per frame, on the online and
// target nets' heads outputs: greedy = argmax q_online (first maximal index, as torch.argmax); the
// action is drawn from pi (1 - eps on greedy, eps / (A - 1) on every other action) by inverse CDF
// on act_heads_kernel's counter-based uniform (seed, counter, frame); q_pi = q_online[action],
// q_star = q_target[greedy].  eps: per frame (eps_f) or one value.  A >= 2.
__global__ __launch_bounds__(256) void dqn_act_kernel(const float* __restrict__ heads_on,
                                                      const float* __restrict__ heads_tg, int n, int A,
                                                      const float* __restrict__ eps_f, float eps_all,
                                                      uint64_t seed, uint64_t counter,
                                                      int64_t* __restrict__ actions,
                                                      float* __restrict__ q_pi, float* __restrict__ q_star,
                                                      int64_t* __restrict__ greedy_out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  float lo[HEADS], lt[HEADS];
#pragma unroll
  for (int j = 0; j < HEADS; j += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(heads_on + (size_t)f * HEADS + j);
    const f32x4 y = *reinterpret_cast<const f32x4*>(heads_tg + (size_t)f * HEADS + j);
    lo[j] = x[0]; lo[j + 1] = x[1]; lo[j + 2] = x[2]; lo[j + 3] = x[3];
    lt[j] = y[0]; lt[j + 1] = y[1]; lt[j + 2] = y[2]; lt[j + 3] = y[3];
  }
  float so = 0.f, st = 0.f;
  for (int k = 0; k < A; ++k) { so += lo[k]; st += lt[k]; }
  const float mo = so / (float)A, mt = st / (float)A;
  float qo[MAX_A];
  float best = (lo[VCOL] + lo[0]) - mo;
  int g = 0;
#pragma unroll
  for (int k = 0; k < MAX_A; ++k) {
    qo[k] = (lo[VCOL] + lo[k]) - mo;
    if (k < A && qo[k] > best) { best = qo[k]; g = k; }
  }
  const float eps = eps_f ? eps_f[f] : eps_all;
  const float pg = 1.f - eps, po = eps / (float)(A - 1);
  const uint64_t r = act_mix64(act_mix64(seed ^ act_mix64(counter)) + (uint64_t)f);
  const float u = (float)(uint32_t)(r >> 40) * (1.f / 16777216.f);  // [0, 1)
  // a draw past the rounded total falls on the last action of nonzero probability
  int act = pg > 0.f ? g : (g == A - 1 ? A - 2 : A - 1);
  float c = 0.f;
  bool done = false;
#pragma unroll
  for (int k = 0; k < MAX_A; ++k) {
    if (k < A && !done) {
      c += k == g ? pg : po;
      if (u < c) { act = k; done = true; }
    }
  }
  float qa = qo[0], qs = 0.f;
#pragma unroll
  for (int k = 0; k < MAX_A; ++k) {
    qa = k == act ? qo[k] : qa;
    qs = k == g ? (lt[VCOL] + lt[k]) - mt : qs;
  }
  actions[f] = act;
  q_pi[f] = qa;
  q_star[f] = qs;
  if (greedy_out) greedy_out[f] = g;
}
