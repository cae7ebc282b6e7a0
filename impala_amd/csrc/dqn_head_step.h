// The Ape-X DQN head's step kernel (csrc/dqn_head.h has the description and the head's other
// kernels): dqn_head_step_kernel with what it alone needs, free of non-template kernels, so that
// more than one translation unit can instantiate it (impala.hip for a batch, dqn_inplace.hip for
// a replay ring read in place).
#pragma once
#include "conv1.h"
#include "gemm.h"
#include "net.h"

using namespace net;

// transitions per workgroup.  LDS at fp32: h 32 x 516 x 4 = 66 KB, Wh 16 x 516 x 4 = 33 KB, the z
// slice 8.7 KB, dH 4.6 KB: 113 KB of the CU's 160 KB (64 rows would need 179 KB)
constexpr int DQN_F = 32;
// workgroups per transition block (hidden-column slices of phases 3 / 4): 64 columns each, one
// 16-column tile per wave
constexpr int DQN_SPLIT = 8;

struct DqnHeadArgs {
  const void* h;      // T [N][512]
  const float* zg;    // [N][512] gelu'(pre-GELU), from the FC forward
  const void* wh;     // T [16][512]
  const void* wht;    // T [512][32]
  const float* bh;    // [16]
  const int64_t* act; // [N]
  const float* tgt;   // [N]
  const float* prob;  // [N] sampling probabilities, or null (w = 1)
  int N, A;
  float beta;         // importance-sampling exponent
  void* dz;           // T [N][512]
  float* partials;    // [gridDim.x][8]: sums of q[a], target, |err|, err^2 w
  float* slab_h;      // [gridDim.x][16][512]
  float* slab_bh;     // [gridDim.x][16]
  float* prio;        // [N] out: |err|
};

// min over the batch of the sampling probabilities, by every thread of a 256-thread workgroup:
// p^-beta is decreasing in p, so max_batch(p^-beta) = (min_batch p)^-beta.  (A minimum does not
// depend on the order it is taken in.)  `red` is 4 floats of LDS; ends with a barrier.
DEV float dqn_batch_pmin(const float* __restrict__ prob, int N, float* red) {
  float m = INFINITY;
  for (int i0 = threadIdx.x; i0 < N; i0 += 256 * 4) {
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = prob[min(i0 + 256 * j, N - 1)];  // clamped: a real element
#pragma unroll
    for (int j = 0; j < 4; ++j) m = fminf(m, x[j]);
  }
  m = -wave_max(-m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// one transition's loss terms from its 16-row heads output (adv rows 0..A-1, v at VCOL)
struct DqnTerm {
  float q, err, w, dq;
};
DEV DqnTerm dqn_term(const float (&hd)[HEADS], int a, int A, float tgt, float w, float inv_n) {
  float s = 0.f, adv_a = 0.f;
#pragma unroll
  for (int k = 0; k < MAX_A; ++k) {  // padded rows A..14 stay out of the mean
    s += k < A ? hd[k] : 0.f;
    adv_a = k == a ? hd[k] : adv_a;
  }
  DqnTerm t;
  t.q = (hd[VCOL] + adv_a) - s / (float)A;
  t.err = tgt - t.q;
  t.w = w;
  t.dq = -(t.err * w) * inv_n;
  return t;
}
// w = p^-beta / max_batch(p^-beta)
DEV float dqn_weight(float p, float pmin, float beta) { return powf(p, -beta) / powf(pmin, -beta); }

// fm: which row of act / tgt holds transition f (conv1.h: ObsDirect for a batch, ObsKeys for a
// replay ring read in place); prob, prio, h, z and dz are indexed by transition either way.
// The body of the two kernels below.  dqn_head_step_kernel keeps its name and its one argument:
// a longer mangled name grows the code object's symbol tables, which moved every kernel of
// impala.hip by 1 KB, and the IMPALA headline rose 0.25 % (fp32) and 0.4 % (bf16) in 7 of 8
// alternating pairs (profiles/dqn_inplace/ab.txt, block 1).
template <typename T, class O>
DEV void dqn_head_step_body(const DqnHeadArgs a, const O fm) {
  constexpr int HID = HID_DQN, FR = DQN_F;
  constexpr int JC = HID / DQN_SPLIT;  // hidden columns per workgroup in phases 3 / 4
  static_assert(JC == 64 && FR == 32, "phase 1 / 3 / 4 wave maps: 4 column tiles, 2 frame tiles");
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int LDH = HID + VEC;   // h / Wh tile row (elements)
  constexpr int LDD = HPAD + VEC;  // dH tile row
  constexpr int LDZ = JC + 4;
  __shared__ __attribute__((aligned(16))) T hs[FR * LDH];
  __shared__ __attribute__((aligned(16))) T whs[HEADS * LDH];
  __shared__ __attribute__((aligned(16))) T dHs[FR * LDD];
  __shared__ __attribute__((aligned(16))) float zs[FR * LDZ];
  __shared__ float lg_s[FR][HEADS + 1];
  __shared__ f32x4 hp[2][64];  // phase 1: the second K half's partial tiles
  __shared__ float bred[4][HEADS];
  __shared__ float pred[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * FR;
  const int nf = min(FR, a.N - f0);  // valid transitions of this workgroup (>= 1)
  const int jw = blockIdx.y * JC;    // this workgroup's hidden-column slice
  const bool lead = blockIdx.y == 0; // writes the per-block outputs
  const int A = a.A;
  const T* hg = reinterpret_cast<const T*>(a.h);
  // ---- every global load, up front and unconditional; rows past the block's transitions are
  // copies of its last one, which only meet zero dH rows or outputs nobody stores ----
  const int fl = min(lane, nf - 1);  // phase 2: this lane's transition (wave 0)
  const size_t row_l = fm.map((size_t)(f0 + fl));  // (ObsKeys: the one key load, f0 + fl < N)
  const int act_l = reinterpret_cast<const int*>(a.act)[2 * row_l];  // low word: in [0, A)
  const float tgt_l = a.tgt[row_l];
  const float* pp = a.prob ? a.prob : a.tgt;  // (unused values without probabilities)
  const float p_l = pp[f0 + fl];
  constexpr int NHV = FR * (HID / VEC) / 256, NZV = FR * (JC / 4) / 256;
  constexpr int NWV = HEADS * (HID / VEC) / 256;
  constexpr int NKH = HID / F::KSTEP / 2, NKT = HPAD / F::KSTEP;  // k-steps of a K half / of dz
  const int kl = F::KPL * (lane >> 4);
  V hv[NHV], whv[NWV], wtf[NKT];
  f32x4 zv[NZV];
#pragma unroll
  for (int i = 0; i < NHV; ++i) {
    const int e = tid + i * 256, f = min(e / (HID / VEC), nf - 1), c = (e % (HID / VEC)) * VEC;
    hv[i] = *reinterpret_cast<const V*>(hg + (size_t)(f0 + f) * HID + c);
  }
#pragma unroll
  for (int i = 0; i < NZV; ++i) {
    const int e = tid + i * 256, f = min(e / (JC / 4), nf - 1), c = (e % (JC / 4)) * 4;
    zv[i] = *reinterpret_cast<const f32x4*>(a.zg + (size_t)(f0 + f) * HID + jw + c);
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
    // wave: frame tile wave & 1, K half wave >> 1; four accumulators over interleaved k-steps,
    // summed in a fixed order (head.h phase 1)
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
  // ---- phase 2: wave 0, one lane per transition ----
  if (wave == 0) {
    const bool valid = lane < nf;
    float hd[HEADS];
#pragma unroll
    for (int k = 0; k < HEADS; ++k) hd[k] = lg_s[fl][k];
    const int aa = min(act_l, A - 1);
    const float w = a.prob ? dqn_weight(p_l, pmin, a.beta) : 1.f;
    const DqnTerm t = dqn_term(hd, aa, A, tgt_l, w, 1.f / (float)a.N);
    if (valid) {
      const float da = -t.dq / (float)A;  // every advantage row's share of the mean
#pragma unroll
      for (int k = 0; k < MAX_A; ++k)
        if (k < A) dHs[lane * LDD + k] = (T)(k == aa ? t.dq + da : da);
      dHs[lane * LDD + VCOL] = (T)t.dq;
      if (lead) a.prio[f0 + lane] = fabsf(t.err);
    }
    float s[4] = {valid ? t.q : 0.f, valid ? tgt_l : 0.f, valid ? fabsf(t.err) : 0.f,
                  valid ? t.err * t.err * t.w : 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0 && lead) {
      float* po = a.partials + (size_t)blockIdx.x * 8;
#pragma unroll
      for (int k = 0; k < 4; ++k) po[k] = s[k];
    }
  }
  __syncthreads();
  // ---- phase 3: dz = gelu'(z) * (dH . Wh): wave -> column tile, both frame tiles ----
  {
    T* dz = reinterpret_cast<T*>(a.dz);
    const int j0 = jw + wave * 16;
#pragma unroll
    for (int ct = 0; ct < FR / 16; ++ct) {
      if (ct * 16 >= nf) break;  // a frame tile past the block's transitions (uniform)
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
        store4(dz + (size_t)(f0 + f) * HID + j, o);
      }
    }
  }
  // ---- phase 4: dWh partial = dH^T . h over the block's transitions (k = transition; the dH
  // rows past them are zero) ----
  {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = jw + wave * 16;
#pragma unroll
    for (int kk = 0; kk < FR; kk += F::KSTEP)
      acc = F::mma(lds_frag_k(dHs + kk * LDD, LDD, lane), lds_frag_k(hs + kk * LDH + c0, LDH, lane), acc);
    float* sl = a.slab_h + (size_t)blockIdx.x * HEADS * HID;
#pragma unroll
    for (int q = 0; q < 4; ++q) sl[(4 * (lane >> 4) + q) * HID + c0 + (lane & 15)] = acc[q];
    if (lead) {  // bias = sum over transitions of dH: 16 groups x 16 heads, fixed-order tree
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

// the step on a batch: act[f], tgt[f]
template <typename T>
__global__ __launch_bounds__(256) void dqn_head_step_kernel(const DqnHeadArgs a) {
  dqn_head_step_body<T>(a, ObsDirect{});
}
// the step on a replay ring read in place: act[keys[f]], tgt[keys[f]] (dqn_inplace.hip)
template <typename T>
__global__ __launch_bounds__(256) void dqn_head_step_keys_kernel(const DqnHeadArgs a, const ObsKeys fm) {
  dqn_head_step_body<T>(a, fm);
}
