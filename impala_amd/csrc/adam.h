// clip_grad_norm_ + torch.optim.Adam on the flat parameter buffer and the re-emission of the
// kernel-layout ("shadow") weights, with what they alone need, free of non-template kernels, so
// that more than one translation unit can instantiate them (kernels.h: adam_kernel for the
// learners of impala.hip; iqn.hip: the same body on the IQN flat order, which has a segment
// inserted in the middle of the dueling net's).
#pragma once
#include "../../include/impala_hip.h"
#include "adam_args.h"
#include "common.h"
#include "conv1.h"
#include "net.h"

using namespace net;

// =========================================================================================
// Shadow-weight emission: canonical (state_dict) index -> kernel layouts (see net.h).
// =========================================================================================
template <typename T, int HID>
DEV void write_shadow(const ShadowPtrs& sp, const Canon& cn, const Shadow& sh, size_t i, float p) {
  using Vecs = VecsT<HID>;
  T* w = reinterpret_cast<T*>(sp.base);
  float* vv = sp.vecs;
  const T pt = (T)p;
  if (i < cn.b1) {
    const int k = (int)i, oc = k / K1, rem = k - oc * K1;
    w[sh.w1 + oc * K1 + c1_kprime(rem >> 6, (rem >> 3) & 7, rem & 7)] = pt;
  } else if (i < cn.w2) {
    vv[Vecs::b1 + (i - cn.b1)] = p;
  } else if (i < cn.b2) {
    const int k = (int)(i - cn.w2), oc = k / K2, rem = k % K2, ci = rem >> 4, kh = (rem >> 2) & 3,
              kw = rem & 3;
    w[sh.w2 + oc * K2 + (kh * 4 + kw) * OC1 + ci] = pt;
    if constexpr (sizeof(T) == 4) w[sh.w2t + w2t_index(oc, kh, kw, ci)] = pt;
  } else if (i < cn.w3) {
    vv[Vecs::b2 + (i - cn.b2)] = p;
  } else if (i < cn.b3) {
    const int k = (int)(i - cn.w3), oc = k / K3, rem = k % K3, ci = rem / 9, tap = rem % 9;
    w[sh.w3 + oc * K3 + tap * OC2 + ci] = pt;
    if constexpr (sizeof(T) == 4) w[sh.w3t + w3t_index(oc, tap, ci)] = pt;
  } else if (i < cn.lng) {
    vv[Vecs::b3 + (i - cn.b3)] = p;
  } else if (i < cn.lnb) {
    const int j = (int)(i - cn.lng);
    vv[Vecs::lng + (j & 15) * OC3 + (j >> 4)] = p;
  } else if (i < cn.wfc) {
    const int j = (int)(i - cn.lnb);
    vv[Vecs::lnb + (j & 15) * OC3 + (j >> 4)] = p;
  } else if (i < cn.bfc) {
    const int k = (int)(i - cn.wfc), o = k >> 10, j = k & 1023;
    const int jj = (j & 15) * OC3 + (j >> 4);
    w[sh.wfc + (size_t)o * FLAT + jj] = pt;
  } else if (i < cn.wa) {
    vv[Vecs::bfc + (i - cn.bfc)] = p;
  } else if (i < cn.ba) {
    const int k = (int)(i - cn.wa), ar = k >> hid_log2<HID>(), j = k & (HID - 1);
    w[sh.wh + ar * HID + j] = pt;
    w[sh.wht + j * HPAD + ar] = pt;
  } else if (i < cn.wc) {
    vv[Vecs::bh + (i - cn.ba)] = p;
  } else if (i < cn.bc) {
    const int j = (int)(i - cn.wc);
    w[sh.wh + VCOL * HID + j] = pt;
    w[sh.wht + j * HPAD + VCOL] = pt;
  } else {
    vv[Vecs::bh + VCOL] = p;
  }
}

// torch Adam's step size lr / (1 - b1^t) and sqrt(1 - b2^t) for step t (double, as torch's
// python scalars), rounded to fp32
DEV void adam_step_scalars(double lr, double b1, double b2, int64_t t, float& step_size, float& bc2s) {
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  step_size = (float)(lr / bc1);
  bc2s = (float)sqrt(bc2);
}

// =========================================================================================
// clip_grad_norm_(max_norm) + torch.optim.Adam (agents/impala/learning.py:172-176,
// builder.py:43-44), then re-emission of the kernel-layout weights.  Every block re-sums
// the sum-of-squares partials itself (deterministic, no grid barrier).
// =========================================================================================
// impala_set_metrics_host: the word of the 16-float host row the Adam kernel sets last
constexpr int kMetricsHostFlag = 15;
// torch.optim.Adam's update of one element (lerp form of exp_avg, sqrt(v) / sqrt(bc2) + eps),
// on the clipped gradient g * gscale
DEV void adam_elem(const AdamArgs& a, float gscale, float step_size, float bc2s, float& g,
                   float& m, float& v, float& p) {
  // every multiply and add rounded on its own, as written: no FMA contraction, whose choice
  // depends on the surrounding code
#pragma clang fp contract(off)
  const float w1 = (float)(1.0 - a.b1), b2f = (float)a.b2, w2 = (float)(1.0 - a.b2);
  g = g * gscale;
  m = m + w1 * (g - m);
  v = v * b2f + w2 * g * g;
  const float denom = sqrtf(v) / bc2s + a.eps;
  p = p - step_size * (m / denom);
}

// flat_at(fm, i): where index i of the handle's own (Canon) order lies in the caller's flat buffers
// (adam_args.h: FlatId, FlatGap).  gap and ins are multiples of 4, so an aligned group of four never
// straddles the insertion.
DEV size_t flat_at(const FlatId&, size_t i) { return i; }
DEV size_t flat_at(const FlatGap& m, size_t i) { return i < m.gap ? i : i + m.ins; }

// the clip norm as adam_body forms it (the same loads, sums and order), for a kernel that updates
// parameters outside the Canon order (iqn.hip: the inserted segment).  By every thread of a
// 256-thread workgroup; `red` is 4 floats of LDS; holds a barrier.
DEV float adam_grad_norm(const AdamArgs& a, float* red) {
  float sq = 0.f;
  const int nq = (a.n_part + 3) / 4;
  for (int q0 = threadIdx.x; q0 < nq; q0 += 256 * 4) {
    f32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(a.sumsq_part + 4 * min(q0 + 256 * j, nq - 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) sq += q0 + 256 * j < nq ? (x[j][0] + x[j][1]) + (x[j][2] + x[j][3]) : 0.f;
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  return sqrtf(red[0] + red[1] + red[2] + red[3]) * a.inv_world;
}

// clip + Adam on 4 consecutive parameters per thread; re-emits the kernel-layout weights.
// Blocks [0, HID) each own one row o of the FC weight (canonical [wfc + o*FLAT, +FLAT): 64% of
// the parameters) and re-emit its kernel-layout row (jj = p*64 + c for canonical j = c*16 + p)
// through LDS as one 16-byte (fp32) / 8-byte (bf16) store per thread: the per-element
// scattered stores of write_shadow cost the step ~3 us (knock-outs in
// profiles/r05tail).  Blocks [HID, ..) take the other parameters, one per thread in canonical
// order with the FC rows skipped.  fm: where a Canon index lies in the flat buffers.
static_assert((OC1 * K1 + OC1 + OC2 * K2 + OC2 + OC3 * K3 + OC3 + 2 * FLAT) % 4 == 0,
              "adam_kernel: the FC weight rows start float4-aligned in the canonical buffer");
template <typename T, int HID, class FM>
DEV void adam_body(const AdamArgs& a, const FM fm) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) T fcrow[FLAT];
  // this thread's 4 parameters, the step scalars and the norm partials are all loaded up
  // front (one memory round trip), then one barrier combines the norm
  const bool fc = blockIdx.x < HID;
  size_t i0;
  if (fc) {
    i0 = a.cn.wfc + (size_t)blockIdx.x * FLAT + threadIdx.x * 4;
  } else {  // one parameter per thread: the scattered shadow stores of write_shadow (two per
            // conv2 / conv3 weight in fp32) spread over 4x the waves (profiles/r05tail)
    const size_t e = (size_t)(blockIdx.x - HID) * 256 + threadIdx.x;
    i0 = e < a.cn.wfc ? e : e + (a.cn.bfc - a.cn.wfc);
  }
  const int n = i0 < a.cn.total ? (fc ? 4 : 1) : 0;
  float g[4], m[4], v[4], p[4];
  if (n == 4) {
    const f32x4 G = *reinterpret_cast<const f32x4*>(a.grads + flat_at(fm, i0));
    const f32x4 M = *reinterpret_cast<const f32x4*>(a.m + flat_at(fm, i0));
    const f32x4 Vv = *reinterpret_cast<const f32x4*>(a.v + flat_at(fm, i0));
    const f32x4 P = *reinterpret_cast<const f32x4*>(a.params + flat_at(fm, i0));
#pragma unroll
    for (int k = 0; k < 4; ++k) { g[k] = G[k]; m[k] = M[k]; v[k] = Vv[k]; p[k] = P[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = k < n;
      g[k] = ok ? a.grads[flat_at(fm, i0) + k] : 0.f; m[k] = ok ? a.m[flat_at(fm, i0) + k] : 0.f;
      v[k] = ok ? a.v[flat_at(fm, i0) + k] : 0.f;     p[k] = ok ? a.params[flat_at(fm, i0) + k] : 0.f;
    }
  }
  const float step_size = a.sc[0], bc2s = a.sc[1];
  const int64_t step = a.step[0];  // for metrics[7] (block 0), loaded with everything else
  float sq = 0.f;  // partials are zero-padded to a multiple of 4 (see impala_create)
  // 4 float4 partial loads in flight per thread (unconditional, clamped; out-of-range ones
  // dropped by a select), same summation order as one at a time
  const int nq = (a.n_part + 3) / 4;
  for (int q0 = threadIdx.x; q0 < nq; q0 += 256 * 4) {
    f32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(a.sumsq_part + 4 * min(q0 + 256 * j, nq - 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) sq += q0 + 256 * j < nq ? (x[j][0] + x[j][1]) + (x[j][2] + x[j][3]) : 0.f;
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  const float norm = sqrtf(red[0] + red[1] + red[2] + red[3]) * a.inv_world;
  const float coef = fminf(a.max_norm / (norm + 1e-6f), 1.f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.metrics[6] = norm;
    a.metrics[7] = (float)step;
  }
  if (a.metrics_host && blockIdx.x == 0 && threadIdx.x == 0) {
    // the whole vector (slots other than 6 and 7 were final when the reduction kernel ended) to
    // host memory with system-scope stores, then a nonzero word at [15] after a system fence:
    // the caller (which zeroed that word before enqueueing the step) may read the vector as soon
    // as it sees the word -- before this kernel's other workgroups have finished -- or after an
    // event recorded behind the step (no device-to-host copy on the stream either way)
    unsigned* out = reinterpret_cast<unsigned*>(a.metrics_host);
    float x[IMPALA_NUM_METRICS];  // every load issued before the first store
#pragma unroll
    for (int i = 0; i < IMPALA_NUM_METRICS; ++i) x[i] = i == 6 ? norm : i == 7 ? (float)step : a.metrics[i];
#pragma unroll
    for (int i = 0; i < IMPALA_NUM_METRICS; ++i)
      __hip_atomic_store(out + i, __float_as_uint(x[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(out + kMetricsHostFlag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (n == 0) return;  // (never an FC block: those are full)
  const float gscale = a.inv_world * coef;
#pragma unroll
  for (int k = 0; k < 4; ++k) adam_elem(a, gscale, step_size, bc2s, g[k], m[k], v[k], p[k]);
  if (n == 4) {
    *reinterpret_cast<f32x4*>(a.grads + flat_at(fm, i0)) = f32x4{g[0], g[1], g[2], g[3]};
    *reinterpret_cast<f32x4*>(a.m + flat_at(fm, i0)) = f32x4{m[0], m[1], m[2], m[3]};
    *reinterpret_cast<f32x4*>(a.v + flat_at(fm, i0)) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(a.params + flat_at(fm, i0)) = f32x4{p[0], p[1], p[2], p[3]};
  } else {
    for (int k = 0; k < n; ++k) {
      a.grads[flat_at(fm, i0) + k] = g[k]; a.m[flat_at(fm, i0) + k] = m[k]; a.v[flat_at(fm, i0) + k] = v[k]; a.params[flat_at(fm, i0) + k] = p[k];
    }
  }
  if (fc) {
    // canonical j = 4 tid + k = c*16 + q  ->  kernel-layout jj = q*64 + c (write_shadow's RK_FC)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = 4 * (int)threadIdx.x + k;
      fcrow[(j & 15) * OC3 + (j >> 4)] = (T)p[k];
    }
    __syncthreads();
    T* w = reinterpret_cast<T*>(a.sp.base) + a.sh.wfc + (size_t)blockIdx.x * FLAT + 4 * threadIdx.x;
    if constexpr (sizeof(T) == 4)
      *reinterpret_cast<f32x4*>(w) = *reinterpret_cast<const f32x4*>(fcrow + 4 * threadIdx.x);
    else
      *reinterpret_cast<uint2*>(w) = *reinterpret_cast<const uint2*>(fcrow + 4 * threadIdx.x);
  } else {
    for (int k = 0; k < n; ++k) write_shadow<T, HID>(a.sp, a.cn, a.sh, i0 + k, p[k]);
  }
}
