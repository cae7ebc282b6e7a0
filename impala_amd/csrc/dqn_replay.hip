// Kernels of the device-side prioritized replay (include/dqn_hip.h, dqn_replay_*) and their
// launchers (csrc/dqn_replay_launch.h).  A translation unit of its own, so the code object of
// impala.hip -- the learner steps' kernels and where they sit in it -- is the same with or
// without the replay; the host side is csrc/dqn_replay.h, included at the end of impala.hip.
//
// Sampling is two launches.  replay_block_sum_kernel: one wavefront per block of
// DQN_REPLAY_BLOCK = 512 rows, 8 consecutive float64 weights per lane summed in order, the 64
// lane sums by a fixed butterfly (DPP and permlane swaps, no LDS).  replay_draw_kernel: every
// workgroup scans the <= 4096 block sums into LDS (thread t walks `chunk` consecutive sums, one
// thread walks the threads' totals: sequential additions only, so the prefix never decreases),
// then one wavefront per draw binary-searches its block and finds the row inside it with a
// wave-wide prefix -- the lanes' sums shifted one lane at a time, as seq_fwd_scan (kernels.h)
// does.  The ring's weights change only where a priority is written, so no pow runs here.
#include "common.h"

#include "../../include/dqn_hip.h"
#include "dqn_replay_launch.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- float64 lane moves: the two dwords through the float helpers' DPP / permlane swaps ----
template <int CTRL> DEV double dppd(double v) {  // lanes without a source read 0.0
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
DEV double swap16_sum_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  uint32_t la = (uint32_t)b, lb = la, ha = (uint32_t)(b >> 32), hb = ha;
  swap16(la, lb);
  swap16(ha, hb);
  return __builtin_bit_cast(double, (uint64_t)la | ((uint64_t)ha << 32)) +
         __builtin_bit_cast(double, (uint64_t)lb | ((uint64_t)hb << 32));
}
DEV double swap32_sum_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  uint32_t la = (uint32_t)b, lb = la, ha = (uint32_t)(b >> 32), hb = ha;
  swap32(la, lb);
  swap32(ha, hb);
  return __builtin_bit_cast(double, (uint64_t)la | ((uint64_t)ha << 32)) +
         __builtin_bit_cast(double, (uint64_t)lb | ((uint64_t)hb << 32));
}
// symmetric pairs only: every lane ends with the bit-identical sum (as wave_sum)
DEV double wave_sum_f64(double v) {
  v += dppd<DPP_QP_1032>(v);
  v += dppd<DPP_QP_2301>(v);
  v += dppd<DPP_ROW_HALF_MIRROR>(v);
  v += dppd<DPP_ROW_MIRROR>(v);
  return swap32_sum_f64(swap16_sum_f64(v));
}
// E_lane = tot_0 + ... + tot_{lane-1}, added in lane order (63 one-lane shifts)
DEV double seq_excl_scan_f64(double tot, int lane) {
  double E = 0.0;
  for (int k = 0; k < WAVE - 1; ++k) {
    const double p = dppd<DPP_WAVE_SHR1>(E + tot);
    E = lane >= 1 ? p : 0.0;
  }
  return E;
}

// a lane's 8 consecutive weights of block `blk`; rows >= size read as 0
DEV void load_block_lane(const double* __restrict__ w, long long blk, long long size, int lane, double x[8]) {
  const long long i0 = blk * DQN_REPLAY_BLOCK + lane * 8;
  if (i0 + 8 <= size) {
    const f64x2* p = reinterpret_cast<const f64x2*>(w + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f64x2 v = p[k];
      x[2 * k] = v[0];
      x[2 * k + 1] = v[1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = i0 + k < size ? w[i0 + k] : 0.0;
  }
}

__global__ __launch_bounds__(256) void replay_block_sum_kernel(const double* __restrict__ w, long long size,
                                                               int nb, double* __restrict__ bsum) {
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nb) return;  // (whole wavefronts)
  double x[8];
  load_block_lane(w, blk, size, lane, x);
  double s = x[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) s += x[k];
  s = wave_sum_f64(s);
  if (lane == 0) bsum[blk] = s;
}

DEV double replay_uniform(uint64_t seed, uint64_t counter, uint64_t j) {
  const uint64_t r = act_mix64(act_mix64(seed ^ act_mix64(counter)) + j);
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);  // [0, 1)
}

// smallest b in [0, nb) with P[b] > x (GE: >= x); nb when there is none
template <bool GE> DEV int replay_lower_bound(const double* P, int nb, double x) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool past = GE ? P[mid] >= x : P[mid] > x;
    if (past) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// dynamic LDS: nb doubles (the block sums' inclusive prefix) + 256 (the scan threads' offsets)
__global__ __launch_bounds__(256) void replay_draw_kernel(const double* __restrict__ w,
                                                          const double* __restrict__ bsum, long long size,
                                                          int nb, int chunk, uint64_t seed, uint64_t counter,
                                                          int n, int64_t* __restrict__ keys,
                                                          float* __restrict__ prob) {
  extern __shared__ double replay_lds[];
  double* P = replay_lds;
  double* off = replay_lds + nb;
  const int tid = threadIdx.x, lane = tid & 63;
  {
    const int b0 = tid * chunk, b1 = min(nb, b0 + chunk);
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) {
      acc += bsum[b];
      P[b] = acc;
    }
    off[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      const int T = (nb + chunk - 1) / chunk;
      double run = 0.0;
      for (int t = 0; t < T; ++t) {
        const double o = run;
        run += off[t];
        off[t] = o;
      }
    }
    __syncthreads();
    const double o = off[tid];
    for (int b = b0; b < b1; ++b) P[b] = o + P[b];
    __syncthreads();
  }
  const int j = blockIdx.x * 4 + (tid >> 6);
  if (j >= n) return;  // (whole wavefronts, after the last barrier)
  const double total = P[nb - 1];
  const double u = replay_uniform(seed, counter, (uint64_t)j);
  if (!(total > 0.0)) {
    if (lane == 0) {
      long long k = (long long)(u * (double)size);
      keys[j] = k < size - 1 ? k : size - 1;
      prob[j] = (float)(1.0 / (double)size);
    }
    return;
  }
  const double target = u * total;
  int blk = replay_lower_bound<false>(P, nb, target);
  double r = 0.0;
  bool past = false;
  if (blk == nb) {  // u * total rounded up to the total: the last block of positive sum
    blk = replay_lower_bound<true>(P, nb, total);
    past = true;
  } else {
    r = target - (blk > 0 ? P[blk - 1] : 0.0);
  }
  double x[8], q[8];
  load_block_lane(w, blk, size, lane, x);
  q[0] = x[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) q[k] = q[k - 1] + x[k];
  const double E = seq_excl_scan_f64(q[7], lane);
  int first = -1, last = -1;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    if (x[k] > 0.0 && E + q[k] > r) first = k;
    if (x[k] > 0.0 && last < 0) last = k;
  }
  const unsigned long long hit = past ? 0ull : __ballot(first >= 0);
  const unsigned long long live = __ballot(last >= 0);
  int src_lane, k;
  if (hit) {
    src_lane = __builtin_ctzll(hit);
    k = first;
  } else {  // the residual is past the block's rounded prefix: its last row of positive weight
    src_lane = 63 - __builtin_clzll(live | 1ull);
    k = last < 0 ? 0 : last;
  }
  if (lane == src_lane) {
    double wk = x[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) wk = i == k ? x[i] : wk;
    keys[j] = (long long)blk * DQN_REPLAY_BLOCK + lane * 8 + k;
    prob[j] = (float)(wk / total);
  }
}

// priority ** alpha in float64.  alpha == 1 is the priority itself: the device pow(x, 1.0) is
// within 1e-14 rel of x but not always x, and at that exponent the weights are exact numbers whose
// sums do not depend on the order (tests/test_gpu_dqn_replay_scale.py draws on that).
DEV double replay_weight(float p, double alpha) { return alpha == 1.0 ? (double)p : pow((double)p, alpha); }

DEV float block_max_256(float m, float* red) {  // every thread of a 256-multiple workgroup calls it
  m = wave_max(m);
  const int nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; ++i) r = fmaxf(r, red[i]);
  return r;
}

// One workgroup: phase 1 stores the priorities, phase 2 re-reads priorities[key] and stores the
// weight of what it read, so duplicate keys leave weights[key] == pow(priorities[key], alpha)
// whichever value landed.  Keys outside [0, cap) are skipped.
__global__ __launch_bounds__(256) void replay_update_kernel(const int64_t* __restrict__ keys,
                                                            const float* __restrict__ pin, int n,
                                                            long long cap, double alpha, float* prio,
                                                            double* __restrict__ w, float* maxp) {
  __shared__ float red[4];
  float m = 0.f;
  for (int j = threadIdx.x; j < n; j += 256) {
    const long long k = keys[j];
    if (k < 0 || k >= cap) continue;
    const float p = pin[j];
    prio[k] = p;
    m = fmaxf(m, p);
  }
  __threadfence();
  m = block_max_256(m, red);  // (its barrier separates the phases)
  for (int j = threadIdx.x; j < n; j += 256) {
    const long long k = keys[j];
    if (k < 0 || k >= cap) continue;
    const float p = *(volatile const float*)(prio + k);
    w[k] = replay_weight(p, alpha);
  }
  if (threadIdx.x == 0) *maxp = fmaxf(*maxp, m);
}

// One thread per appended row: the small fields, the priority and the weight (obs rows travel by
// device copies).  pin null: every row takes the running maximum.  The kernel only reads *maxp;
// replay_raise_max_kernel, the next launch on the stream, raises it.
__global__ __launch_bounds__(256) void replay_extend_kernel(const int64_t* __restrict__ act,
                                                            const float* __restrict__ tgt,
                                                            const float* __restrict__ pin, long long n,
                                                            long long cursor, long long cap, double alpha,
                                                            int64_t* __restrict__ r_act, float* __restrict__ r_tgt,
                                                            float* __restrict__ r_prio, double* __restrict__ w,
                                                            const float* __restrict__ maxp,
                                                            int64_t* __restrict__ keys_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long k = (cursor + i) % cap;
  r_act[k] = act[i];
  r_tgt[k] = tgt[i];
  const float p = pin ? pin[i] : *maxp;
  r_prio[k] = p;
  w[k] = replay_weight(p, alpha);
  if (keys_out) keys_out[i] = k;
}

// One thread per transition: ApexActor._async_make_replay's targets and priorities for K = L - 1
// transitions.  *maxp is left to replay_raise_max_kernel.
__global__ __launch_bounds__(256) void replay_rollout_kernel(const int64_t* __restrict__ act,
                                                             const float* __restrict__ rew,
                                                             const uint8_t* __restrict__ done,
                                                             const float* __restrict__ q_pi,
                                                             const float* __restrict__ q_star, long long K,
                                                             int n_step, float gamma, long long cursor,
                                                             long long cap, double alpha, int64_t* __restrict__ r_act,
                                                             float* __restrict__ r_tgt, float* __restrict__ r_prio,
                                                             double* __restrict__ w, int64_t* __restrict__ keys_out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= K) return;
  const long long mm = min((long long)n_step, K - t);
  float acc = q_star[t + mm];  // v_{t+m-1}
  for (long long k = t + mm - 1; k >= t; --k) {
    const float d = done[k] ? 0.f : gamma;  // gamma (1 - done), exactly
    acc = fmaf(d, acc, rew[k]);             // one rounding per step
  }
  const float p = fabsf(acc - q_pi[t]);
  const long long k = (cursor + t) % cap;
  r_act[k] = act[t];
  r_tgt[k] = acc;
  r_prio[k] = p;
  w[k] = replay_weight(p, alpha);
  if (keys_out) keys_out[t] = k;
}

// One workgroup (the one writer of *maxp): the maximum of the n ring priorities just written at
// (cursor + i) % cap, one float load per row, then one store.
__global__ __launch_bounds__(1024) void replay_raise_max_kernel(const float* __restrict__ r_prio, long long n,
                                                                long long cursor, long long cap, float* maxp) {
  __shared__ float red[16];
  float m = *maxp;
  const long long first = n < cap - cursor ? n : cap - cursor;  // rows before the wrap
  for (long long i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, r_prio[i < first ? cursor + i : i - first]);
  m = block_max_256(m, red);  // (every thread read *maxp before this barrier)
  if (threadIdx.x == 0) *maxp = m;
}

}  // namespace

namespace dqn_replay_dev {

hipError_t launch_block_sum(const double* w, long long size, int nb, double* bsum, hipStream_t st) {
  replay_block_sum_kernel<<<(nb + 3) / 4, 256, 0, st>>>(w, size, nb, bsum);
  return hipGetLastError();
}

hipError_t launch_draw(const double* w, const double* bsum, long long size, int nb, int chunk, uint64_t seed,
                       uint64_t counter, int n, int64_t* keys, float* prob, hipStream_t st) {
  const size_t lds = ((size_t)nb + 256) * sizeof(double);
  replay_draw_kernel<<<(n + 3) / 4, 256, lds, st>>>(w, bsum, size, nb, chunk, seed, counter, n, keys, prob);
  return hipGetLastError();
}

hipError_t launch_update(const int64_t* keys, const float* pin, int n, long long cap, double alpha, float* prio,
                         double* w, float* maxp, hipStream_t st) {
  replay_update_kernel<<<1, 256, 0, st>>>(keys, pin, n, cap, alpha, prio, w, maxp);
  return hipGetLastError();
}

hipError_t launch_extend(const int64_t* act, const float* tgt, const float* pin, long long n, long long cursor,
                         long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                         float* maxp, int64_t* keys_out, hipStream_t st) {
  replay_extend_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(act, tgt, pin, n, cursor, cap, alpha, r_act,
                                                                    r_tgt, r_prio, w, maxp, keys_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !pin) return e;  // rows at the running maximum do not raise it
  replay_raise_max_kernel<<<1, 1024, 0, st>>>(r_prio, n, cursor, cap, maxp);
  return hipGetLastError();
}

hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* q_pi,
                          const float* q_star, long long K, int n_step, float gamma, long long cursor,
                          long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                          float* maxp, int64_t* keys_out, hipStream_t st) {
  replay_rollout_kernel<<<(unsigned)((K + 255) / 256), 256, 0, st>>>(act, rew, done, q_pi, q_star, K, n_step,
                                                                     gamma, cursor, cap, alpha, r_act, r_tgt,
                                                                     r_prio, w, keys_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  replay_raise_max_kernel<<<1, 1024, 0, st>>>(r_prio, K, cursor, cap, maxp);
  return hipGetLastError();
}

hipError_t launch_raise_max(const float* r_prio, long long n, long long cursor, long long cap, float* maxp,
                            hipStream_t st) {
  replay_raise_max_kernel<<<1, 1024, 0, st>>>(r_prio, n, cursor, cap, maxp);
  return hipGetLastError();
}

}  // namespace dqn_replay_dev
