// The two ingest kernels of the device-side IQN replay (include/iqn_hip.h, iqn_replay_*) and their
// launchers (csrc/iqn_replay_launch.h): a ring whose target rows are W floats wide.  A translation
// unit of its own, so no other code object changes with it; sampling, the priority update and the
// running maximum are csrc/dqn_replay.hip's kernels, reached through its launchers.  The host side
// is csrc/iqn_replay.h, included at the end of impala.hip.
//
// Both kernels store with plain vector stores, add in one fixed order and use no atomics: equal
// inputs give equal bits.  Neither writes *maxp; replay_raise_max_kernel, the next launch on the
// stream, raises it from the ring priorities just written.
#include "common.h"

#include "../../include/iqn_hip.h"
#include "iqn_replay_host.h"
#include "iqn_replay_launch.h"

namespace {

// priority ** alpha in float64, as csrc/dqn_replay.hip's replay_weight (alpha == 1: the priority)
DEV double iqn_replay_weight(float p, double alpha) { return alpha == 1.0 ? (double)p : pow((double)p, alpha); }

// One thread per target: row i / W of the append, column i % W.  The thread of column 0 also
// writes the row's action, its priority (pin null: the running maximum) and its float64 weight.
__global__ __launch_bounds__(256) void iqn_replay_extend_kernel(const int64_t* __restrict__ act,
                                                                const float* __restrict__ tgt,
                                                                const float* __restrict__ pin, long long n, int W,
                                                                long long cursor, long long cap, double alpha,
                                                                int64_t* __restrict__ r_act,
                                                                float* __restrict__ r_tgt,
                                                                float* __restrict__ r_prio, double* __restrict__ w,
                                                                const float* __restrict__ maxp,
                                                                int64_t* __restrict__ keys_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * W) return;
  const long long t = i / W;
  const int k = (int)(i - t * W);
  const long long row = (cursor + t) % cap;
  r_tgt[row * W + k] = tgt[i];
  if (k != 0) return;
  r_act[row] = act[t];
  const float p = pin ? pin[t] : *maxp;
  r_prio[row] = p;
  w[row] = iqn_replay_weight(p, alpha);
  if (keys_out) keys_out[t] = row;
}

// The fused ingest of one rollout: K = L - 1 transitions, `rows` whole transitions per workgroup,
// thread lr * W + k on column k of the workgroup's transition lr.  Column k is iqn_nstep_kernel's
// recurrence (csrc/iqn.hip): v = q_star[t + m][k], one fmaf per step.  The W targets of a transition
// meet in LDS, and its thread of column 0 adds them from 0 in k order -- iqn_nstep_prio_kernel's
// sum -- so the priority does not depend on W or on where the row sits in a wavefront.
__global__ __launch_bounds__(256) void iqn_replay_rollout_kernel(
    const int64_t* __restrict__ act, const float* __restrict__ rew, const uint8_t* __restrict__ done,
    const float* __restrict__ q_pi, const float* __restrict__ q_star, long long K, int W, int rows, int n_step,
    float gamma, long long cursor, long long cap, double alpha, int64_t* __restrict__ r_act,
    float* __restrict__ r_tgt, float* __restrict__ r_prio, double* __restrict__ w,
    int64_t* __restrict__ keys_out) {
  __shared__ float tg[256];
  const int tid = threadIdx.x;
  const int lr = tid / W, k = tid - lr * W;
  const long long t = (long long)blockIdx.x * rows + lr;
  const bool live = lr < rows && t < K;
  long long row = 0;
  if (live) {
    row = (cursor + t) % cap;
    const long long mm = min((long long)n_step, K - t);
    float acc = q_star[(t + mm) * W + k];  // v_{t+m-1}
    for (long long s = t + mm - 1; s >= t; --s) {
      const float d = done[s] ? 0.f : gamma;  // gamma (1 - done), exactly
      acc = fmaf(d, acc, rew[s]);             // one rounding per step
    }
    r_tgt[row * W + k] = acc;
    tg[tid] = acc;
  }
  __syncthreads();
  if (!live || k != 0) return;
  float s = 0.f;
  for (int j = 0; j < W; ++j) s += tg[tid + j];
  const float p = fabsf(s / (float)W - q_pi[t]);
  r_act[row] = act[t];
  r_prio[row] = p;
  w[row] = iqn_replay_weight(p, alpha);
  if (keys_out) keys_out[t] = row;
}

}  // namespace

namespace iqn_replay_dev {

hipError_t launch_extend(const int64_t* act, const float* tgt, const float* pin, long long n, int W,
                         long long cursor, long long cap, double alpha, int64_t* r_act, float* r_tgt,
                         float* r_prio, double* w, const float* maxp, int64_t* keys_out, hipStream_t st) {
  iqn_replay_extend_kernel<<<(unsigned)iqn_replay_host::extend_wgs(n, W), 256, 0, st>>>(
      act, tgt, pin, n, W, cursor, cap, alpha, r_act, r_tgt, r_prio, w, maxp, keys_out);
  return hipGetLastError();
}

hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* q_pi,
                          const float* q_star, long long K, int W, int n_step, float gamma, long long cursor,
                          long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                          int64_t* keys_out, hipStream_t st) {
  const iqn_replay_host::RolloutShape sh = iqn_replay_host::rollout_shape(K, W);
  iqn_replay_rollout_kernel<<<(unsigned)sh.wgs, 256, 0, st>>>(act, rew, done, q_pi, q_star, K, W, sh.rows, n_step,
                                                              gamma, cursor, cap, alpha, r_act, r_tgt, r_prio, w,
                                                              keys_out);
  return hipGetLastError();
}

}  // namespace iqn_replay_dev
