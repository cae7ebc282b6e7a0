// PPO on the device (csrc/ppo_replay_launch.h): the kernel of the actor's ingest
// (include/impala_hip.h, impala_ppo_extend_rollout) with its launcher, and the fused head
// instantiated for a PPO handle that reads a ring in place (impala_ppo_train_step_rows).  A
// translation unit of its own, as dqn_replay.hip is: the code object of impala.hip -- the
// learner steps' kernels and where they sit in it -- is the same with or without them (the head
// instantiated inside impala.hip moved every kernel behind it, and the PPO bf16 step from 0.0616
// to 0.0625 ms: profiles/ppo_replay/ab.txt).
//
// The ingest:
// One workgroup per rollout.  All threads stage r, the discounts d_t = done[t] ? 0 : gamma and v
// in LDS (coalesced loads); one lane runs the lambda-return scan, a dependent chain of K <= 1024
// steps, and leaves target[t] in r's place; all threads then write the K action, target and
// logits rows, each row's ring index computed from the cursor (the obs rows travel by device
// copies).  Nothing outside the K ring rows is written.
#include "common.h"
#include "head.h"

#include "ppo_replay_launch.h"

namespace {

constexpr int kMaxK = (int)ppo_replay_dev::kMaxRollout - 1;

// rlax lambda_returns(r[:-1], discount[:-1], v[1:], lambda) in fp32, every operation rounded
// once (no contraction into fused multiply-adds), in the order the header states.
__global__ __launch_bounds__(256) void ppo_rollout_kernel(const int64_t* __restrict__ act,
                                                          const float* __restrict__ rew,
                                                          const uint8_t* __restrict__ done,
                                                          const float* __restrict__ logits,
                                                          const float* __restrict__ values, int K, int A,
                                                          float gamma, float lambda, long long cursor,
                                                          long long cap, int64_t* __restrict__ r_act,
                                                          float* __restrict__ r_tgt, float* __restrict__ r_mu) {
#pragma clang fp contract(off)
  __shared__ float rs[kMaxK];      // r[t], then target[t]
  __shared__ float ds[kMaxK];      // d_t
  __shared__ float vs[kMaxK + 1];  // v[0 .. K]
  const int tid = threadIdx.x;
  for (int t = tid; t < K; t += 256) {
    rs[t] = rew[t];
    ds[t] = done[t] ? 0.f : gamma;
  }
  for (int t = tid; t <= K; t += 256) vs[t] = values[t];
  __syncthreads();
  if (tid == 0) {
    const float oml = 1.f - lambda;
    float acc = vs[K];
    for (int t = K - 1; t >= 0; --t) {
      const float p = oml * vs[t + 1];
      const float q = lambda * acc;
      const float s = p + q;
      const float m = ds[t] * s;
      acc = rs[t] + m;
      rs[t] = acc;
    }
  }
  __syncthreads();
  for (int t = tid; t < K; t += 256) {
    long long k = cursor + t;  // cursor < cap and t < K <= cap: one wrap at most
    if (k >= cap) k -= cap;
    r_act[k] = act[t];
    r_tgt[k] = rs[t];
  }
  for (int i = tid; i < K * A; i += 256) {
    const int t = i / A, j = i - t * A;
    long long k = cursor + t;
    if (k >= cap) k -= cap;
    r_mu[k * A + j] = logits[i];
  }
}

}  // namespace

namespace ppo_replay_dev {

HeadRowsKernel head_rows_kernel(bool bf16) {
  return bf16 ? head_step_kernel<__bf16, true, ObsRows> : head_step_kernel<float, true, ObsRows>;
}

hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* logits,
                          const float* values, long long L, int A, float gamma, float lambda,
                          long long cursor, long long cap, int64_t* r_act, float* r_tgt, float* r_mu,
                          hipStream_t st) {
  const long long K = L - 1;
  if (K < 1 || K > kMaxK || K > cap || cursor < 0 || cursor >= cap || A < 1) return hipErrorInvalidValue;
  ppo_rollout_kernel<<<1, 256, 0, st>>>(act, rew, done, logits, values, (int)K, A, gamma, lambda, cursor, cap,
                                        r_act, r_tgt, r_mu);
  return hipGetLastError();
}

}  // namespace ppo_replay_dev
