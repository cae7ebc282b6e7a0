// What csrc/impala.hip takes from csrc/ppo_replay.hip: the launcher of the PPO ingest kernel
// (impala_ppo_extend_rollout; it enqueues one kernel on `st` and returns hipGetLastError()), and
// the fused head instantiated for a PPO handle reading a ring in place
// (impala_ppo_train_step_rows), which launch_backward launches like every other learner kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct HeadArgs;
struct ObsRows;

namespace ppo_replay_dev {

// head_step_kernel<T, true, ObsRows> (head.h), T = __bf16 or float
using HeadRowsKernel = void (*)(const HeadArgs, const ObsRows);
HeadRowsKernel head_rows_kernel(bool bf16);

constexpr long long kMaxRollout = 1025;  // L: the kernel stages K = L - 1 <= 1024 steps in LDS

// target[t], t < K = L - 1, by the recurrence of include/impala_hip.h (impala_ppo_extend_rollout),
// then actions[t], target[t] and logits[t][0..A) into ring rows (cursor + t) % cap.
// Needs 2 <= L <= kMaxRollout, K <= cap, 0 <= cursor < cap, 1 <= A.
hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* logits,
                          const float* values, long long L, int A, float gamma, float lambda,
                          long long cursor, long long cap, int64_t* r_act, float* r_tgt, float* r_mu,
                          hipStream_t st);

}  // namespace ppo_replay_dev
