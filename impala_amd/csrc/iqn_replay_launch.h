// Launchers of the IQN replay's ingest kernels (csrc/iqn_replay.hip), called by the host side in
// csrc/iqn_replay.h.  Each enqueues one kernel on `st` and returns hipGetLastError(); neither
// kernel writes *maxp (dqn_replay_dev::launch_raise_max follows where priorities were given).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iqn_replay_dev {

// n rows of W targets appended at the cursor (across the wrap); pin null: rows take *maxp
hipError_t launch_extend(const int64_t* act, const float* tgt, const float* pin, long long n, int W,
                         long long cursor, long long cap, double alpha, int64_t* r_act, float* r_tgt,
                         float* r_prio, double* w, const float* maxp, int64_t* keys_out, hipStream_t st);
// K = L - 1 transitions of one rollout: targets [K][W], priorities, weights, actions at their ring rows
hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* q_pi,
                          const float* q_star, long long K, int W, int n_step, float gamma, long long cursor,
                          long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                          int64_t* keys_out, hipStream_t st);

}  // namespace iqn_replay_dev
