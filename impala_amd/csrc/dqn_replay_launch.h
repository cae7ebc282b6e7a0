// Launchers of the replay kernels (csrc/dqn_replay.hip), called by the host side in
// csrc/dqn_replay.h.  Each enqueues one kernel on `st` and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dqn_replay_dev {

// bsum[b] = the sum of weights[b * 512 .. min(size, (b + 1) * 512)), b < nb
hipError_t launch_block_sum(const double* w, long long size, int nb, double* bsum, hipStream_t st);
// keys [n], prob [n] by the sampling contract of include/dqn_hip.h; chunk = scan_chunk(nb)
hipError_t launch_draw(const double* w, const double* bsum, long long size, int nb, int chunk, uint64_t seed,
                       uint64_t counter, int n, int64_t* keys, float* prob, hipStream_t st);
hipError_t launch_update(const int64_t* keys, const float* pin, int n, long long cap, double alpha, float* prio,
                         double* w, float* maxp, hipStream_t st);
hipError_t launch_extend(const int64_t* act, const float* tgt, const float* pin, long long n, long long cursor,
                         long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                         float* maxp, int64_t* keys_out, hipStream_t st);
hipError_t launch_rollout(const int64_t* act, const float* rew, const uint8_t* done, const float* q_pi,
                          const float* q_star, long long K, int n_step, float gamma, long long cursor,
                          long long cap, double alpha, int64_t* r_act, float* r_tgt, float* r_prio, double* w,
                          float* maxp, int64_t* keys_out, hipStream_t st);
// *maxp = max(*maxp, the n ring priorities at (cursor + i) % cap): what launch_extend and
// launch_rollout end with, for an ingest kernel of another unit (csrc/iqn_replay.hip)
hipError_t launch_raise_max(const float* r_prio, long long n, long long cursor, long long cap, float* maxp,
                            hipStream_t st);

}  // namespace dqn_replay_dev
