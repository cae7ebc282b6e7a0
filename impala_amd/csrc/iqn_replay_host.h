// Host bookkeeping of iqn_replay (include/iqn_hip.h) beyond dqn_replay's own
// (csrc/dqn_replay_host.h, which it reuses for the ring, the spans and the scalar checks): the
// width check, the launch shapes of the two ingest kernels (csrc/iqn_replay.hip) and the split of a
// priority update into launches of at most DQN_MAX_BATCH keys.  No HIP here, so
// tests/iqn_replay_check.cpp runs it on the CPU under sanitizers; csrc/iqn_replay.h is its only
// other user.
#pragma once
#include <cstdint>

#include "../../include/iqn_hip.h"
#include "dqn_replay_host.h"

namespace iqn_replay_host {

constexpr int kWg = 256;  // threads of a workgroup of both ingest kernels

// Argument checks: nullptr when fine, else the message (it names the argument).
inline const char* check_n_tau(int n_tau) {
  if (n_tau < 1 || n_tau > IQN_MAX_TAU) return "n_tau must be in [1, 32]";
  return nullptr;
}

inline const char* check_create(int64_t capacity, int n_tau, double priority_exponent) {
  if (const char* m = check_n_tau(n_tau)) return m;
  return dqn_replay_host::check_create(capacity, priority_exponent);
}

// iqn_replay_extend_kernel: one thread per target, n * W of them
inline int64_t extend_wgs(int64_t n, int W) { return (n * W + kWg - 1) / kWg; }

// iqn_replay_rollout_kernel: a workgroup holds `rows` whole transitions, W consecutive threads
// each (threads past rows * W idle), so a transition's targets never straddle two workgroups
struct RolloutShape {
  int rows;
  int64_t wgs;
};
inline RolloutShape rollout_shape(int64_t K, int W) {
  const int rows = kWg / W;
  return RolloutShape{rows, (K + rows - 1) / rows};
}

// A priority update of n keys as launches of at most DQN_MAX_BATCH keys, in order: chunk i of
// update_chunks(n) covers keys [off, off + len).
struct Chunk {
  int off, len;
};
inline int update_chunks(int n) { return n < 1 ? 0 : (n + DQN_MAX_BATCH - 1) / DQN_MAX_BATCH; }
inline Chunk update_chunk(int n, int i) {
  const int off = i * DQN_MAX_BATCH;
  return Chunk{off, n - off < DQN_MAX_BATCH ? n - off : DQN_MAX_BATCH};
}

}  // namespace iqn_replay_host
