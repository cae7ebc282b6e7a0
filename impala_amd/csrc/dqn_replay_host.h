// Host bookkeeping of the prioritized ring behind dqn_replay (include/dqn_hip.h, W = 1 target per
// row) and iqn_replay (include/iqn_hip.h, W = n_tau): the ring's cursor / size arithmetic, the
// split of an append into contiguous spans, the launch shapes of the sampling and ingest kernels,
// the split of a long priority update into launches and every argument check.  No HIP here, so
// tests/dqn_replay_check.cpp and tests/iqn_replay_check.cpp run it on the CPU under sanitizers;
// csrc/dqn_replay.{h,hip} and csrc/iqn_replay.h are its other users.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/dqn_hip.h"

namespace dqn_replay_host {

// the draw kernel keeps every block sum in LDS: at most 4096 doubles (32 KB)
constexpr int64_t kMaxBlocks = 4096;
constexpr int64_t kMaxCapacity = kMaxBlocks * DQN_REPLAY_BLOCK;
constexpr int kMaxSample = 1 << 20;
constexpr int kScanThreads = 256;
constexpr int kWg = 256;       // threads of a workgroup of both ingest kernels
constexpr int kMaxWidth = 32;  // IQN_MAX_TAU (csrc/iqn_replay.h asserts that the two agree)

struct Ring {
  int64_t cap = 0, size = 0, cursor = 0;
};

// rows [src, src + n) of an append land on ring rows [dst, dst + n)
struct Span {
  int64_t dst, src, n;
};

inline void reset(Ring& r) { r.size = r.cursor = 0; }

// -> number of spans (1 or 2; 0 when n is out of range) of an append of n rows at the cursor
inline int spans(const Ring& r, int64_t n, Span out[2]) {
  if (n < 1 || n > r.cap) return 0;
  const int64_t first = n < r.cap - r.cursor ? n : r.cap - r.cursor;
  out[0] = Span{r.cursor, 0, first};
  if (first == n) return 1;
  out[1] = Span{0, first, n - first};
  return 2;
}

inline void advance(Ring& r, int64_t n) {
  r.cursor = (r.cursor + n) % r.cap;
  r.size = r.size + n < r.cap ? r.size + n : r.cap;
}

inline int64_t blocks(int64_t size) { return (size + DQN_REPLAY_BLOCK - 1) / DQN_REPLAY_BLOCK; }

// The draw kernel's scan of nb block sums: thread t sums `chunk` consecutive sums in order, then
// one thread walks the threads' totals in order.  chunk ~ sqrt(nb) keeps both walks short;
// chunk * kScanThreads >= nb always.
inline int scan_chunk(int64_t nb) {
  int c = (int)std::ceil(std::sqrt((double)nb));
  if (c < 1) c = 1;
  while ((int64_t)c * kScanThreads < nb) ++c;
  return c;
}

// Argument checks: nullptr when fine, else the message (it names the argument).
inline const char* check_create(int64_t capacity, double priority_exponent) {
  if (capacity < 1) return "capacity must be >= 1";
  if (capacity > kMaxCapacity) return "capacity must be <= 2097152 (4096 blocks of 512 rows)";
  if (!(priority_exponent >= 0.0) || std::isinf(priority_exponent))
    return "priority_exponent must be finite and >= 0";
  return nullptr;
}

inline const char* check_n_tau(int n_tau) {
  if (n_tau < 1 || n_tau > kMaxWidth) return "n_tau must be in [1, 32]";
  return nullptr;
}

inline const char* check_create(int64_t capacity, int n_tau, double priority_exponent) {
  if (const char* m = check_n_tau(n_tau)) return m;
  return check_create(capacity, priority_exponent);
}

// The checks below run twice: with r null before the handle is looked at (what the scalars alone
// decide), then with the ring.
inline const char* check_extend(const Ring* r, int64_t n) {
  if (n < 1) return "n must be >= 1";
  if (r && n > r->cap) return "n must be <= capacity";
  return nullptr;
}

inline const char* check_rollout(const Ring* r, int64_t L, int n_step, float gamma) {
  if (L < 2) return "L must be >= 2";
  if (n_step < 1 || n_step > DQN_REPLAY_MAX_NSTEP) return "n_step must be in [1, 16]";
  if (!(gamma >= 0.f && gamma <= 1.f)) return "gamma must be in [0, 1]";
  if (r && L - 1 > r->cap) return "L - 1 must be <= capacity";
  return nullptr;
}

inline const char* check_sample(const Ring* r, int64_t n) {
  if (n < 1) return "n must be >= 1";
  if (n > kMaxSample) return "n must be <= 1048576";
  if (r && r->size < 1) return "the replay is empty (size 0)";
  return nullptr;
}

inline const char* check_update(int64_t n) {
  if (n < 1) return "n must be >= 1";
  if (n > DQN_MAX_BATCH) return "n must be <= DQN_MAX_BATCH (4096)";
  return nullptr;
}

// replay_extend_kernel: one thread per target, n * W of them
inline int64_t extend_wgs(int64_t n, int W) { return (n * W + kWg - 1) / kWg; }

// replay_rollout_kernel: a workgroup holds `rows` whole transitions, W consecutive threads each
// (threads past rows * W idle), so a transition's targets never straddle two workgroups
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

}  // namespace dqn_replay_host
