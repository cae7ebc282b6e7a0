// Host bookkeeping of dqn_replay (include/dqn_hip.h): the ring's cursor / size arithmetic, the
// split of an append into contiguous spans, the launch shapes of the two sampling kernels and
// every argument check.  No HIP here, so tests/dqn_replay_check.cpp runs it on the CPU under
// sanitizers; csrc/dqn_replay.h is its only other user.
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

}  // namespace dqn_replay_host
