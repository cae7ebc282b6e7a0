// CPU check of impala_amd/csrc/iqn_replay_host.h (tests/test_iqn_replay_host.py): the width and
// create checks, the launch shapes of the two ingest kernels against a per-thread model of their
// indexing, and the split of a priority update into chunks.  Built with
// -fsanitize=address,undefined; no GPU involved.
#include "../impala_amd/csrc/iqn_replay_host.h"

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace iqn_replay_host;
  // the checks name the argument; n_tau comes first
  CHECK(check_n_tau(1) == nullptr && check_n_tau(IQN_MAX_TAU) == nullptr);
  CHECK(std::strstr(check_n_tau(0), "n_tau") && std::strstr(check_n_tau(IQN_MAX_TAU + 1), "n_tau"));
  CHECK(check_create(1, 1, 0.0) == nullptr);
  CHECK(check_create(dqn_replay_host::kMaxCapacity, IQN_MAX_TAU, 0.6) == nullptr);
  CHECK(std::strstr(check_create(0, 0, -1.0), "n_tau"));
  CHECK(std::strstr(check_create(0, 8, -1.0), "capacity"));
  CHECK(std::strstr(check_create(dqn_replay_host::kMaxCapacity + 1, 8, 0.6), "capacity"));
  CHECK(std::strstr(check_create(8, 8, -1.0), "priority_exponent"));
  CHECK(std::strstr(check_create(8, 8, NAN), "priority_exponent"));
  CHECK(std::strstr(check_create(8, 8, INFINITY), "priority_exponent"));

  for (int W = 1; W <= IQN_MAX_TAU; ++W) {
    // the extend kernel: one thread per target, every target of n rows covered once
    for (int64_t n : {(int64_t)1, (int64_t)6, (int64_t)255, (int64_t)257, (int64_t)1000}) {
      const int64_t wgs = extend_wgs(n, W);
      CHECK(wgs >= 1 && wgs * kWg >= n * W && (wgs - 1) * kWg < n * W);
    }
    // the rollout kernel: a per-thread model of its indexing (thread tid of workgroup b is column
    // tid % W of transition b * rows + tid / W when tid / W < rows); every (t, k) is owned once,
    // the column-0 thread's LDS reads [tid, tid + W) stay inside the workgroup's 256 floats and
    // inside its own transition
    for (int64_t K : {(int64_t)1, (int64_t)2, (int64_t)100, (int64_t)600, (int64_t)1023}) {
      const RolloutShape sh = rollout_shape(K, W);
      CHECK(sh.rows >= 1 && sh.rows * W <= kWg && (sh.rows + 1) * W > kWg);
      CHECK(sh.wgs >= 1 && sh.wgs * sh.rows >= K && (sh.wgs - 1) * sh.rows < K);
      std::vector<int> owned((size_t)K * W, 0);
      for (int64_t b = 0; b < sh.wgs; ++b)
        for (int tid = 0; tid < kWg; ++tid) {
          const int lr = tid / W, k = tid - lr * W;
          const int64_t t = b * sh.rows + lr;
          if (!(lr < sh.rows && t < K)) continue;
          owned[(size_t)(t * W + k)] += 1;
          if (k == 0) CHECK(tid + W <= kWg && (tid + W - 1) / W == lr);
        }
      for (int v : owned) CHECK(v == 1);
    }
  }
  CHECK(extend_wgs(dqn_replay_host::kMaxCapacity, IQN_MAX_TAU) < ((int64_t)1 << 31));

  // the update's chunks cover [0, n) once, in order, each at most DQN_MAX_BATCH
  CHECK(update_chunks(0) == 0 && update_chunks(-4) == 0);
  for (int n : {1, 2, DQN_MAX_BATCH - 1, DQN_MAX_BATCH, DQN_MAX_BATCH + 1, 3 * DQN_MAX_BATCH, IQN_MAX_ROWS}) {
    const int nc = update_chunks(n);
    CHECK(nc >= 1);
    int covered = 0;
    for (int i = 0; i < nc; ++i) {
      const Chunk c = update_chunk(n, i);
      CHECK(c.off == covered && c.len >= 1 && c.len <= DQN_MAX_BATCH);
      CHECK(dqn_replay_host::check_update(c.len) == nullptr);
      covered += c.len;
    }
    CHECK(covered == n);
  }
  std::printf("iqn_replay ok\n");
  return 0;
}
