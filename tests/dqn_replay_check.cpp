// CPU check of impala_amd/csrc/dqn_replay_host.h (tests/test_dqn_replay_host.py): the ring's
// cursor / size / wrap arithmetic against a plain per-row model, the spans of an append, the
// launch shape of the block-sum scan and the argument checks.  Built with
// -fsanitize=address,undefined; no GPU involved.  With the argument "scan_chunk" it prints
// scan_chunk(nb) for every legal nb instead, one per line: the table the Python mirror
// (tests/dqn_replay_oracle.py) is compared with.
#include "../impala_amd/csrc/dqn_replay_host.h"

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

int main(int argc, char** argv) {
  using namespace dqn_replay_host;
  if (argc > 1 && std::strcmp(argv[1], "scan_chunk") == 0) {
    for (int64_t nb = 1; nb <= kMaxBlocks; ++nb) std::printf("%d\n", scan_chunk(nb));
    return 0;
  }
  // appends of every size at every cursor against a per-row model: the spans cover the input
  // once, in order, inside the ring
  for (int64_t cap : {1, 2, 7, 8, 64}) {
    Ring r;
    r.cap = cap;
    std::vector<int64_t> model(cap, -1), ring(cap, -1);
    int64_t written = 0, stamp = 0;
    for (int round = 0; round < 5; ++round)
      for (int64_t n = 1; n <= cap; ++n) {
        Span sp[2];
        const int ns = spans(r, n, sp);
        CHECK(ns == 1 || ns == 2);
        int64_t covered = 0;
        for (int i = 0; i < ns; ++i) {
          CHECK(sp[i].n >= 1 && sp[i].src == covered);
          CHECK(sp[i].dst >= 0 && sp[i].dst + sp[i].n <= cap);
          for (int64_t k = 0; k < sp[i].n; ++k) ring[sp[i].dst + k] = stamp + sp[i].src + k;
          covered += sp[i].n;
        }
        CHECK(covered == n);
        CHECK(ns == 1 || (sp[0].dst + sp[0].n == cap && sp[1].dst == 0));
        for (int64_t i = 0; i < n; ++i) model[(r.cursor + i) % cap] = stamp + i;
        const int64_t cursor0 = r.cursor;
        advance(r, n);
        written += n;
        stamp += n;
        CHECK(r.cursor == (cursor0 + n) % cap && r.cursor >= 0 && r.cursor < cap);
        CHECK(r.size == (written < cap ? written : cap));
        CHECK(ring == model);
      }
    Span sp[2];
    CHECK(spans(r, 0, sp) == 0 && spans(r, cap + 1, sp) == 0 && spans(r, -1, sp) == 0);
    reset(r);
    CHECK(r.size == 0 && r.cursor == 0 && r.cap == cap);
  }
  // blocks and the scan's shape: chunk * threads covers every block sum, for every legal capacity
  CHECK(blocks(1) == 1 && blocks(DQN_REPLAY_BLOCK) == 1 && blocks(DQN_REPLAY_BLOCK + 1) == 2);
  CHECK(blocks(kMaxCapacity) == kMaxBlocks);
  for (int64_t nb = 1; nb <= kMaxBlocks; ++nb) {
    const int c = scan_chunk(nb);
    CHECK(c >= 1 && (int64_t)c * kScanThreads >= nb);
    CHECK((nb + c - 1) / c <= kScanThreads);
    CHECK(c <= 65 || nb > 4096);  // about sqrt(nb)
  }
  // argument checks name the argument
  CHECK(check_create(1, 0.0) == nullptr && check_create(kMaxCapacity, 0.6) == nullptr);
  CHECK(std::strstr(check_create(0, 0.6), "capacity"));
  CHECK(std::strstr(check_create(kMaxCapacity + 1, 0.6), "capacity"));
  CHECK(std::strstr(check_create(8, -1.0), "priority_exponent"));
  CHECK(std::strstr(check_create(8, NAN), "priority_exponent"));
  Ring r;
  r.cap = 10;
  CHECK(check_extend(&r, 10) == nullptr && check_extend(nullptr, 11) == nullptr);
  CHECK(std::strstr(check_extend(&r, 11), "capacity") && std::strstr(check_extend(&r, 0), "n must"));
  CHECK(check_rollout(&r, 11, 3, 0.99f) == nullptr && check_rollout(&r, 2, 16, 1.f) == nullptr);
  CHECK(std::strstr(check_rollout(&r, 12, 3, 0.99f), "capacity"));
  CHECK(std::strstr(check_rollout(&r, 1, 3, 0.99f), "L must"));
  CHECK(std::strstr(check_rollout(&r, 5, 0, 0.99f), "n_step") && std::strstr(check_rollout(&r, 5, 17, 0.99f), "n_step"));
  CHECK(std::strstr(check_rollout(&r, 5, 3, -0.1f), "gamma") && std::strstr(check_rollout(&r, 5, 3, NAN), "gamma"));
  CHECK(std::strstr(check_sample(&r, 4), "empty") && check_sample(nullptr, 4) == nullptr);
  advance(r, 3);
  CHECK(check_sample(&r, 4) == nullptr && check_sample(&r, 1000) == nullptr);  // draws with replacement
  CHECK(std::strstr(check_sample(&r, 0), "n must") && std::strstr(check_sample(&r, kMaxSample + 1), "n must"));
  CHECK(check_update(1) == nullptr && check_update(DQN_MAX_BATCH) == nullptr);
  CHECK(std::strstr(check_update(0), "n must") && std::strstr(check_update(DQN_MAX_BATCH + 1), "DQN_MAX_BATCH"));
  std::printf("dqn_replay ok\n");
  return 0;
}
