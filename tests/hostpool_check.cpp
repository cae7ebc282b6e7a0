// CPU check of impala_amd/csrc/hostpool.h (tests/test_hostpool.py): the thread pool runs every
// task exactly once per call, copy_stream copies exactly, the staging thread runs jobs in
// order, waits per slot and reports a failed job's status once, and the staged batch's layout
// and the row collate (StageLayout, collate_rows) equal a plain per-field concatenation.
#include "../impala_amd/csrc/hostpool.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main() {
  using namespace impala_host;
  // pool: 1000 calls of 257 tasks on 3 workers + the caller
  {
    HostPool pool(3, local_node_cpus());
    std::vector<std::atomic<int>> hits(257);
    for (int rep = 0; rep < 1000; ++rep)
      pool.run(257, [&](int i) { hits[i].fetch_add(1); });
    for (auto& h : hits) CHECK(h.load() == 1000);
  }
  // streaming copy: aligned and unaligned sizes / destinations
  {
    std::vector<char> src(70001), dst(70016 + 16);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (char)(i * 131 + 7);
    for (size_t n : {0ul, 16ul, 48ul, 64ul, 65536ul, 70000ul, 70001ul})
      for (size_t off : {0ul, 16ul, 3ul}) {
        std::fill(dst.begin(), dst.end(), 0);
        copy_stream(dst.data() + off + (16 - ((uintptr_t)dst.data() & 15)) % 16, src.data(), n);
        const char* d = dst.data() + off + (16 - ((uintptr_t)dst.data() & 15)) % 16;
        for (size_t i = 0; i < n; ++i) CHECK(d[i] == src[i]);
      }
  }
  // stager: in-order jobs, per-slot waits, one failure reported once
  {
    Stager st;
    std::vector<int> order;
    std::mutex mu;
    for (int j = 0; j < 40; ++j)
      st.submit(j % 3, [&, j](std::string& msg) {
        std::lock_guard<std::mutex> lk(mu);
        order.push_back(j);
        if (j == 7) {
          msg = "job 7";
          return 42;
        }
        return 0;
      });
    std::string m;
    CHECK(st.wait(1, m) == 42 && m == "job 7");  // slot 1 ran job 7
    m.clear();
    CHECK(st.wait(-1, m) == 0 && m.empty());      // reported once
    CHECK(order.size() == 40);
    for (int j = 0; j < 40; ++j) CHECK(order[j] == j);
  }
  // layout + collate: against a plain per-field concatenation, byte for byte.  IMPALA shape
  // (obs row 73 728 B: one whole 64 KB piece and a ragged one) and PPO shape (obs row 12 288 B:
  // one short piece; discounts null, its region of the block untouched); 3-worker pool and serial
  for (int ppo = 0; ppo < 2; ++ppo) {
    const size_t B = 3, T = ppo ? 1 : 6, A = 2;
    const StageLayout L(B, T, A);
    // the layout rule, spelled out: field f holds B rows of T frames of frame[f] bytes and
    // starts at the end of field f - 1 rounded up to 256
    const size_t frame[5] = {3 * 64 * 64, 8, 4, 4, A * 4};
    size_t end = 0;
    for (int f = 0; f < 5; ++f) {
      CHECK(L.row[f] == T * frame[f] && L.bytes[f] == B * T * frame[f]);
      CHECK(L.off[f] == (end + 255) / 256 * 256 && L.off[f] % 256 == 0);
      end = L.off[f] + L.bytes[f];
    }
    CHECK(L.off[5] == (end + 255) / 256 * 256);
    CHECK(L.row[0] == (ppo ? 12288u : 73728u));
    // every row its own allocation, handed over in non-ascending address order
    std::vector<std::vector<char>> store[5];
    const void* ptr[5][3];
    for (int f = 0; f < 5; ++f) {
      for (size_t b = 0; b < B; ++b) {
        store[f].emplace_back(L.row[f]);
        for (size_t i = 0; i < L.row[f]; ++i)
          store[f][b][i] = (char)(i * 31 + (i >> 8) * 7 + (i >> 16) * 13 + b * 101 + f * 17 + 3);
      }
      std::vector<const char*> p;
      for (auto& v : store[f]) p.push_back(v.data());
      std::sort(p.begin(), p.end());
      ptr[f][0] = p[2], ptr[f][1] = p[0], ptr[f][2] = p[1];
    }
    const void* const* rows[5] = {ptr[0], ptr[1], ptr[2], ppo ? nullptr : ptr[3], ptr[4]};
    std::vector<char> want(L.off[5], (char)0x5a);
    for (int f = 0; f < 5; ++f)
      for (size_t b = 0; b < B && rows[f]; ++b)
        std::memcpy(want.data() + L.off[f] + b * L.row[f], rows[f][b], L.row[f]);
    HostPool pool(3);
    for (HostPool* p : {&pool, (HostPool*)nullptr}) {
      // a 16-byte aligned block, as the page-locked one is (copy_stream's streaming stores)
      std::vector<char> got(L.off[5] + 16, (char)0x5a);
      char* g = got.data() + (16 - ((uintptr_t)got.data() & 15)) % 16;
      collate_rows(L, rows, (int)B, g, p);
      CHECK(std::memcmp(g, want.data(), L.off[5]) == 0);
    }
  }
  std::printf("hostpool ok\n");
  return 0;
}
