// CPU check of impala_amd/csrc/arena.h (tests/test_arena.py): the sizing pass on a null base and
// the pass on an allocation use the same bytes, every piece starts on a 256-byte boundary of the
// base, pieces do not overlap, and the null-base pass hands out null.
#include "../impala_amd/csrc/arena.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main() {
  // (no piece is touched: the 5 GiB one lies far past the block the base points to)
  const std::vector<size_t> sizes = {0, 1, 255, 256, 257, ((size_t)5 << 30) + 3, 1, 0, 4096, 8};
  char* block = (char*)std::aligned_alloc(256, 4096);
  CHECK(block);

  Arena sizing{};
  for (size_t n : sizes) CHECK(sizing.take(n) == nullptr);
  CHECK(sizing.base == nullptr);

  Arena real{block};
  uintptr_t prev_end = (uintptr_t)block;
  for (size_t i = 0; i < sizes.size(); ++i) {
    const uintptr_t p = (uintptr_t)real.take(sizes[i]);
    const uintptr_t off = p - (uintptr_t)block;
    CHECK(off % 256 == 0);                      // base + 256 k
    CHECK(p >= prev_end);                       // past the piece before it
    CHECK(p - prev_end < 256);                  // and no further than the next boundary
    CHECK(real.used == off + sizes[i]);
    prev_end = p + sizes[i];
  }
  CHECK(real.used == sizing.used);
  CHECK(real.used > ((size_t)5 << 30));         // (nothing was truncated to 32 bits)

  CHECK(Arena::align(0) == 0 && Arena::align(1) == 256 && Arena::align(256) == 256 && Arena::align(257) == 512);
  CHECK(Arena::align(real.used) % 256 == 0 && Arena::align(real.used) - real.used < 256);
  // the first piece of an arena is its base
  Arena first{block};
  CHECK(first.take(7) == (void*)block && first.used == 7);
  std::free(block);
  std::printf("arena ok\n");
  return 0;
}
