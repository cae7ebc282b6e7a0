// Workspace carving for the handles (create_learner, dqn_create, iqn_create, iqn_alloc_step, the
// replay's buffers, sac.hip's carve).  Plain C++, no HIP: tests/arena_check.cpp compiles it alone.
//
// A handle's carve is one function that assigns its pointers straight from take() and is run
// twice: on a null base, where every take() returns null and `used` ends at the bytes needed, and
// on the allocation.  A buffer is therefore named once, sized where it is pointed to.  The sizes
// must not depend on pointers the carve itself sets.
#pragma once
#include <cstddef>

struct Arena {
  char* base = nullptr;
  size_t used = 0;
  static size_t align(size_t n) { return (n + 255) & ~(size_t)255; }
  // `bytes` at the next 256-byte boundary (null while base is null)
  void* take(size_t bytes) {
    const size_t a = align(used);
    used = a + bytes;
    return base ? base + a : nullptr;
  }
};
