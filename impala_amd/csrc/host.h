// Host-side toolkit of the handles (impala.hip with dqn.h / dqn_replay.h / iqn.h, and sac.hip):
// the error checks, the integer helpers and the hipGraph cache.  No kernel and no launch lives
// here; the device-only units (iqn.hip, dqn_replay.hip, ppo_replay.hip, dqn_inplace.hip) do not
// include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "arena.h"

// one last-error slot per thread for the library; impala.hip owns it
namespace impala_internal {
int set_error(int code, const std::string& msg);
}

namespace {

int fail(int code, const std::string& msg) { return impala_internal::set_error(code, msg); }

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess)                                                              \
      return fail((int)e_, std::string(#x) + ": " + hipGetErrorString(e_));           \
  } while (0)

#define CK_LAUNCH(name)                                                                \
  do {                                                                                 \
    hipError_t e_ = hipGetLastError();                                                 \
    if (e_ != hipSuccess)                                                              \
      return fail((int)e_, std::string("launch ") + (name) + ": " + hipGetErrorString(e_)); \
  } while (0)

// a launcher of a device-only unit, which returns the launch's hipError_t
#define CK_KERNEL(name, call)                                                          \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail((int)e_, std::string("launch ") + name + ": " + hipGetErrorString(e_)); \
  } while (0)

inline int rup(int x, int m) { return (x + m - 1) / m * m; }
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// hipGraph replay of whole steps: the launch sequence of a step is captured once per kind and
// key (the batch's address set) on a private capture stream and replayed with one hipGraphLaunch.
// The owner's unit declares `bool same_key(const Key&, const Key&)` at global scope (found by
// argument-dependent lookup), and creates and destroys `cap`: every stream a process creates
// takes a share of its hardware queues, so a handle that never replays has none.
template <class Key, int Slots>
struct GraphCache {
  struct Slot {
    hipGraphExec_t exec = nullptr;
    int kind = -1;
    Key key{};
    uint64_t used = 0;
  };
  Slot slots[Slots];
  uint64_t tick = 0;
  hipStream_t cap = nullptr;

  // Run `body` (which enqueues a step's launches on the stream it is given) through the cache:
  // replay a graph captured for the same kind and key, or capture one on the private capture
  // stream, instantiate it and launch it on `st`.  Not `enabled` (the owner's bypass: a live
  // timer needs its events recorded per launch): the launches go straight to `st`.
  template <class Body>
  int run(bool enabled, int kind, const Key& key, hipStream_t st, Body&& body) {
    if (!enabled) return body(st);
    for (Slot& g : slots)
      if (g.exec && g.kind == kind && same_key(g.key, key)) {
        g.used = ++tick;
        CK(hipGraphLaunch(g.exec, st));
        return 0;
      }
    CK(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    const int r = body(cap);
    hipGraph_t graph = nullptr;
    const hipError_t ee = hipStreamEndCapture(cap, &graph);
    if (r || ee != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      return r ? r : fail((int)ee, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) return fail((int)ei, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    Slot* slot = &slots[0];  // the first empty slot, else the least recently used
    for (Slot& g : slots) {
      if (!g.exec) { slot = &g; break; }
      if (g.used < slot->used) slot = &g;
    }
    if (slot->exec) (void)hipGraphExecDestroy(slot->exec);
    *slot = Slot{exec, kind, key, ++tick};
    CK(hipGraphLaunch(exec, st));
    return 0;
  }

  // captured launches hold the pointers they were captured with: drop them when one changes
  void drop() {
    for (Slot& g : slots) {
      if (g.exec) (void)hipGraphExecDestroy(g.exec);
      g = Slot{};
    }
  }
};

}  // namespace
