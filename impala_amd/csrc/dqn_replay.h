// Host side of the device-side prioritized replay of the Ape-X DQN learner (include/dqn_hip.h,
// dqn_replay_*).  Included at the end of impala.hip after dqn.h: dqn_train_step_replay enqueues
// the step exactly as dqn_train_step does, and the batch gather is gather_rows_kernel with its
// device index; dqn_train_step_replay_rows skips the gather and switches the core handle's key
// map on (ObsKeys, conv1.h), so the step reads the sampled ring rows in place through the kernels
// of csrc/dqn_inplace.hip.  The replay's own kernels live in csrc/dqn_replay.hip (a translation unit of its
// own, so impala.hip's code object does not change with them) behind csrc/dqn_replay_launch.h;
// the ring's bookkeeping and the argument checks are csrc/dqn_replay_host.h.
#pragma once
#include "../../include/dqn_hip.h"
#include "dqn_replay_host.h"
#include "dqn_replay_launch.h"

struct dqn_replay {
  dqn_replay_host::Ring ring;
  double alpha = 0.0;
  int device = 0;
  // caller-owned (dqn_replay_bind)
  uint8_t* obs = nullptr;
  int64_t* actions = nullptr;
  float* targets = nullptr;
  float* priorities = nullptr;
  // library-owned sampling state: weights [cap], block sums [blocks(cap)], the running maximum
  char* state = nullptr;
  double* weights = nullptr;
  double* bsum = nullptr;
  float* maxp = nullptr;
  // library-owned gather buffer of one batch (dqn_train_step_replay)
  char* gbuf = nullptr;
  int g_rows = 0;
  uint8_t* g_obs = nullptr;
  int64_t *g_act = nullptr, *g_keys = nullptr;
  float *g_tgt = nullptr, *g_prob = nullptr, *g_prio = nullptr;
  // library-owned per-transition scratch of one batch read in place (dqn_train_step_replay_rows):
  // keys, probabilities, priorities -- no obs rows
  char* sbuf = nullptr;
  int s_rows = 0;
  int64_t* s_keys = nullptr;
  float *s_prob = nullptr, *s_prio = nullptr;
};

namespace {

constexpr size_t kObsRowBytes = 3 * 64 * 64;

// the first null pointer's argument name, or nullptr
struct NamedPtr {
  const char* name;
  const void* p;
};
const char* first_null(std::initializer_list<NamedPtr> ps) {
  for (const NamedPtr& x : ps)
    if (!x.p) return x.name;
  return nullptr;
}
#define CK_PTRS(entry, ...)                                                             \
  do {                                                                                  \
    if (const char* a_ = first_null({__VA_ARGS__}))                                     \
      return fail(IMPALA_E_INVALID, std::string(entry ": null pointer: ") + a_);        \
  } while (0)

int replay_check(const dqn_replay* r, bool bound) {
  if (!r) return fail(IMPALA_E_INVALID, "null replay handle");
  if (bound && !r->obs) return fail(IMPALA_E_STATE, "dqn_replay_bind() not called");
  return 0;
}

int replay_copy_obs(dqn_replay* r, const uint8_t* obs, int64_t n, hipStream_t st) {
  dqn_replay_host::Span sp[2];
  const int ns = dqn_replay_host::spans(r->ring, n, sp);
  for (int i = 0; i < ns; ++i)
    CK(hipMemcpyAsync(r->obs + (size_t)sp[i].dst * kObsRowBytes, obs + (size_t)sp[i].src * kObsRowBytes,
                      (size_t)sp[i].n * kObsRowBytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

// keys [n], probabilities [n] of n draws (the two sampling launches)
int replay_enqueue_draws(dqn_replay* r, uint64_t seed, uint64_t counter, int n, int64_t* keys, float* prob,
                         hipStream_t st) {
  const int nb = (int)dqn_replay_host::blocks(r->ring.size);
  CK_KERNEL("replay_block_sum", dqn_replay_dev::launch_block_sum(r->weights, r->ring.size, nb, r->bsum, st));
  CK_KERNEL("replay_draw", dqn_replay_dev::launch_draw(r->weights, r->bsum, r->ring.size, nb,
                                                       dqn_replay_host::scan_chunk(nb), seed, counter, n, keys,
                                                       prob, st));
  return 0;
}

int replay_enqueue_gather(dqn_replay* r, const int64_t* keys, int n, uint8_t* obs, int64_t* act, float* tgt,
                          hipStream_t st) {
  const void* src[3] = {r->obs, r->actions, r->targets};
  void* dst[3] = {obs, act, tgt};
  const size_t rb[3] = {kObsRowBytes, sizeof(int64_t), sizeof(float)};
  return gather_launch(src, dst, rb, 3, keys, nullptr, n, st);
}

int replay_enqueue_update(dqn_replay* r, const int64_t* keys, const float* prio, int n, hipStream_t st) {
  CK_KERNEL("replay_update", dqn_replay_dev::launch_update(keys, prio, n, r->ring.cap, r->alpha, r->priorities,
                                                           r->weights, r->maxp, st));
  return 0;
}

int replay_ensure_gather(dqn_replay* r, int n) {
  if (r->g_rows >= n) return 0;
  if (r->gbuf) CK(hipFree(r->gbuf));  // (synchronises: no launch still reads it)
  r->gbuf = nullptr;
  r->g_rows = 0;
  auto carve = [&](Arena a) {
    r->g_obs = (uint8_t*)a.take((size_t)n * kObsRowBytes);
    r->g_act = (int64_t*)a.take((size_t)n * 8);
    r->g_keys = (int64_t*)a.take((size_t)n * 8);
    r->g_tgt = (float*)a.take((size_t)n * 4);
    r->g_prob = (float*)a.take((size_t)n * 4);
    r->g_prio = (float*)a.take((size_t)n * 4);
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  CK(hipMalloc((void**)&r->gbuf, total));
  carve(Arena{r->gbuf});
  r->g_rows = n;
  return 0;
}

int replay_ensure_scratch(dqn_replay* r, int n) {
  if (r->s_rows >= n) return 0;
  if (r->sbuf) CK(hipFree(r->sbuf));  // (synchronises: no launch still reads it)
  r->sbuf = nullptr;
  r->s_rows = 0;
  auto carve = [&](Arena a) {
    r->s_keys = (int64_t*)a.take((size_t)n * 8);
    r->s_prob = (float*)a.take((size_t)n * 4);
    r->s_prio = (float*)a.take((size_t)n * 4);
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  CK(hipMalloc((void**)&r->sbuf, total));
  carve(Arena{r->sbuf});
  r->s_rows = n;
  return 0;
}

}  // namespace

extern "C" {

int dqn_replay_block(void) { return DQN_REPLAY_BLOCK; }

int dqn_replay_create(int64_t capacity, double priority_exponent, int device, dqn_replay** out) {
  CK_PTRS("dqn_replay_create", {"out", out});
  *out = nullptr;
  if (const char* m = dqn_replay_host::check_create(capacity, priority_exponent))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_create: ") + m);
  if (device < 0) return fail(IMPALA_E_INVALID, "dqn_replay_create: device must be >= 0");
  dqn_replay* r = new (std::nothrow) dqn_replay();
  if (!r) return fail(IMPALA_E_INVALID, "out of host memory");
  r->ring.cap = capacity;
  r->alpha = priority_exponent;
  r->device = device;
  auto carve = [&](Arena a) {
    r->weights = (double*)a.take((size_t)capacity * 8);
    r->bsum = (double*)a.take((size_t)dqn_replay_host::blocks(capacity) * 8);
    r->maxp = (float*)a.take(4);
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&r->state, total);
  if (e == hipSuccess) e = hipMemset(r->state, 0, total);
  carve(Arena{r->state});
  const float one = 1.f;
  if (e == hipSuccess) e = hipMemcpy(r->maxp, &one, 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (r->state) (void)hipFree(r->state);
    delete r;
    return fail((int)e, std::string("dqn_replay_create: ") + hipGetErrorString(e));
  }
  *out = r;
  return 0;
}

int dqn_replay_destroy(dqn_replay* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  if (r->gbuf) (void)hipFree(r->gbuf);
  if (r->sbuf) (void)hipFree(r->sbuf);
  if (r->state) (void)hipFree(r->state);
  delete r;
  return 0;
}

int dqn_replay_bind(dqn_replay* r, uint8_t* obs, int64_t* actions, float* targets, float* priorities,
                    void* stream) {
  // (arguments first, then the handle: every check is reachable without a device)
  CK_PTRS("dqn_replay_bind", {"obs", obs}, {"actions", actions}, {"targets", targets}, {"priorities", priorities});
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "dqn_replay_bind: obs must be 16-byte aligned");
  if (int e = replay_check(r, false)) return e;
  CK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  CK(hipMemsetAsync(r->weights, 0, (size_t)r->ring.cap * 8, st));
  CK(hipMemsetD32Async((hipDeviceptr_t)r->maxp, 0x3f800000, 1, st));  // 1.0f
  r->obs = obs; r->actions = actions; r->targets = targets; r->priorities = priorities;
  dqn_replay_host::reset(r->ring);
  return 0;
}

int dqn_replay_state(const dqn_replay* r, int64_t* size, int64_t* cursor) {
  CK_PTRS("dqn_replay_state", {"size", size}, {"cursor", cursor});
  if (int e = replay_check(r, false)) return e;
  *size = r->ring.size;
  *cursor = r->ring.cursor;
  return 0;
}

int dqn_replay_extend(dqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* targets,
                      const float* priorities, int64_t n, int64_t* keys_out, void* stream) {
  if (const char* m = dqn_replay_host::check_extend(nullptr, n))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_extend: ") + m);
  CK_PTRS("dqn_replay_extend", {"obs", obs}, {"actions", actions}, {"targets", targets});
  if (int e = replay_check(r, true)) return e;
  if (const char* m = dqn_replay_host::check_extend(&r->ring, n))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_extend: ") + m);
  CK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = replay_copy_obs(r, obs, n, st)) return e;
  CK_KERNEL("replay_extend",
            dqn_replay_dev::launch_extend(actions, targets, priorities, n, r->ring.cursor, r->ring.cap, r->alpha,
                                          r->actions, r->targets, r->priorities, r->weights, r->maxp, keys_out, st));
  dqn_replay_host::advance(r->ring, n);
  return 0;
}

int dqn_replay_extend_rollout(dqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* rewards,
                              const uint8_t* done, const float* q_pi, const float* q_star, int64_t L,
                              int n_step, float gamma, int64_t* keys_out, void* stream) {
  if (const char* m = dqn_replay_host::check_rollout(nullptr, L, n_step, gamma))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_extend_rollout: ") + m);
  CK_PTRS("dqn_replay_extend_rollout", {"obs", obs}, {"actions", actions}, {"rewards", rewards}, {"done", done},
          {"q_pi", q_pi}, {"q_star", q_star});
  if (int e = replay_check(r, true)) return e;
  if (const char* m = dqn_replay_host::check_rollout(&r->ring, L, n_step, gamma))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_extend_rollout: ") + m);
  CK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t K = L - 1;
  if (int e = replay_copy_obs(r, obs, K, st)) return e;
  CK_KERNEL("replay_rollout",
            dqn_replay_dev::launch_rollout(actions, rewards, done, q_pi, q_star, K, n_step, gamma, r->ring.cursor,
                                           r->ring.cap, r->alpha, r->actions, r->targets, r->priorities,
                                           r->weights, r->maxp, keys_out, st));
  dqn_replay_host::advance(r->ring, K);
  return 0;
}

int dqn_replay_sample(dqn_replay* r, uint64_t seed, uint64_t counter, int64_t n, int64_t* keys,
                      float* probabilities, uint8_t* obs_out, int64_t* actions_out, float* targets_out,
                      void* stream) {
  if (const char* m = dqn_replay_host::check_sample(nullptr, n))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_sample: ") + m);
  CK_PTRS("dqn_replay_sample", {"keys", keys}, {"probabilities", probabilities});
  const bool gather = obs_out || actions_out || targets_out;
  if (gather && (!obs_out || !actions_out || !targets_out))
    return fail(IMPALA_E_INVALID, "dqn_replay_sample: obs_out, actions_out, targets_out: all or none");
  if (gather && ((uintptr_t)obs_out & 15) != 0)
    return fail(IMPALA_E_INVALID, "dqn_replay_sample: obs_out must be 16-byte aligned");
  if (int e = replay_check(r, true)) return e;
  if (const char* m = dqn_replay_host::check_sample(&r->ring, n))
    return fail(IMPALA_E_STATE, std::string("dqn_replay_sample: ") + m);
  CK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = replay_enqueue_draws(r, seed, counter, (int)n, keys, probabilities, st)) return e;
  if (!gather) return 0;
  return replay_enqueue_gather(r, keys, (int)n, obs_out, actions_out, targets_out, st);
}

int dqn_replay_update(dqn_replay* r, const int64_t* keys, const float* priorities, int64_t n, void* stream) {
  if (const char* m = dqn_replay_host::check_update(n))
    return fail(IMPALA_E_INVALID, std::string("dqn_replay_update: ") + m);
  CK_PTRS("dqn_replay_update", {"keys", keys}, {"priorities", priorities});
  if (int e = replay_check(r, true)) return e;
  CK(hipSetDevice(r->device));
  return replay_enqueue_update(r, keys, priorities, (int)n, (hipStream_t)stream);
}

int dqn_train_step_replay(dqn_learner* h, dqn_replay* r, uint64_t seed, uint64_t counter, int64_t* keys_out,
                          float* priorities_out, void* stream) {
  if (int e = dqn_check(h, true, false)) return e;
  if (int e = replay_check(r, true)) return e;
  impala_learner* c = h->core;
  if (r->device != c->device)
    return fail(IMPALA_E_INVALID, "dqn_train_step_replay: the replay and the learner are on different devices");
  if (r->ring.size < 1) return fail(IMPALA_E_STATE, "dqn_train_step_replay: the replay is empty (size 0)");
  CK(hipSetDevice(c->device));
  const int N = c->N;
  if (int e = replay_ensure_gather(r, N)) return e;
  hipStream_t st = (hipStream_t)stream;
  // the caller's arrays, where given, take the keys and the new priorities directly (no copies)
  int64_t* keys = keys_out ? keys_out : r->g_keys;
  float* prio = priorities_out ? priorities_out : r->g_prio;
  if (int e = replay_enqueue_draws(r, seed, counter, N, keys, r->g_prob, st)) return e;
  if (int e = replay_enqueue_gather(r, keys, N, r->g_obs, r->g_act, r->g_tgt, st)) return e;
  dqn_batch b{};
  b.obs = r->g_obs; b.actions = r->g_act; b.targets = r->g_tgt; b.probabilities = r->g_prob;
  b.priorities = prio;
  c->dqn_prio = b.priorities;
  const impala_batch ib = dqn_core_batch(&b);
  if (int e = enqueue_grads(c, &ib, st)) return e;
  if (int e = enqueue_update(c, st)) return e;
  return replay_enqueue_update(r, keys, prio, N, st);
}

int dqn_train_step_replay_rows(dqn_learner* h, dqn_replay* r, uint64_t seed, uint64_t counter,
                               int64_t* keys_out, float* priorities_out, void* stream) {
  if (int e = dqn_check(h, true, false)) return e;
  if (int e = replay_check(r, true)) return e;
  impala_learner* c = h->core;
  if (r->device != c->device)
    return fail(IMPALA_E_INVALID, "dqn_train_step_replay_rows: the replay and the learner are on different devices");
  if (r->ring.size < 1) return fail(IMPALA_E_STATE, "dqn_train_step_replay_rows: the replay is empty (size 0)");
  // only the default launches read the batch through the key map: the fused forward
  // (conv12_fwd_s2d), the dueling head and the fused per-frame backward (lnc3_conv12_bwd), whose
  // workgroups hold their frames' keys one per lane, as 32-bit rows (conv1.h, ObsKeysWg)
  const int N = c->N;
  const int fwd_fpw = c->c12f_fpw > 0 ? c->c12f_fpw : std::max(1, cdiv(N, c->n_cu));
  if (!c->lc12 || c->ln_fpw != c->c1_fpw || fwd_fpw > kObsKeysFpwMax || c->ln_fpw > kObsKeysFpwMax ||
      r->ring.cap > (int64_t)INT32_MAX)
    return fail(IMPALA_E_UNSUPPORTED, "dqn_train_step_replay_rows: not on the default kernel path");
  CK(hipSetDevice(c->device));
  if (int e = replay_ensure_scratch(r, N)) return e;
  hipStream_t st = (hipStream_t)stream;
  // the caller's arrays, where given, take the keys and the new priorities directly (no copies)
  int64_t* keys = keys_out ? keys_out : r->s_keys;
  float* prio = priorities_out ? priorities_out : r->s_prio;
  if (int e = replay_enqueue_draws(r, seed, counter, N, keys, r->s_prob, st)) return e;
  dqn_batch b{};  // the bound ring is the batch; transition f is its row keys[f]
  b.obs = r->obs; b.actions = r->actions; b.targets = r->targets; b.probabilities = r->s_prob;
  b.priorities = prio;
  c->dqn_prio = b.priorities;
  const impala_batch ib = dqn_core_batch(&b);
  static_assert(sizeof(long long) == sizeof(int64_t), "ObsKeys reads the int64 keys");
  c->obs_keys.keys = reinterpret_cast<const long long*>(keys);
  c->keys_on = true;
  int e = enqueue_grads(c, &ib, st);
  if (e == 0) e = enqueue_update(c, st);
  c->keys_on = false;
  if (e) return e;
  return replay_enqueue_update(r, keys, prio, N, st);
}

int dqn_replay_weights(dqn_replay* r, double* weights_out, float* max_priority_out, void* stream) {
  CK_PTRS("dqn_replay_weights", {"weights_out", weights_out});
  if (int e = replay_check(r, false)) return e;
  CK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  CK(hipMemcpyAsync(weights_out, r->weights, (size_t)r->ring.cap * 8, hipMemcpyDeviceToDevice, st));
  if (max_priority_out) CK(hipMemcpyAsync(max_priority_out, r->maxp, 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // extern "C"
