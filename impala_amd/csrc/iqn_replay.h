// Host side of the device-side prioritized replay of the distributional (IQN) Ape-X learner
// (include/iqn_hip.h, iqn_replay_*).  Included at the end of impala.hip after iqn.h and
// dqn_replay.h: an iqn_replay owns a dqn_replay -- the ring's bookkeeping, the float64 weights, their
// block sums and the running maximum, sampled and updated by dqn_replay.hip's kernels through the
// helpers of dqn_replay.h -- and the width W of its target rows.  What W changes is the ingest (the
// two kernels of csrc/iqn_replay.hip behind csrc/iqn_replay_launch.h), the gather's third row size
// and the batch buffer; iqn_train_step_replay enqueues the step exactly as iqn_train_step does.  The
// width check, the ingest's launch shapes and the update's chunks are csrc/iqn_replay_host.h.
#pragma once
#include "../../include/iqn_hip.h"
#include "iqn_replay_host.h"
#include "iqn_replay_launch.h"

struct iqn_replay {
  dqn_replay* d = nullptr;  // owned (dqn_replay_create / dqn_replay_destroy)
  int W = 0;
  // library-owned gather buffer of one batch (iqn_train_step_replay)
  char* gbuf = nullptr;
  int g_rows = 0;
  uint8_t* g_obs = nullptr;
  int64_t *g_act = nullptr, *g_keys = nullptr;
  float *g_tgt = nullptr, *g_prob = nullptr, *g_prio = nullptr;
};

namespace {

int iqn_replay_check(const iqn_replay* r, bool bound) {
  if (!r || !r->d) return fail(IMPALA_E_INVALID, "null replay handle");
  if (bound && !r->d->obs) return fail(IMPALA_E_STATE, "iqn_replay_bind() not called");
  return 0;
}

int iqn_replay_enqueue_gather(iqn_replay* r, const int64_t* keys, int n, uint8_t* obs, int64_t* act, float* tgt,
                              hipStream_t st) {
  const dqn_replay* d = r->d;
  const void* src[3] = {d->obs, d->actions, d->targets};
  void* dst[3] = {obs, act, tgt};
  const size_t rb[3] = {kObsRowBytes, sizeof(int64_t), sizeof(float) * (size_t)r->W};
  return gather_launch(src, dst, rb, 3, keys, nullptr, n, st);
}

// the priority update at n keys: launches of at most DQN_MAX_BATCH keys, in order
int iqn_replay_enqueue_update(iqn_replay* r, const int64_t* keys, const float* prio, int n, hipStream_t st) {
  for (int i = 0; i < iqn_replay_host::update_chunks(n); ++i) {
    const iqn_replay_host::Chunk c = iqn_replay_host::update_chunk(n, i);
    if (int e = replay_enqueue_update(r->d, keys + c.off, prio + c.off, c.len, st)) return e;
  }
  return 0;
}

int iqn_replay_ensure_gather(iqn_replay* r, int n) {
  if (r->g_rows >= n) return 0;
  if (r->gbuf) CK(hipFree(r->gbuf));  // (synchronises: no launch still reads it)
  r->gbuf = nullptr;
  r->g_rows = 0;
  auto carve = [&](Arena a) {
    r->g_obs = (uint8_t*)a.take((size_t)n * kObsRowBytes);
    r->g_act = (int64_t*)a.take((size_t)n * 8);
    r->g_keys = (int64_t*)a.take((size_t)n * 8);
    r->g_tgt = (float*)a.take((size_t)n * r->W * 4);
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

}  // namespace

extern "C" {

int iqn_replay_create(int64_t capacity, int n_tau, double priority_exponent, int device, iqn_replay** out) {
  if (const char* m = iqn_replay_host::check_create(capacity, n_tau, priority_exponent))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_create: ") + m);
  if (device < 0) return fail(IMPALA_E_INVALID, "iqn_replay_create: device must be >= 0");
  CK_PTRS("iqn_replay_create", {"out", out});
  *out = nullptr;
  iqn_replay* r = new (std::nothrow) iqn_replay();
  if (!r) return fail(IMPALA_E_INVALID, "out of host memory");
  r->W = n_tau;
  if (int e = dqn_replay_create(capacity, priority_exponent, device, &r->d)) {
    delete r;
    return e;
  }
  *out = r;
  return 0;
}

int iqn_replay_destroy(iqn_replay* r) {
  if (!r) return 0;
  const int device = r->d ? r->d->device : 0;
  dqn_replay_destroy(r->d);  // (synchronises the device)
  (void)hipSetDevice(device);
  if (r->gbuf) (void)hipFree(r->gbuf);
  delete r;
  return 0;
}

int iqn_replay_bind(iqn_replay* r, uint8_t* obs, int64_t* actions, float* targets, float* priorities,
                    void* stream) {
  // (arguments first, then the handle: every check is reachable without a device)
  CK_PTRS("iqn_replay_bind", {"obs", obs}, {"actions", actions}, {"targets", targets}, {"priorities", priorities});
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "iqn_replay_bind: obs must be 16-byte aligned");
  if (int e = iqn_replay_check(r, false)) return e;
  return dqn_replay_bind(r->d, obs, actions, targets, priorities, stream);
}

int iqn_replay_state(const iqn_replay* r, int64_t* size, int64_t* cursor) {
  CK_PTRS("iqn_replay_state", {"size", size}, {"cursor", cursor});
  if (int e = iqn_replay_check(r, false)) return e;
  *size = r->d->ring.size;
  *cursor = r->d->ring.cursor;
  return 0;
}

int iqn_replay_extend(iqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* targets,
                      const float* priorities, int64_t n, int64_t* keys_out, void* stream) {
  if (const char* m = dqn_replay_host::check_extend(nullptr, n))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_extend: ") + m);
  CK_PTRS("iqn_replay_extend", {"obs", obs}, {"actions", actions}, {"targets", targets});
  if (int e = iqn_replay_check(r, true)) return e;
  dqn_replay* d = r->d;
  if (const char* m = dqn_replay_host::check_extend(&d->ring, n))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_extend: ") + m);
  CK(hipSetDevice(d->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = replay_copy_obs(d, obs, n, st)) return e;
  CK_KERNEL("iqn_replay_extend",
            iqn_replay_dev::launch_extend(actions, targets, priorities, n, r->W, d->ring.cursor, d->ring.cap,
                                          d->alpha, d->actions, d->targets, d->priorities, d->weights, d->maxp,
                                          keys_out, st));
  if (priorities)  // (rows at the running maximum do not raise it)
    CK_KERNEL("replay_raise_max",
              dqn_replay_dev::launch_raise_max(d->priorities, n, d->ring.cursor, d->ring.cap, d->maxp, st));
  dqn_replay_host::advance(d->ring, n);
  return 0;
}

int iqn_replay_extend_rollout(iqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* rewards,
                              const uint8_t* done, const float* q_pi, const float* q_star, int64_t L,
                              int n_step, float gamma, int64_t* keys_out, void* stream) {
  if (const char* m = dqn_replay_host::check_rollout(nullptr, L, n_step, gamma))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_extend_rollout: ") + m);
  CK_PTRS("iqn_replay_extend_rollout", {"obs", obs}, {"actions", actions}, {"rewards", rewards}, {"done", done},
          {"q_pi", q_pi}, {"q_star", q_star});
  if (int e = iqn_replay_check(r, true)) return e;
  dqn_replay* d = r->d;
  if (const char* m = dqn_replay_host::check_rollout(&d->ring, L, n_step, gamma))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_extend_rollout: ") + m);
  CK(hipSetDevice(d->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t K = L - 1;
  if (int e = replay_copy_obs(d, obs, K, st)) return e;
  CK_KERNEL("iqn_replay_rollout",
            iqn_replay_dev::launch_rollout(actions, rewards, done, q_pi, q_star, K, r->W, n_step, gamma,
                                           d->ring.cursor, d->ring.cap, d->alpha, d->actions, d->targets,
                                           d->priorities, d->weights, keys_out, st));
  CK_KERNEL("replay_raise_max",
            dqn_replay_dev::launch_raise_max(d->priorities, K, d->ring.cursor, d->ring.cap, d->maxp, st));
  dqn_replay_host::advance(d->ring, K);
  return 0;
}

int iqn_replay_sample(iqn_replay* r, uint64_t seed, uint64_t counter, int64_t n, int64_t* keys,
                      float* probabilities, uint8_t* obs_out, int64_t* actions_out, float* targets_out,
                      void* stream) {
  if (const char* m = dqn_replay_host::check_sample(nullptr, n))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_sample: ") + m);
  CK_PTRS("iqn_replay_sample", {"keys", keys}, {"probabilities", probabilities});
  const bool gather = obs_out || actions_out || targets_out;
  if (gather && (!obs_out || !actions_out || !targets_out))
    return fail(IMPALA_E_INVALID, "iqn_replay_sample: obs_out, actions_out, targets_out: all or none");
  if (gather && ((uintptr_t)obs_out & 15) != 0)
    return fail(IMPALA_E_INVALID, "iqn_replay_sample: obs_out must be 16-byte aligned");
  if (int e = iqn_replay_check(r, true)) return e;
  dqn_replay* d = r->d;
  if (const char* m = dqn_replay_host::check_sample(&d->ring, n))
    return fail(IMPALA_E_STATE, std::string("iqn_replay_sample: ") + m);
  CK(hipSetDevice(d->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = replay_enqueue_draws(d, seed, counter, (int)n, keys, probabilities, st)) return e;
  if (!gather) return 0;
  return iqn_replay_enqueue_gather(r, keys, (int)n, obs_out, actions_out, targets_out, st);
}

int iqn_replay_update(iqn_replay* r, const int64_t* keys, const float* priorities, int64_t n, void* stream) {
  if (const char* m = dqn_replay_host::check_update(n))
    return fail(IMPALA_E_INVALID, std::string("iqn_replay_update: ") + m);
  CK_PTRS("iqn_replay_update", {"keys", keys}, {"priorities", priorities});
  if (int e = iqn_replay_check(r, true)) return e;
  CK(hipSetDevice(r->d->device));
  return replay_enqueue_update(r->d, keys, priorities, (int)n, (hipStream_t)stream);
}

int iqn_replay_weights(iqn_replay* r, double* weights_out, float* max_priority_out, void* stream) {
  CK_PTRS("iqn_replay_weights", {"weights_out", weights_out});
  if (int e = iqn_replay_check(r, false)) return e;
  return dqn_replay_weights(r->d, weights_out, max_priority_out, stream);
}

int iqn_train_step_replay(iqn_learner* h, iqn_replay* r, uint64_t seed, uint64_t counter, const float* taus,
                          uint64_t tau_seed, uint64_t tau_counter, int64_t* keys_out, float* priorities_out,
                          float* taus_out, void* stream) {
  // every refusal comes before the first launch
  if (int e = iqn_check(h)) return e;
  if (!h->train) return fail(IMPALA_E_STATE, "iqn_bind_state() not called");
  if (int e = iqn_replay_check(r, true)) return e;
  impala_learner* c = h->core;
  dqn_replay* d = r->d;
  if (r->W != h->cfg.n_tau)
    return fail(IMPALA_E_INVALID, "iqn_train_step_replay: the replay's n_tau differs from the learner's");
  if (d->device != c->device)
    return fail(IMPALA_E_INVALID, "iqn_train_step_replay: the replay and the learner are on different devices");
  if (d->ring.size < 1) return fail(IMPALA_E_STATE, "iqn_train_step_replay: the replay is empty (size 0)");
  CK(hipSetDevice(c->device));
  const int N = h->cfg.batch_size;
  if (int e = iqn_replay_ensure_gather(r, N)) return e;
  hipStream_t st = (hipStream_t)stream;
  // the caller's arrays, where given, take the keys and the new priorities directly (no copies)
  int64_t* keys = keys_out ? keys_out : r->g_keys;
  float* prio = priorities_out ? priorities_out : r->g_prio;
  if (int e = replay_enqueue_draws(d, seed, counter, N, keys, r->g_prob, st)) return e;
  if (int e = iqn_replay_enqueue_gather(r, keys, N, r->g_obs, r->g_act, r->g_tgt, st)) return e;
  iqn_batch b{};
  b.obs = r->g_obs; b.actions = r->g_act; b.targets = r->g_tgt; b.probabilities = r->g_prob;
  b.taus = taus; b.priorities = prio; b.taus_out = taus_out;
  b.seed = tau_seed; b.counter = tau_counter;
  if (int e = iqn_enqueue_grads(h, &b, st)) return e;
  if (int e = iqn_enqueue_update(h, st)) return e;
  return iqn_replay_enqueue_update(r, keys, prio, N, st);
}

}  // extern "C"
