// Host side of the device-side prioritized replay of the distributional (IQN) Ape-X learner
// (include/iqn_hip.h, iqn_replay_*).  Included at the end of impala.hip after iqn.h and
// dqn_replay.h: an iqn_replay is dqn_replay.h's ring at W = n_tau targets per row, and every entry
// point it shares with dqn_replay is that header's body under the "iqn" prefix.  What is IQN's own
// is here: a priority update longer than one launch takes, and iqn_train_step_replay, which enqueues
// the step exactly as iqn_train_step does.
#pragma once
#include "../../include/iqn_hip.h"
#include "dqn_replay.h"

static_assert(dqn_replay_host::kMaxWidth == IQN_MAX_TAU, "dqn_replay_host::check_n_tau bounds n_tau by IQN_MAX_TAU");

struct iqn_replay : dqn_replay {};  // (a type of its own for the C header; no state beyond the ring)

namespace {

// the priority update at n keys: launches of at most DQN_MAX_BATCH keys, in order
int iqn_replay_enqueue_update(iqn_replay* r, const int64_t* keys, const float* prio, int n, hipStream_t st) {
  for (int i = 0; i < dqn_replay_host::update_chunks(n); ++i) {
    const dqn_replay_host::Chunk c = dqn_replay_host::update_chunk(n, i);
    if (int e = replay_enqueue_update(r, keys + c.off, prio + c.off, c.len, st)) return e;
  }
  return 0;
}

}  // namespace

extern "C" {

int iqn_replay_create(int64_t capacity, int n_tau, double priority_exponent, int device, iqn_replay** out) {
  return replay_create("iqn", capacity, n_tau, priority_exponent, device, out);
}

int iqn_replay_destroy(iqn_replay* r) { return replay_destroy(r); }

int iqn_replay_bind(iqn_replay* r, uint8_t* obs, int64_t* actions, float* targets, float* priorities,
                    void* stream) {
  return replay_bind("iqn", r, obs, actions, targets, priorities, stream);
}

int iqn_replay_state(const iqn_replay* r, int64_t* size, int64_t* cursor) {
  return replay_state("iqn", r, size, cursor);
}

int iqn_replay_extend(iqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* targets,
                      const float* priorities, int64_t n, int64_t* keys_out, void* stream) {
  return replay_extend("iqn", r, obs, actions, targets, priorities, n, keys_out, stream);
}

int iqn_replay_extend_rollout(iqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* rewards,
                              const uint8_t* done, const float* q_pi, const float* q_star, int64_t L,
                              int n_step, float gamma, int64_t* keys_out, void* stream) {
  return replay_extend_rollout("iqn", r, obs, actions, rewards, done, q_pi, q_star, L, n_step, gamma, keys_out,
                               stream);
}

int iqn_replay_sample(iqn_replay* r, uint64_t seed, uint64_t counter, int64_t n, int64_t* keys,
                      float* probabilities, uint8_t* obs_out, int64_t* actions_out, float* targets_out,
                      void* stream) {
  return replay_sample("iqn", r, seed, counter, n, keys, probabilities, obs_out, actions_out, targets_out, stream);
}

int iqn_replay_update(iqn_replay* r, const int64_t* keys, const float* priorities, int64_t n, void* stream) {
  return replay_update("iqn", r, keys, priorities, n, stream);
}

int iqn_replay_weights(iqn_replay* r, double* weights_out, float* max_priority_out, void* stream) {
  return replay_weights("iqn", r, weights_out, max_priority_out, stream);
}

int iqn_train_step_replay(iqn_learner* h, iqn_replay* r, uint64_t seed, uint64_t counter, const float* taus,
                          uint64_t tau_seed, uint64_t tau_counter, int64_t* keys_out, float* priorities_out,
                          float* taus_out, void* stream) {
  // every refusal comes before the first launch
  if (int e = iqn_check(h)) return e;
  if (!h->train) return fail(IMPALA_E_STATE, "iqn_bind_state() not called");
  if (int e = replay_check("iqn", r, true)) return e;
  impala_learner* c = h->core;
  if (r->W != h->cfg.n_tau)
    return fail(IMPALA_E_INVALID, "iqn_train_step_replay: the replay's n_tau differs from the learner's");
  if (r->device != c->device)
    return fail(IMPALA_E_INVALID, "iqn_train_step_replay: the replay and the learner are on different devices");
  if (r->ring.size < 1) return fail(IMPALA_E_STATE, "iqn_train_step_replay: the replay is empty (size 0)");
  CK(hipSetDevice(c->device));
  const int N = h->cfg.batch_size;
  if (int e = replay_ensure_gather(r, N)) return e;
  hipStream_t st = (hipStream_t)stream;
  // the caller's arrays, where given, take the keys and the new priorities directly (no copies)
  int64_t* keys = keys_out ? keys_out : r->g_keys;
  float* prio = priorities_out ? priorities_out : r->g_prio;
  if (int e = replay_enqueue_draws(r, seed, counter, N, keys, r->g_prob, st)) return e;
  if (int e = replay_enqueue_gather(r, keys, N, r->g_obs, r->g_act, r->g_tgt, st)) return e;
  iqn_batch b{};
  b.obs = r->g_obs; b.actions = r->g_act; b.targets = r->g_tgt; b.probabilities = r->g_prob;
  b.taus = taus; b.priorities = prio; b.taus_out = taus_out;
  b.seed = tau_seed; b.counter = tau_counter;
  if (int e = iqn_enqueue_grads(h, &b, st)) return e;
  if (int e = iqn_enqueue_update(h, st)) return e;
  return iqn_replay_enqueue_update(r, keys, prio, N, st);
}

}  // extern "C"
