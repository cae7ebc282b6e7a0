// Host side of the Ape-X DQN C-ABI (include/dqn_hip.h).  Included at the end of impala.hip: a
// dqn_learner is an impala_learner created at the 512-wide projection (create_learner with
// ALGO_DQN), so the trunk, FC, reduction and Adam launchers are the IMPALA step's own
// instantiated at HID_DQN, with dqn_head_step_kernel in head_step's slot -- plus a second set of
// kernel-layout weights and a heads buffer for the target net, which only act / forward read.
#pragma once
#include "../../include/dqn_hip.h"
#include "dqn_head.h"

struct dqn_learner {
  impala_learner* core = nullptr;
  dqn_config cfg{};
  float* target_params = nullptr;  // caller-owned (dqn_bind_target)
  // library-owned: the target net's kernel-layout weights, side vectors and heads output
  char* tws = nullptr;
  void* t_shadow = nullptr;
  float* t_vecs = nullptr;
  float* t_heads = nullptr;
  size_t shadow_bytes = 0, vecs_bytes = 0;
};

namespace {

// The core's launchers take an impala_batch.  A DQN batch travels in it by NAME, not by position:
// targets in `rewards`, the sampling probabilities (or null) in `discounts`; `behaviour_logits`
// is unused.  dqn_core_batch writes that mapping and launch_dqn_head reads it back; nothing else
// looks at those two fields on a DQN handle.
inline impala_batch dqn_core_batch(const dqn_batch* b) {
  impala_batch ib{};
  ib.obs = b->obs;
  ib.actions = b->actions;
  ib.rewards = b->targets;
  ib.discounts = b->probabilities;
  ib.behaviour_logits = nullptr;
  return ib;
}

template <typename T>
int launch_dqn_head(impala_learner* h, const impala_batch* b, hipStream_t st) {
  using namespace net;
  const T* sw = reinterpret_cast<const T*>(h->shadow);
  DqnHeadArgs ha{};
  ha.h = h->h; ha.zg = h->zg; ha.wh = sw + h->sh.wh; ha.wht = sw + h->sh.wht;
  ha.bh = h->vecs + VecsDqn::bh;
  // (dqn_core_batch's mapping)
  ha.act = b->actions; ha.tgt = b->rewards; ha.prob = b->discounts;
  ha.N = h->N; ha.A = h->A; ha.beta = h->dqn_beta;
  ha.dz = h->dz; ha.partials = h->loss_part; ha.slab_h = h->s_h; ha.slab_bh = h->s_bh;
  ha.prio = h->dqn_prio;
  if (h->keys_on)  // act / tgt are a replay ring read in place (instantiated in dqn_inplace.hip)
    return klaunch(h, K_HEAD_STEP, "head_step", dqn_inplace_dev::head_keys_kernel<T>(),
                   dim3(h->n_loss_wg, DQN_SPLIT), dim3(256), st, ha, h->obs_keys);
  return klaunch(h, K_HEAD_STEP, "head_step", dqn_head_step_kernel<T>, dim3(h->n_loss_wg, DQN_SPLIT),
                 dim3(256), st, ha);
}

// While alive, the core handle reads the target net: its flat parameters, kernel-layout weights,
// side vectors and heads buffer stand in for the online net's (host-side pointer swap).  Valid
// because the launchers read these four pointers from the handle at every call and nothing caches
// them: DQN entry points launch directly, never through the core's graph cache (run_graphed), and
// a handle serves one host thread at a time, as every handle of this library does.  Only
// launch_forward and launch_pack may run under a view.
struct TargetView {
  impala_learner* c;
  float *params, *vecs, *heads;
  void* shadow;
  template <class H>  // dqn_learner, iqn_learner (iqn.h)
  explicit TargetView(H* h) : c(h->core), params(c->params), vecs(c->vecs), heads(c->heads), shadow(c->shadow) {
    c->params = h->target_params; c->vecs = h->t_vecs; c->heads = h->t_heads; c->shadow = h->t_shadow;
  }
  ~TargetView() { c->params = params; c->vecs = vecs; c->heads = heads; c->shadow = shadow; }
};

int dqn_check(dqn_learner* h, bool train, bool target) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (int r = check_bound(h->core, train)) return r;
  if (target && !h->target_params) return fail(IMPALA_E_STATE, "dqn_bind_target() not called");
  return 0;
}

// ---- shared by the Q-learner handles: dqn_learner, and iqn_learner (iqn.h) ----
int check_frames(int core_N, const uint8_t* obs, int n) {
  if (!obs) return fail(IMPALA_E_INVALID, "null pointer");
  if (n < 1 || n > core_N) return fail(IMPALA_E_INVALID, "n must be in [1, batch_size]");
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  return 0;
}

int check_optim(float lr, float b1, float b2, float eps, float max_norm, float is_exponent) {
  if (!(lr >= 0.f) || !(eps > 0.f) || !(max_norm > 0.f) || !(b1 >= 0.f && b1 < 1.f) || !(b2 >= 0.f && b2 < 1.f))
    return fail(IMPALA_E_INVALID, "bad optimizer settings");
  if (!(is_exponent >= 0.f)) return fail(IMPALA_E_INVALID, "importance_sampling_exponent must be >= 0");
  return 0;
}

// The core of a Q-learner: an impala_learner on flat transitions at the 512-wide projection.
// optim: the handle's optimizer settings, or null where they arrive later (iqn_bind_state).
int create_q_core(int batch_size, int num_actions, int dtype, const dqn_config* optim, int device,
                  impala_learner** out) {
  impala_config ic;
  impala_config_default(&ic);
  ic.batch_size = batch_size;
  ic.rollout_length = 1;
  ic.num_actions = num_actions;
  ic.dtype = dtype;
  if (optim) {
    ic.lr = optim->lr; ic.adam_beta1 = optim->adam_beta1; ic.adam_beta2 = optim->adam_beta2;
    ic.adam_eps = optim->adam_eps;
    ic.max_grad_norm = optim->max_grad_norm;
  }
  ic.entropy_coeff = 0.f;
  ic.world_size = 1;
  ic.algo = ALGO_DQN;
  return impala_internal::create_learner(&ic, device, net::HID_DQN, out);
}

// destroys the core (null: nothing) and leaves its device current for the handle's own frees
void destroy_q_core(impala_learner* core) {
  if (!core) return;
  const int device = core->device;
  impala_destroy(core);  // (synchronises the device)
  (void)hipSetDevice(device);
}

// forward, loss and backward of one batch: the pre-clip gradient in the bound grads, the
// priorities and metrics 0..3 (dqn_train_step's first half, and all of dqn_compute_grads)
int dqn_enqueue_grads(dqn_learner* h, const dqn_batch* b, void* stream) {
  if (int r = dqn_check(h, true, false)) return r;
  if (!b || !b->obs || !b->actions || !b->targets || !b->priorities)
    return fail(IMPALA_E_INVALID, "null batch pointer");
  if (((uintptr_t)b->obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  c->dqn_prio = b->priorities;
  const impala_batch ib = dqn_core_batch(b);
  return enqueue_grads(c, &ib, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int dqn_abi_version(void) { return DQN_ABI_VERSION; }
const char* dqn_last_error(void) { return g_err.c_str(); }

int dqn_config_default(dqn_config* c) {
  if (!c) return fail(IMPALA_E_INVALID, "null cfg");
  c->batch_size = 512;
  c->num_actions = 15;
  c->dtype = IMPALA_DTYPE_F32;
  c->lr = 6.25e-5f;
  c->adam_beta1 = 0.9f;
  c->adam_beta2 = 0.999f;
  c->adam_eps = 1e-4f;
  c->max_grad_norm = 40.f;
  c->importance_sampling_exponent = 0.4f;
  return 0;
}

size_t dqn_param_count(int num_actions) { return net::canon_dqn(num_actions).total; }

int dqn_create(const dqn_config* cfg, int device, dqn_learner** out) {
  using namespace net;
  if (!cfg || !out) return fail(IMPALA_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->batch_size < 1 || cfg->batch_size > DQN_MAX_BATCH)
    return fail(IMPALA_E_INVALID, "batch_size must be in [1, 4096]");
  if (cfg->num_actions < 1 || cfg->num_actions > MAX_A)
    return fail(IMPALA_E_UNSUPPORTED, "num_actions must be in [1, 15]");
  if (cfg->dtype != IMPALA_DTYPE_F32 && cfg->dtype != IMPALA_DTYPE_BF16)
    return fail(IMPALA_E_INVALID, "unknown dtype");
  if (int r = check_optim(cfg->lr, cfg->adam_beta1, cfg->adam_beta2, cfg->adam_eps, cfg->max_grad_norm,
                          cfg->importance_sampling_exponent))
    return r;
  dqn_learner* h = new (std::nothrow) dqn_learner();
  if (!h) return fail(IMPALA_E_INVALID, "out of host memory");
  h->cfg = *cfg;
  if (int r = create_q_core(cfg->batch_size, cfg->num_actions, cfg->dtype, cfg, device, &h->core)) {
    delete h;
    return r;
  }
  h->core->dqn_beta = cfg->importance_sampling_exponent;
  const size_t es = h->core->bf16 ? 2 : 4;
  h->shadow_bytes = h->core->sh.total * es;
  h->vecs_bytes = VecsDqn::total * 4;
  auto carve = [&](Arena a) {
    h->t_shadow = a.take(h->shadow_bytes);
    h->t_vecs = (float*)a.take(h->vecs_bytes);
    h->t_heads = (float*)a.take((size_t)h->core->N * HEADS * 4);
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  hipError_t e = hipMalloc(&h->tws, total);
  if (e == hipSuccess) e = hipMemset(h->tws, 0, total);
  if (e != hipSuccess) {
    dqn_destroy(h);
    return fail((int)e, std::string("dqn_create (target net workspace): ") + hipGetErrorString(e));
  }
  carve(Arena{h->tws});
  *out = h;
  return 0;
}

int dqn_destroy(dqn_learner* h) {
  if (!h) return 0;
  destroy_q_core(h->core);
  if (h->tws) (void)hipFree(h->tws);
  delete h;
  return 0;
}

int dqn_bind_state(dqn_learner* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                   float* metrics, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  return impala_bind_state(h->core, params, grads, exp_avg, exp_avg_sq, metrics, stream);
}

int dqn_bind_target(dqn_learner* h, float* target_params, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (!target_params) return fail(IMPALA_E_INVALID, "null target_params pointer");
  h->target_params = target_params;
  CK(hipSetDevice(h->core->device));
  TargetView tv(h);
  return BY_NET(h->core, launch_pack, h->core, (hipStream_t)stream);
}

int dqn_sync_target(dqn_learner* h, void* stream) {
  if (int r = dqn_check(h, false, true)) return r;
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CK(hipMemcpyAsync(h->target_params, c->params, c->cn.total * 4, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->t_shadow, c->shadow, h->shadow_bytes, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->t_vecs, c->vecs, h->vecs_bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

int dqn_refresh_weights(dqn_learner* h, void* stream) {
  if (int r = dqn_check(h, false, false)) return r;
  if (int r = impala_refresh_weights(h->core, stream)) return r;
  if (!h->target_params) return 0;
  TargetView tv(h);
  return BY_NET(h->core, launch_pack, h->core, (hipStream_t)stream);
}

int dqn_set_step(dqn_learner* h, int64_t step, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  return impala_set_step(h->core, step, stream);
}
int dqn_set_metrics(dqn_learner* h, float* metrics) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  return impala_set_metrics(h->core, metrics);
}
int dqn_set_metrics_host(dqn_learner* h, float* host) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  return impala_set_metrics_host(h->core, host);
}

int dqn_forward(dqn_learner* h, const uint8_t* obs, int n, int which, float* q, void* stream) {
  if (which != 0 && which != 1) return fail(IMPALA_E_INVALID, "which must be 0 (online) or 1 (target)");
  if (int r = dqn_check(h, false, which == 1)) return r;
  if (!q) return fail(IMPALA_E_INVALID, "null pointer");
  if (int r = check_frames(h->core->N, obs, n)) return r;
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const float* heads = which == 1 ? h->t_heads : c->heads;
  {
    std::unique_ptr<TargetView> tv(which == 1 ? new TargetView(h) : nullptr);
    if (int r = BY_NET(c, launch_forward, c, obs, n, st, true)) return r;
  }
  dqn_q_kernel<<<cdiv(n, 256), 256, 0, st>>>(heads, n, c->A, q);
  CK_LAUNCH("dqn_q");
  return 0;
}

int dqn_act(dqn_learner* h, const uint8_t* obs, int n, const float* eps, float eps_all,
            uint64_t seed, uint64_t counter, int64_t* actions, float* q_pi, float* q_star,
            int64_t* greedy, void* stream) {
  if (int r = dqn_check(h, false, true)) return r;
  if (!actions || !q_pi || !q_star) return fail(IMPALA_E_INVALID, "null pointer");
  if (int r = check_frames(h->core->N, obs, n)) return r;
  impala_learner* c = h->core;
  if (c->A < 2) return fail(IMPALA_E_UNSUPPORTED, "dqn_act needs num_actions >= 2 (eps / (A - 1))");
  if (!eps && !(eps_all >= 0.f && eps_all <= 1.f)) return fail(IMPALA_E_INVALID, "eps must be in [0, 1]");
  CK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  // two forwards through the one workspace (same stream: the second starts after the first's
  // heads are written), each into its own heads buffer
  if (int r = BY_NET(c, launch_forward, c, obs, n, st, true)) return r;
  {
    TargetView tv(h);
    if (int r = BY_NET(c, launch_forward, c, obs, n, st, true)) return r;
  }
  dqn_act_kernel<<<cdiv(n, 256), 256, 0, st>>>(c->heads, h->t_heads, n, c->A, eps, eps_all, seed, counter,
                                               actions, q_pi, q_star, greedy);
  CK_LAUNCH("dqn_act");
  return 0;
}

int dqn_train_step(dqn_learner* h, const dqn_batch* b, void* stream) {
  if (int r = dqn_enqueue_grads(h, b, stream)) return r;
  return enqueue_update(h->core, (hipStream_t)stream);
}

int dqn_compute_grads(dqn_learner* h, const dqn_batch* b, void* stream) {
  return dqn_enqueue_grads(h, b, stream);
}

int dqn_debug_read(dqn_learner* h, int net, int which, void* dst, size_t bytes, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (net != 0 && net != 1) return fail(IMPALA_E_INVALID, "net must be 0 (online) or 1 (target)");
  if (net == 0 || which != IMPALA_DBG_HEADS) return impala_debug_read(h->core, which, dst, bytes, stream);
  // the one tensor the target net keeps to itself (the workspace serves both nets)
  if (!dst) return fail(IMPALA_E_INVALID, "null destination");
  const size_t size = (size_t)h->core->N * net::HEADS * 4;
  if (bytes == 0 || bytes > size) return fail(IMPALA_E_INVALID, "bytes must be in (0, the tensor's size]");
  CK(hipSetDevice(h->core->device));
  CK(hipMemcpyAsync(dst, h->t_heads, bytes, hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

int dqn_loss_head(const float* adv, const float* v, const int64_t* actions, const float* targets,
                  const float* probabilities, int N, int A, float beta, float* dadv, float* dv,
                  float* priorities, float* metrics4, void* stream) {
  if (N < 1 || A < 1 || A > net::MAX_A) return fail(IMPALA_E_INVALID, "need N >= 1, 1 <= A <= 15");
  if (!adv || !v || !actions || !targets || !dadv || !dv || !priorities || !metrics4)
    return fail(IMPALA_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int wgs = cdiv(N, 256);
  float* part = nullptr;
  CK(hipMallocAsync((void**)&part, (size_t)wgs * 8 * 4, st));
  dqn_loss_head_kernel<<<wgs, 256, 0, st>>>(adv, v, actions, targets, probabilities, N, A, beta, dadv,
                                            dv, priorities, part);
  CK_LAUNCH("dqn_loss_head");
  finalize_dqn_kernel<<<1, 64, 0, st>>>(part, wgs, N, metrics4);
  CK_LAUNCH("finalize_dqn");
  CK(hipFreeAsync(part, st));
  return 0;
}

}  // extern "C"
