// Host side of the IQN C-ABI (include/iqn_hip.h).  Included at the end of impala.hip: an
// iqn_learner wraps an impala_learner created at the 512-wide projection (create_learner with
// ALGO_DQN), whose launch_forward it runs in trunk-only mode to obtain act3; the quantile head's
// kernels are csrc/iqn.hip's, launched through csrc/iqn_launch.h on rows the handle owns.
//
// The IQN flat layout is the dueling net's with Wq, bq (66,560 floats) inserted before the
// LayerNorm.  pack_params_kernel finds a parameter's segment by comparing its index with the
// Canon offsets in turn, so a Canon with a gap would send the inserted floats to the segment
// before the gap (b3, 64 entries); instead the handle keeps a staging buffer in the dueling layout,
// copies the two halves of a net's flat buffer into it (device copies, at bind / refresh only)
// and lets the core pack from there.  Wq and bq go through iqn_pack.
#pragma once
#include "../../include/iqn_hip.h"
#include "iqn_launch.h"

struct iqn_learner {
  impala_learner* core = nullptr;
  iqn_config cfg{};
  float *online = nullptr, *target = nullptr;  // caller-owned (iqn_bind_params)
  size_t gap = 0, ins = 0, total = 0;          // the inserted segment: [gap, gap + ins) of `total`
  int rows = 0;                                // batch_size * n_tau
  // library-owned, one allocation
  char* ws = nullptr;
  float* stage = nullptr;         // one net's parameters in the dueling layout (the core's `params`)
  float* target_params = nullptr; // = stage (TargetView)
  void* t_shadow = nullptr;       // the target net's kernel-layout weights, side vectors (TargetView)
  float* t_vecs = nullptr;
  float* t_heads = nullptr;       // = the core's (unused: the heads run on `work`)
  size_t shadow_bytes = 0, vecs_bytes = 0, wq_bytes = 0;
  void* wq[2] = {nullptr, nullptr};  // kernel-layout Wq, bq: online, target
  float* bq[2] = {nullptr, nullptr};
  iqn_dev::HeadWork work{};
  float* taus[2] = {nullptr, nullptr};  // [rows] the taus the library drew
  float* q[2] = {nullptr, nullptr};     // [rows][A] (iqn_act)
};

namespace {

int iqn_check(iqn_learner* h) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->online || !h->target) return fail(IMPALA_E_STATE, "iqn_bind_params() not called");
  return 0;
}

// one net's flat parameters -> its kernel-layout weights (under a TargetView: the target's)
int iqn_pack_net(iqn_learner* h, const float* flat, int which, hipStream_t st) {
  impala_learner* c = h->core;
  CK(hipMemcpyAsync(h->stage, flat, h->gap * 4, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->stage + h->gap, flat + h->gap + h->ins, (h->total - h->gap - h->ins) * 4,
                    hipMemcpyDeviceToDevice, st));
  {
    std::unique_ptr<TargetView> tv(which == 1 ? new TargetView(h) : nullptr);
    if (int r = BY_NET(c, launch_pack, c, st)) return r;
  }
  CK(iqn_dev::launch_pack(c->bf16, flat + h->gap, h->wq[which], h->bq[which], st));
  return 0;
}

int iqn_pack_both(iqn_learner* h, hipStream_t st) {
  if (int r = iqn_pack_net(h, h->online, 0, st)) return r;
  return iqn_pack_net(h, h->target, 1, st);
}

// q [n W][A] of net `which` into `q`; taus: the caller's, or drawn into the handle's buffer
int iqn_run_net(iqn_learner* h, const uint8_t* obs, int n, int which, const float* taus, uint64_t seed,
                uint64_t counter, float* q, float* taus_out, hipStream_t st) {
  using namespace net;
  impala_learner* c = h->core;
  const int W = h->cfg.n_tau, R = n * W;
  if (!taus) {
    CK(iqn_dev::launch_taus(seed, counter, which, R, h->taus[which], st));
    taus = h->taus[which];
  }
  if (taus_out && taus_out != taus)
    CK(hipMemcpyAsync(taus_out, taus, (size_t)R * 4, hipMemcpyDeviceToDevice, st));
  std::unique_ptr<TargetView> tv(which == 1 ? new TargetView(h) : nullptr);
  if (int r = BY_NET(c, launch_forward, c, obs, n, st, true)) return r;  // (trunk_only: act3)
  const size_t es = c->bf16 ? 2 : 4;
  const char* sw = (const char*)c->shadow;
  iqn_dev::HeadWeights w{};
  w.wq = h->wq[which]; w.bq = h->bq[which];
  w.gam = c->vecs + VecsDqn::lng; w.bet = c->vecs + VecsDqn::lnb;
  w.wfc = sw + c->sh.wfc * es; w.bfc = c->vecs + VecsDqn::bfc;
  w.wh = sw + c->sh.wh * es; w.bh = c->vecs + VecsDqn::bh;
  CK(iqn_dev::launch_head(c->bf16, w, h->work, c->act3, taus, R, W, c->A, c->n_cu, q, st));
  return 0;
}

int iqn_check_frames(iqn_learner* h, const uint8_t* obs, int n) {
  if (!obs) return fail(IMPALA_E_INVALID, "null pointer");
  if (n < 1 || n > h->cfg.batch_size) return fail(IMPALA_E_INVALID, "n must be in [1, batch_size]");
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  return 0;
}

}  // namespace

extern "C" {

int iqn_abi_version(void) { return IQN_ABI_VERSION; }
const char* iqn_last_error(void) { return g_err.c_str(); }

int iqn_config_default(iqn_config* c) {
  if (!c) return fail(IMPALA_E_INVALID, "null cfg");
  c->batch_size = 128;
  c->num_actions = 15;
  c->n_tau = 8;
  c->dtype = IMPALA_DTYPE_F32;
  return 0;
}

size_t iqn_param_count(int num_actions) {
  return net::canon_dqn(num_actions).total + (size_t)net::FLAT * IQN_COS + net::FLAT;
}

int iqn_create(const iqn_config* cfg, int device, iqn_learner** out) {
  using namespace net;
  if (!cfg || !out) return fail(IMPALA_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->n_tau < 1 || cfg->n_tau > IQN_MAX_TAU) return fail(IMPALA_E_INVALID, "n_tau must be in [1, 32]");
  if (cfg->num_actions < 1 || cfg->num_actions > MAX_A)
    return fail(IMPALA_E_UNSUPPORTED, "num_actions must be in [1, 15]");
  if (cfg->batch_size < 1 || (long long)cfg->batch_size * cfg->n_tau > IQN_MAX_ROWS)
    return fail(IMPALA_E_INVALID, "batch_size must be >= 1 and batch_size * n_tau <= 16384");
  if (cfg->dtype != IMPALA_DTYPE_F32 && cfg->dtype != IMPALA_DTYPE_BF16)
    return fail(IMPALA_E_INVALID, "unknown dtype");
  impala_config ic;
  impala_config_default(&ic);
  ic.batch_size = cfg->batch_size;
  ic.rollout_length = 1;
  ic.num_actions = cfg->num_actions;
  ic.dtype = cfg->dtype;
  ic.entropy_coeff = 0.f;
  ic.world_size = 1;
  ic.algo = ALGO_DQN;
  iqn_learner* h = new (std::nothrow) iqn_learner();
  if (!h) return fail(IMPALA_E_INVALID, "out of host memory");
  h->cfg = *cfg;
  if (int r = impala_internal::create_learner(&ic, device, HID_DQN, &h->core)) {
    delete h;
    return r;
  }
  impala_learner* c = h->core;
  c->trunk_only = true;
  h->gap = c->cn.lng;
  h->ins = (size_t)FLAT * IQN_COS + FLAT;
  h->total = c->cn.total + h->ins;
  h->rows = cfg->batch_size * cfg->n_tau;
  const size_t es = c->bf16 ? 2 : 4, R = (size_t)h->rows, A = (size_t)c->A;
  h->shadow_bytes = c->sh.total * es;
  h->vecs_bytes = VecsDqn::total * 4;
  h->wq_bytes = (size_t)FLAT * IQN_COS * es;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_stage = take(c->cn.total * 4), o_tsh = take(h->shadow_bytes), o_tv = take(h->vecs_bytes);
  const size_t o_wq0 = take(h->wq_bytes), o_wq1 = take(h->wq_bytes);
  const size_t o_bq0 = take(FLAT * 4), o_bq1 = take(FLAT * 4);
  const size_t o_y = take(R * YLD * es), o_zg = take(R * HID_DQN * 4), o_h = take(R * HID_DQN * es);
  const size_t o_heads = take(R * HEADS * 4);
  const size_t o_t0 = take(R * 4), o_t1 = take(R * 4), o_q0 = take(R * A * 4), o_q1 = take(R * A * 4);
  hipError_t e = hipMalloc(&h->ws, off);
  if (e == hipSuccess) e = hipMemset(h->ws, 0, off);
  if (e != hipSuccess) {
    iqn_destroy(h);
    return fail((int)e, std::string("iqn_create (workspace): ") + hipGetErrorString(e));
  }
  char* w = h->ws;
  h->stage = h->target_params = (float*)(w + o_stage);
  h->t_shadow = w + o_tsh;
  h->t_vecs = (float*)(w + o_tv);
  h->t_heads = c->heads;
  h->wq[0] = w + o_wq0; h->wq[1] = w + o_wq1;
  h->bq[0] = (float*)(w + o_bq0); h->bq[1] = (float*)(w + o_bq1);
  h->work.y = w + o_y; h->work.zg = (float*)(w + o_zg); h->work.h = w + o_h;
  h->work.heads = (float*)(w + o_heads);
  h->taus[0] = (float*)(w + o_t0); h->taus[1] = (float*)(w + o_t1);
  h->q[0] = (float*)(w + o_q0); h->q[1] = (float*)(w + o_q1);
  c->params = h->stage;  // what the core packs from (iqn_pack_net)
  *out = h;
  return 0;
}

int iqn_destroy(iqn_learner* h) {
  if (!h) return 0;
  if (h->core) {
    const int device = h->core->device;
    impala_destroy(h->core);  // (synchronises the device)
    (void)hipSetDevice(device);
  }
  if (h->ws) (void)hipFree(h->ws);
  delete h;
  return 0;
}

int iqn_bind_params(iqn_learner* h, float* online, float* target, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (!online || !target) return fail(IMPALA_E_INVALID, "null params pointer");
  h->online = online;
  h->target = target;
  CK(hipSetDevice(h->core->device));
  return iqn_pack_both(h, (hipStream_t)stream);
}

int iqn_sync_target(iqn_learner* h, void* stream) {
  if (int r = iqn_check(h)) return r;
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CK(hipMemcpyAsync(h->target, h->online, h->total * 4, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->t_shadow, c->shadow, h->shadow_bytes, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->t_vecs, c->vecs, h->vecs_bytes, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->wq[1], h->wq[0], h->wq_bytes, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(h->bq[1], h->bq[0], net::FLAT * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int iqn_refresh_weights(iqn_learner* h, void* stream) {
  if (int r = iqn_check(h)) return r;
  CK(hipSetDevice(h->core->device));
  return iqn_pack_both(h, (hipStream_t)stream);
}

int iqn_forward(iqn_learner* h, const uint8_t* obs, int n, int which, const float* taus, uint64_t seed,
                uint64_t counter, float* q, float* taus_out, void* stream) {
  if (which != 0 && which != 1) return fail(IMPALA_E_INVALID, "which must be 0 (online) or 1 (target)");
  if (int r = iqn_check(h)) return r;
  if (!q) return fail(IMPALA_E_INVALID, "null pointer");
  if (int r = iqn_check_frames(h, obs, n)) return r;
  CK(hipSetDevice(h->core->device));
  return iqn_run_net(h, obs, n, which, taus, seed, counter, q, taus_out, (hipStream_t)stream);
}

int iqn_act(iqn_learner* h, const uint8_t* obs, int n, const float* eps, float eps_all, uint64_t seed,
            uint64_t counter, const float* taus_online, const float* taus_target, int64_t* actions,
            float* q_pi, float* q_star, int64_t* greedy, void* stream) {
  if (int r = iqn_check(h)) return r;
  if (!actions || !q_pi || !q_star) return fail(IMPALA_E_INVALID, "null pointer");
  if (int r = iqn_check_frames(h, obs, n)) return r;
  impala_learner* c = h->core;
  if (c->A < 2) return fail(IMPALA_E_UNSUPPORTED, "iqn_act needs num_actions >= 2 (eps / (A - 1))");
  if (!eps && !(eps_all >= 0.f && eps_all <= 1.f)) return fail(IMPALA_E_INVALID, "eps must be in [0, 1]");
  CK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  // two forwards through the one workspace (same stream), each into its own q buffer
  if (int r = iqn_run_net(h, obs, n, 0, taus_online, seed, counter, h->q[0], nullptr, st)) return r;
  if (int r = iqn_run_net(h, obs, n, 1, taus_target, seed, counter, h->q[1], nullptr, st)) return r;
  CK(iqn_dev::launch_act(h->q[0], h->q[1], n, h->cfg.n_tau, c->A, eps, eps_all, seed, counter, actions, q_pi,
                         q_star, greedy, st));
  return 0;
}

int iqn_debug_read(iqn_learner* h, int which, void* dst, size_t bytes, void* stream) {
  using namespace net;
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  impala_learner* c = h->core;
  const size_t R = (size_t)h->rows, es = c->bf16 ? 2 : 4;
  const void* src = nullptr;
  size_t size = 0;
  switch (which) {  // the quantile head's rows (the carve-up in iqn_create); the trunk's are the core's
    case IMPALA_DBG_ACT1:
    case IMPALA_DBG_ACT2:
    case IMPALA_DBG_ACT3:
    case IMPALA_DBG_MASK1: return impala_debug_read(c, which, dst, bytes, stream);
    case IMPALA_DBG_Y: src = h->work.y; size = R * FLAT * es; break;
    case IMPALA_DBG_ZG: src = h->work.zg; size = R * HID_DQN * 4; break;
    case IMPALA_DBG_H: src = h->work.h; size = R * HID_DQN * es; break;
    case IMPALA_DBG_HEADS: src = h->work.heads; size = R * HEADS * 4; break;
    default: return fail(IMPALA_E_INVALID, "not a tensor of the IQN forward (act1-3, mask1, y, zg, h, heads)");
  }
  if (!dst) return fail(IMPALA_E_INVALID, "null destination");
  if (bytes == 0 || bytes > size) return fail(IMPALA_E_INVALID, "bytes must be in (0, the tensor's size]");
  static_assert(YLD == FLAT, "y's rows are exported as they lie: one copy");
  CK(hipSetDevice(c->device));
  CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

int iqn_nstep_targets(const float* rewards, const uint8_t* done, const float* q_pi, const float* q_star,
                      int64_t L, int W, int n_step, float gamma, float* targets, float* priorities,
                      void* stream) {
  if (L < 2) return fail(IMPALA_E_INVALID, "a rollout needs L >= 2 steps");
  if (W < 1 || W > IQN_MAX_TAU) return fail(IMPALA_E_INVALID, "W must be in [1, 32]");
  if (n_step < 1 || n_step > IQN_MAX_NSTEP) return fail(IMPALA_E_INVALID, "n_step must be in [1, 16]");
  if (!(gamma >= 0.f && gamma <= 1.f)) return fail(IMPALA_E_INVALID, "gamma must be in [0, 1]");
  if ((L - 1) * (int64_t)W > ((int64_t)1 << 30)) return fail(IMPALA_E_INVALID, "rollout too long");
  if (!rewards || !done || !q_pi || !q_star || !targets || !priorities)
    return fail(IMPALA_E_INVALID, "null pointer");
  CK(iqn_dev::launch_nstep(rewards, done, q_pi, q_star, (long long)(L - 1), W, n_step, gamma, targets,
                           priorities, (hipStream_t)stream));
  return 0;
}

int iqn_loss_head(const float* adv, const float* v, const int64_t* actions, const float* taus,
                  const float* targets, const float* probabilities, int N, int Ws, int Wt, int A,
                  float huber_param, float beta, float* dadv, float* dv, float* priorities, float* metrics4,
                  void* stream) {
  if (N < 1 || A < 1 || A > net::MAX_A) return fail(IMPALA_E_INVALID, "need N >= 1, 1 <= A <= 15");
  if (Ws < 1 || Ws > IQN_MAX_TAU || Wt < 1 || Wt > IQN_MAX_TAU)
    return fail(IMPALA_E_INVALID, "Ws and Wt must be in [1, 32]");
  if (!(huber_param >= 0.f)) return fail(IMPALA_E_INVALID, "huber_param must be >= 0");
  if (!adv || !v || !actions || !taus || !targets || !dadv || !dv || !priorities || !metrics4)
    return fail(IMPALA_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int wgs = cdiv(N, 256);
  float* part = nullptr;
  CK(hipMallocAsync((void**)&part, (size_t)wgs * 4 * 4, st));
  CK(iqn_dev::launch_loss_head(adv, v, actions, taus, targets, probabilities, N, Ws, Wt, A, huber_param, beta,
                               dadv, dv, priorities, part, metrics4, st));
  CK(hipFreeAsync(part, st));
  return 0;
}

}  // extern "C"
