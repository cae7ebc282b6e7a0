// Host side of the IQN C-ABI (include/iqn_hip.h).  Included at the end of impala.hip: an
// iqn_learner wraps an impala_learner created at the 512-wide projection (create_learner with
// ALGO_DQN), whose launch_forward it runs in trunk-only mode to obtain act3; the quantile head's
// kernels are csrc/iqn.hip's, launched through csrc/iqn_launch.h on rows the handle owns.  The
// training step (iqn_bind_state, iqn_train_step) runs the core's trunk forward, iqn.hip's step
// launches, then the core's own conv weight-gradient launch and slab reduction (iqn_alloc_step
// has how the reduction is pointed at the IQN flat order), and iqn.hip's Adam on that order.
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
  // ---- training (iqn_bind_state): the caller's state in the IQN flat order, the step's workspace
  // (one allocation, made at the first bind) and its launch plans ----
  bool train = false;
  iqn_optim opt{};
  float *grads = nullptr, *exp_avg = nullptr, *exp_avg_sq = nullptr, *metrics = nullptr;
  char* tws = nullptr;
  iqn_dev::StepWork step{};  // the workspace pointers and plans (the weights are filled per call)
  float* sumsq = nullptr;    // clip-norm partials: the core's reduction workgroups, then the inserted segment's
  int n_head_wg = 0, n_part = 0;
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

// The step's workspace and launch plans, and the core's slab reduction pointed at them.  The core
// handle was created for the dueling net on N frames; the quantile head's gradients come from R = N W
// rows, so the LayerNorm, FC and heads slabs are the step's own, and every segment past the gap is
// written `ins` floats further on: reduce_grads_kernel adds a segment's canonical offset on its
// write side, so the shifted offsets are all it takes.
int iqn_alloc_step(iqn_learner* h) {
  using namespace net;
  impala_learner* c = h->core;
  const int N = h->cfg.batch_size, W = h->cfg.n_tau, R = h->rows;
  const size_t es = c->bf16 ? 2 : 4;
  iqn_dev::StepWork& s = h->step;
  const int fc_base = c->bf16 ? 96 : 128;
  // FC weight gradient: 64 tiles; splits of about 512 rows, never fewer workgroups than the dueling step's
  const Split spfc = plan_split(R, (FLAT / 128) * (HID_DQN / 64), std::max(fc_base, 64 * cdiv(R, 512)));
  const Split spwq = plan_split(R, FLAT / 64, 256);
  s.fc_S = spfc.S; s.fc_mps = spfc.mps; s.wq_S = spwq.S; s.wq_mps = spwq.mps;
  // whole frames per workgroup, at least one 16-row tile's worth, two workgroups per CU at most
  s.ln_fpw = std::max(cdiv(16, W), cdiv(N, 2 * c->n_cu));
  s.ln_wgs = cdiv(N, s.ln_fpw);
  h->n_head_wg = iqn_dev::head_step_wgs(N, W);
  // the reduction table with the step's slabs (split-group rule of create_learner, 16 loads per
  // thread), planned on a copy: the core's own is replaced only once the workspace exists, so a failed
  // allocation leaves the handle as it was and a later bind plans from the unshifted table again
  RedArgs ra = c->red;
  const size_t ins = h->ins;
  auto set = [&](int i, int S, long long canon) {
    ra.seg[i].S = S;
    ra.seg[i].canon = canon;
  };
  set(RS_LN, s.ln_wgs, (long long)(c->cn.lng + ins));
  set(RS_FC, s.fc_S, (long long)(c->cn.wfc + ins));
  set(RS_FC + 1, s.fc_S, (long long)(c->cn.bfc + ins));
  set(RS_FC + 2, h->n_head_wg, 0);
  set(RS_FC + 3, h->n_head_wg, 0);
  for (size_t* f : {&ra.cn.lng, &ra.cn.lnb, &ra.cn.wfc, &ra.cn.bfc, &ra.cn.wa, &ra.cn.ba, &ra.cn.wc, &ra.cn.bc,
                    &ra.cn.total})
    *f += ins;
  for (int i = 0; i < RS_END; ++i) {
    int sg = 1;
    while (sg < 16 && sg * 16 < ra.seg[i].S) sg <<= 1;
    ra.seg[i].sg = sg;
    ra.wg_start[i + 1] = ra.wg_start[i] + cdiv(ra.seg[i].count / 4, 256 / sg);
  }
  const int n_red_wg = ra.wg_start[RS_END], n_part = n_red_wg + iqn_dev::ins_wgs();
  const size_t Rz = (size_t)R, nh = (size_t)h->n_head_wg;
  auto carve = [&](Arena a) {  // (every size is of the plan above, none of a pointer set here)
    auto F = [&](size_t bytes) { return (float*)a.take(bytes); };
    s.stats = F(Rz * 2 * 4);
    s.e = a.take(Rz * IQN_COS * es);
    s.dz = a.take(Rz * HID_DQN * es);
    s.dy = F(Rz * FLAT * 4);
    s.dpre = a.take(Rz * FLAT * es);
    s.dx = F((size_t)N * FLAT * 4);
    s.s_ln = F((size_t)s.ln_wgs * 2 * FLAT * 4);
    s.s_fc = F((size_t)s.fc_S * HID_DQN * FLAT * 4);
    s.s_bfc = F((size_t)s.fc_S * HID_DQN * 4);
    s.s_h = F(nh * HEADS * HID_DQN * 4);
    s.s_bh = F(nh * HEADS * 4);
    s.s_wq = F((size_t)s.wq_S * FLAT * IQN_COS * 4);
    s.s_bq = F((size_t)s.wq_S * FLAT * 4);
    s.loss_part = F(nh * 8 * 4);
    h->sumsq = F((size_t)(n_part + 3) / 4 * 16);  // zero tail: float4 reads
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  hipError_t e = hipMalloc(&h->tws, total);
  if (e == hipSuccess) e = hipMemset(h->tws, 0, total);
  if (e != hipSuccess) {
    if (h->tws) (void)hipFree(h->tws);
    h->tws = nullptr;
    return fail((int)e, std::string("iqn_bind_state (workspace): ") + hipGetErrorString(e));
  }
  carve(Arena{h->tws});
  s.fw = h->work;
  ra.seg[RS_LN].slab = s.s_ln;
  ra.seg[RS_FC].slab = s.s_fc;
  ra.seg[RS_FC + 1].slab = s.s_bfc;
  ra.seg[RS_FC + 2].slab = s.s_h;
  ra.seg[RS_FC + 3].slab = s.s_bh;
  ra.sumsq_part = h->sumsq;
  c->red = ra;
  c->n_red_wg = n_red_wg;
  h->n_part = n_part;
  return 0;
}

// forward, loss and backward of one batch: the pre-clip gradient in the bound grads (IQN flat order),
// the priorities and metrics 0..3; the step counter advances (iqn_train_step's first half, and all of
// iqn_compute_grads)
int iqn_enqueue_grads(iqn_learner* h, const iqn_batch* b, hipStream_t st) {
  using namespace net;
  if (int r = iqn_check(h)) return r;
  if (!h->train) return fail(IMPALA_E_STATE, "iqn_bind_state() not called");
  if (!b || !b->obs || !b->actions || !b->targets || !b->priorities)
    return fail(IMPALA_E_INVALID, "null batch pointer");
  if (((uintptr_t)b->obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  const int N = h->cfg.batch_size, W = h->cfg.n_tau, R = h->rows;
  const float* taus = b->taus;
  if (!taus) {
    CK(iqn_dev::launch_taus(b->seed, b->counter, 0, R, h->taus[0], st));
    taus = h->taus[0];
  }
  if (b->taus_out && b->taus_out != taus)
    CK(hipMemcpyAsync(b->taus_out, taus, (size_t)R * 4, hipMemcpyDeviceToDevice, st));
  if (int r = BY_NET(c, launch_forward, c, b->obs, N, st, true)) return r;  // (trunk_only: act3)
  const size_t es = c->bf16 ? 2 : 4;
  const char* sw = (const char*)c->shadow;
  iqn_dev::StepWork s = h->step;
  s.w.wq = h->wq[0]; s.w.bq = h->bq[0];
  s.w.gam = c->vecs + VecsDqn::lng; s.w.bet = c->vecs + VecsDqn::lnb;
  s.w.wfc = sw + c->sh.wfc * es; s.w.bfc = c->vecs + VecsDqn::bfc;
  s.w.wh = sw + c->sh.wh * es; s.w.bh = c->vecs + VecsDqn::bh;
  s.wht = sw + c->sh.wht * es;
  iqn_dev::TrunkBwd tb{};
  tb.act3 = c->act3; tb.w3 = sw + c->sh.w3 * es; tb.w3t = sw + c->sh.w3t * es; tb.act2 = c->act2;
  tb.w2 = sw + c->sh.w2 * es; tb.w2t = sw + c->sh.w2t * es; tb.dact3 = c->dact3; tb.dact2 = c->dact2;
  tb.obs = b->obs; tb.mask1 = c->mask1; tb.s_w1 = c->s_w1; tb.s_b1 = c->s_b1;
  tb.fpw = c->c1_fpw; tb.wgs = c->c1_wg;
  tb.act1 = c->act1; tb.s_w3 = c->s_w3; tb.s_b3 = c->s_b3; tb.s_w2 = c->s_w2; tb.s_b2 = c->s_b2;
  tb.S3 = c->sp3.S; tb.mps3 = c->sp3.mps; tb.S2 = c->sp2.S; tb.mps2 = c->sp2.mps;
  CK(iqn_dev::launch_step(c->bf16, s, tb, taus, b->actions, b->targets, b->probabilities, b->priorities, N, W, c->A,
                          h->opt.importance_sampling_exponent, h->opt.huber_param, c->n_cu, st));
  // Every segment of the core's table (the trunk's slabs, and the step's own past the gap); the
  // metrics and the step counter are the inserted segment's reduction's.  The reduction is reached
  // as a backward part with no stage in it (first > last), through the launch_backward
  // instantiations the core already has: naming reduce_segments<512> or wgrad23_kernel here moved
  // wgrad23_kernel and reduce_grads_kernel<512> to the end of impala.hip's code object and changed
  // the address of 26 of its 66 kernels (profiles/iqn_step/isa_cmp.txt), so the conv weight
  // gradients are launched from iqn.hip's own instantiation (launch_step) and nothing here names
  // a kernel of the core.
  const BwdPart reduce_only{-2, BS_C2_C1 + 1, BS_C2_C1, RS_CONV1, RS_END, 0};
  const impala_batch no_batch{};
  if (int r = BY_NET(c, launch_backward, c, &no_batch, st, &reduce_only)) return r;
  iqn_dev::RedInsArgs ra{};
  ra.s_wq = s.s_wq; ra.s_bq = s.s_bq; ra.S = s.wq_S;
  ra.grads_ins = h->grads + h->gap;
  ra.sumsq = h->sumsq + c->n_red_wg;
  ra.loss_part = s.loss_part; ra.n_loss_part = h->n_head_wg; ra.N = N;
  ra.metrics = h->metrics; ra.step = c->step;
  ra.lr = c->red.lr; ra.b1 = c->red.b1; ra.b2 = c->red.b2;
  ra.adam_sc = c->adam_sc;
  CK(iqn_dev::launch_reduce_ins(ra, 1, st));
  return 0;
}

// clip + Adam on the bound state, Wq / bq and the core's kernel-layout weights re-emitted
int iqn_enqueue_update(iqn_learner* h, hipStream_t st) {
  impala_learner* c = h->core;
  iqn_dev::AdamIns ai{};
  AdamArgs& aa = ai.a;
  aa.params = h->online; aa.grads = h->grads; aa.m = h->exp_avg; aa.v = h->exp_avg_sq;
  aa.metrics = h->metrics; aa.metrics_host = nullptr;
  aa.sumsq_part = h->sumsq; aa.n_part = h->n_part;
  aa.step = c->step;
  aa.sc = c->adam_sc; aa.b1 = c->red.b1; aa.b2 = c->red.b2;
  aa.eps = h->opt.adam_eps; aa.max_norm = h->opt.max_grad_norm;
  aa.inv_world = 1.f;
  aa.sp = ShadowPtrs{c->shadow, c->vecs, c->A};
  aa.cn = c->cn; aa.sh = c->sh;
  ai.fm = FlatGap{h->gap, h->ins};
  ai.wq = h->wq[0]; ai.bq = h->bq[0];
  const long rest = (long)c->cn.total - (long)(c->cn.bfc - c->cn.wfc);
  ai.grid = net::HID_DQN + cdiv(rest, 256);
  CK(iqn_dev::launch_adam(c->bf16, ai, st));
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
  iqn_learner* h = new (std::nothrow) iqn_learner();
  if (!h) return fail(IMPALA_E_INVALID, "out of host memory");
  h->cfg = *cfg;
  if (int r = create_q_core(cfg->batch_size, cfg->num_actions, cfg->dtype, nullptr, device, &h->core)) {
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
  auto carve = [&](Arena a) {
    auto F = [&](size_t bytes) { return (float*)a.take(bytes); };
    h->stage = h->target_params = F(c->cn.total * 4);
    h->t_shadow = a.take(h->shadow_bytes);
    h->t_vecs = F(h->vecs_bytes);
    h->wq[0] = a.take(h->wq_bytes);
    h->wq[1] = a.take(h->wq_bytes);
    h->bq[0] = F(FLAT * 4);
    h->bq[1] = F(FLAT * 4);
    h->work.y = a.take(R * YLD * es);
    h->work.zg = F(R * HID_DQN * 4);
    h->work.h = a.take(R * HID_DQN * es);
    h->work.heads = F(R * HEADS * 4);
    h->taus[0] = F(R * 4);
    h->taus[1] = F(R * 4);
    h->q[0] = F(R * A * 4);
    h->q[1] = F(R * A * 4);
    return Arena::align(a.used);
  };
  const size_t total = carve(Arena{});
  hipError_t e = hipMalloc(&h->ws, total);
  if (e == hipSuccess) e = hipMemset(h->ws, 0, total);
  if (e != hipSuccess) {
    iqn_destroy(h);
    return fail((int)e, std::string("iqn_create (workspace): ") + hipGetErrorString(e));
  }
  carve(Arena{h->ws});
  h->t_heads = c->heads;
  c->params = h->stage;  // what the core packs from (iqn_pack_net)
  *out = h;
  return 0;
}

int iqn_destroy(iqn_learner* h) {
  if (!h) return 0;
  destroy_q_core(h->core);
  if (h->ws) (void)hipFree(h->ws);
  if (h->tws) (void)hipFree(h->tws);
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
  if (int r = check_frames(h->core->N, obs, n)) return r;
  CK(hipSetDevice(h->core->device));
  return iqn_run_net(h, obs, n, which, taus, seed, counter, q, taus_out, (hipStream_t)stream);
}

int iqn_act(iqn_learner* h, const uint8_t* obs, int n, const float* eps, float eps_all, uint64_t seed,
            uint64_t counter, const float* taus_online, const float* taus_target, int64_t* actions,
            float* q_pi, float* q_star, int64_t* greedy, void* stream) {
  if (int r = iqn_check(h)) return r;
  if (!actions || !q_pi || !q_star) return fail(IMPALA_E_INVALID, "null pointer");
  if (int r = check_frames(h->core->N, obs, n)) return r;
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

int iqn_optim_default(iqn_optim* o) {
  if (!o) return fail(IMPALA_E_INVALID, "null optim");
  dqn_config d;
  dqn_config_default(&d);
  o->lr = d.lr;
  o->adam_beta1 = d.adam_beta1;
  o->adam_beta2 = d.adam_beta2;
  o->adam_eps = d.adam_eps;
  o->max_grad_norm = d.max_grad_norm;
  o->importance_sampling_exponent = d.importance_sampling_exponent;
  o->huber_param = 1.f;
  return 0;
}

int iqn_bind_state(iqn_learner* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                   float* metrics, const iqn_optim* optim, void* stream) {
  using namespace net;
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !metrics)
    return fail(IMPALA_E_INVALID, "null state pointer");
  iqn_optim o;
  iqn_optim_default(&o);
  if (optim) o = *optim;
  if (int r = check_optim(o.lr, o.adam_beta1, o.adam_beta2, o.adam_eps, o.max_grad_norm,
                          o.importance_sampling_exponent))
    return r;
  if (!(o.huber_param >= 0.f)) return fail(IMPALA_E_INVALID, "huber_param must be >= 0");
  impala_learner* c = h->core;
  CK(hipSetDevice(c->device));
  if (!h->tws) {
    if (int r = iqn_alloc_step(h)) return r;
  }
  h->opt = o;
  h->online = params;
  h->grads = grads; h->exp_avg = exp_avg; h->exp_avg_sq = exp_avg_sq; h->metrics = metrics;
  c->red.grads = grads;
  c->red.metrics = metrics;
  c->red.lr = dec(o.lr); c->red.b1 = dec(o.adam_beta1); c->red.b2 = dec(o.adam_beta2);
  h->train = true;
  return iqn_pack_net(h, h->online, 0, (hipStream_t)stream);
}

int iqn_set_metrics(iqn_learner* h, float* metrics) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  if (!metrics) return fail(IMPALA_E_INVALID, "null metrics pointer");
  h->metrics = metrics;
  h->core->red.metrics = metrics;
  return 0;
}

int iqn_set_step(iqn_learner* h, int64_t step, void* stream) {
  if (!h || !h->core) return fail(IMPALA_E_INVALID, "null handle");
  return impala_set_step(h->core, step, stream);
}

int iqn_compute_grads(iqn_learner* h, const iqn_batch* b, void* stream) {
  return iqn_enqueue_grads(h, b, (hipStream_t)stream);
}

int iqn_train_step(iqn_learner* h, const iqn_batch* b, void* stream) {
  if (int r = iqn_enqueue_grads(h, b, (hipStream_t)stream)) return r;
  return iqn_enqueue_update(h, (hipStream_t)stream);
}

int iqn_apply_update(iqn_learner* h, void* stream) {
  if (int r = iqn_check(h)) return r;
  if (!h->train) return fail(IMPALA_E_STATE, "iqn_bind_state() not called");
  CK(hipSetDevice(h->core->device));
  return iqn_enqueue_update(h, (hipStream_t)stream);
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
    case IMPALA_DBG_DACT3:
    case IMPALA_DBG_DACT2:
      if (!h->train) return fail(IMPALA_E_STATE, "a tensor of the training step: iqn_bind_state() not called");
      return impala_debug_read(c, which, dst, bytes, stream);
    case IMPALA_DBG_DZ: src = h->step.dz; size = R * HID_DQN * es; break;
    case IMPALA_DBG_DY: src = h->step.dy; size = R * FLAT * 4; break;
    case IMPALA_DBG_LNSTAT: src = h->step.stats; size = R * 2 * 4; break;
    case IQN_DBG_DPRE: src = h->step.dpre; size = R * FLAT * es; break;
    case IQN_DBG_DX: src = h->step.dx; size = (size_t)h->cfg.batch_size * FLAT * 4; break;
    case IQN_DBG_COS: src = h->step.e; size = R * IQN_COS * es; break;
    default:
      return fail(IMPALA_E_INVALID,
                  "not a tensor of the IQN net (act1-3, mask1, y, zg, h, heads; of the step: lnstat, cos, dz, dy, "
                  "dpre, dx, dact3, dact2)");
  }
  if (!src) return fail(IMPALA_E_STATE, "a tensor of the training step: iqn_bind_state() not called");
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
