// libimpala_hip.so — C-ABI of the MI355X-native IMPALA learner (see include/impala_hip.h).
//
// One handle = one learner replica on one device.  The handle owns the activation, gradient
// slab and kernel-layout weight workspaces (hipMalloc'd once at create, sized for B*T
// frames); the caller owns the canonical parameters, gradients, Adam moments and the metrics
// buffer (bound with impala_bind_state), so the Python host exposes them as ordinary torch
// tensors (state_dict, checkpoint, RCCL all-reduce) without copies.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <cctype>
#include <type_traits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/impala_hip.h"
#include "dqn_head.h"
#include "dqn_inplace_launch.h"
#include "head.h"
#include "host.h"
#include "hostpool.h"
#include "kernels.h"
#include "lnc3.h"
#include "ops.h"
#include "ppo_replay_launch.h"

namespace {
thread_local std::string g_err;
}  // namespace

// shared with the SAC translation unit (sac.hip) through csrc/host.h's fail: one last-error slot
// per thread for the library
namespace impala_internal {
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
// cfg->algo of the handle behind a dqn_learner (never accepted by impala_create)
constexpr int ALGO_DQN = 2;
int create_learner(const impala_config* cfg, int device, int hid, impala_learner** out);
}  // namespace impala_internal
using impala_internal::ALGO_DQN;

namespace {

inline int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}
// recover the decimal constant a float config value was written as (0.9f -> 0.9)
inline double dec(float x) {
  if (x == 0.f) return 0.0;
  const double e = std::floor(std::log10(std::fabs((double)x)));
  const double s = std::pow(10.0, 7.0 - e);
  return std::round((double)x * s) / s;
}

struct Split {
  int S = 1, mps = 32;  // splits, m per split
};
Split plan_split(long M, int tiles, int target_wgs, int chunk = 64) {
  Split s;
  const long chunks = (M + chunk - 1) / chunk;
  long S = (target_wgs + tiles - 1) / tiles;
  if (S < 1) S = 1;
  if (S > chunks) S = chunks;
  long mps = ((M + S - 1) / S + chunk - 1) / chunk * chunk;
  s.mps = (int)mps;
  s.S = (int)((M + mps - 1) / mps);
  return s;
}

}  // namespace

#include "stage.h"

// kernel ids for the live launch timer (impala_timer_*)
enum KernelId {
  K_CONV12_FWD = 0, K_CONV3_FWD, K_FC_FWD, K_HEADS_FWD, K_HEAD_STEP, K_LNC3_BWD, K_CONV3_WGRAD,
  K_CONV2_WGRAD, K_CONV12_BWD, K_REDUCE, K_SUMSQ, K_ADAM, K_FC_BWD, K_WGRAD23, K_CONV123_FWD,
  K_LNC12_BWD,
  K_COUNT
};
const char* const kKernelNames[K_COUNT] = {
    "conv1_fwd_conv2_fwd", "conv3_fwd", "fc_fwd", "heads_fwd", "head_step", "ln_bwd_conv3_dgrad",
    "conv3_wgrad", "conv2_wgrad", "conv2_dgrad_conv1_wgrad", "reduce_grads", "sumsq", "adam",
    "fc_wgrad_fc_dgrad", "conv3_wgrad_conv2_wgrad", "conv1_conv2_conv3_fwd",
    "ln_conv3_conv2_dgrad_conv1_wgrad"};

// the graph cache's key equality (GraphCache, host.h): a batch is its five addresses
static bool same_key(const impala_batch& a, const impala_batch& b) {
  return a.obs == b.obs && a.actions == b.actions && a.rewards == b.rewards &&
         a.discounts == b.discounts && a.behaviour_logits == b.behaviour_logits;
}

struct impala_learner {
  impala_config cfg;
  int device = 0;
  int N = 0;  // frames per step = B * T
  int A = 15;
  bool bf16 = false;
  int hid = net::HID_AC;  // projection width: the launchers' HID instantiation (BY_NET)
  net::Canon cn;
  net::Shadow sh;
  // caller-owned (bound)
  float *params = nullptr, *grads = nullptr, *exp_avg = nullptr, *exp_avg_sq = nullptr,
        *metrics = nullptr;
  float* metrics_host = nullptr;  // impala_set_metrics_host: the step's metrics also to host memory
  // impala_train_step_rows: while its launches are enqueued, the batch's frames are read from a
  // replay ring through obs_rows (conv12_fwd_s2d, head_step_kernel, lnc3_conv12_bwd)
  bool rows_on = false;
  ObsRows obs_rows{};
  // dqn_train_step_replay_rows: likewise through obs_keys, the keys the replay drew on the device
  // (the same three launches, instantiated in dqn_inplace.hip)
  bool keys_on = false;
  ObsKeys obs_keys{};
  // library-owned
  char* ws = nullptr;
  size_t ws_bytes = 0;
  void* shadow = nullptr;
  float* vecs = nullptr;
  void *act1, *act2, *act3, *y, *h, *dz, *dact3, *dact2;
  uint32_t* mask1;  // conv1 ReLU bit mask [N][225]
  float *lnstat, *zg, *heads, *dy;  // zg = gelu'(FC pre-activation)
  float *s_w1, *s_b1, *s_w2, *s_b2, *s_w3, *s_b3, *s_ln, *s_fc, *s_bfc, *s_h, *s_bh;
  float *loss_part, *sumsq_part, *adam_sc;
  int64_t* step;
  bool wg23_merged = true;    // conv3 + conv2 weight gradients in one launch (wgrad23_kernel)
  bool c3_tail = true;        // bf16: conv3 + LayerNorm as the tail of the fused conv1/conv2 forward
  bool lc12 = true;           // LayerNorm/conv3 dgrad + conv2 dgrad/conv1 wgrad in one launch
  Split sp1, sp2, sp3, spfc, sph;
  // n_red_wg: slab-reduction workgroups = clip-norm partials (one sum of squares each)
  int n_ln_wg = 0, ln_fpw = 0, n_loss_wg = 0, S_seg = 32, n_red_wg = 0;
  RedArgs red{};
  int n_cu = 256;
  int c1_fpw = 1, c1_wg = 1;  // conv1 wgrad: frames per workgroup, workgroups (= splits)
  int c12f_fpw = 0;           // conv1+conv2 forward frames per workgroup (0: N / CUs)
  float* vt_dbg = nullptr;    // impala_set_debug_vtrace: the step's V-trace outputs
  // DQN handles (dqn.h): the step's priorities output and the importance-sampling exponent
  float* dqn_prio = nullptr;
  float dqn_beta = 0.4f;
  // IQN handles (iqn.h): launch_forward stops after the conv trunk (act3); the quantile head runs
  // on the handle's own rows
  bool trunk_only = false;
  // live launch timer (impala_timer_*): per kernel id, event pairs handed to
  // hipExtLaunchKernel, which stamps the kernel's own start / end (as rocprofv3 does)
  struct KTimer {
    hipEvent_t* ev = nullptr;
    int cap = 0, n = 0;
    bool armed = false;
  };
  KTimer timers[K_COUNT];
  int timers_armed = 0, timer_last = -1;
  // device step clock (impala_step_clock): stamps[clock_i] by the next step's first kernel
  unsigned long long* clock_buf = nullptr;
  int clock_n = 0, clock_i = 0;
  // hipGraph replay of whole steps: the launch sequence of a step is captured once per batch
  // address set (on a private capture stream) and replayed with one hipGraphLaunch; the kinds
  // are G_GRADS, G_UPDATE, G_STEP, G_GRADS0 + part
  GraphCache<impala_batch, 8> graphs;
  bool use_graph = false;
  StageRing stage;  // host staging ring (impala_stage*, impala_slot_*): csrc/stage.h
  // native data-parallel step (impala_dp_*): the library's own RCCL communicator, so the
  // gradient all-reduces are enqueued with no host round trip and no c10d bookkeeping; the FC +
  // heads bucket is all-reduced on dp_stream while the per-frame backward runs
  ncclComm_t dp_comm = nullptr;
  hipStream_t dp_stream = nullptr;
  hipEvent_t dp_ev[3] = {nullptr, nullptr, nullptr};
  int dp_nranks = 0, dp_rank = -1;
};

namespace {
// persistent grid for gemm_tile: a few workgroups per CU, never more than the tile count
inline int persist_grid(const impala_learner* h, long tiles) {
  const long cap = (long)h->n_cu * 3;
  return (int)(tiles < cap ? tiles : cap);
}

// Every learner kernel is launched through klaunch: hipExtLaunchKernel, with the start / stop
// events of the live timer when kernel id `kid` is armed (the events then carry the kernel's
// own begin / end timestamps, so the timed duration excludes the launch and inter-kernel gap,
// as rocprofv3's kernel trace does).  Steps run without graph replay while a timer is armed.
template <typename... KArgs, typename... Args>
int klaunch(impala_learner* h, int kid, const char* name, void (*kernel)(KArgs...), dim3 grid,
            dim3 block, hipStream_t st, Args... args) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kid >= 0) {
    auto& t = h->timers[kid];
    if (t.armed && t.n < t.cap) {
      e0 = t.ev[2 * t.n];
      e1 = t.ev[2 * t.n + 1];
      t.n++;
    }
  }
  hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, args...);
  CK_LAUNCH(name);
  return 0;
}
}  // namespace

namespace {

// the device step clock's slot for the step being enqueued (nullptr: not armed / full)
unsigned long long* step_stamp(impala_learner* h) {
  return h->clock_buf && h->clock_i < h->clock_n ? h->clock_buf + h->clock_i++ : nullptr;
}

// The launchers are instantiated per compute type and projection width; BY_NET picks the
// handle's instantiation.
#define BY_NET(h, fn, ...)                                                                   \
  ((h)->hid == net::HID_DQN                                                                  \
       ? ((h)->bf16 ? fn<__bf16, net::HID_DQN>(__VA_ARGS__) : fn<float, net::HID_DQN>(__VA_ARGS__)) \
       : ((h)->bf16 ? fn<__bf16, net::HID_AC>(__VA_ARGS__) : fn<float, net::HID_AC>(__VA_ARGS__)))

template <typename T, int HID>
int launch_forward(impala_learner* h, const uint8_t* obs, int n, hipStream_t st,
                   bool with_heads) {
  using namespace net;
  using Vecs = VecsT<HID>;
  // K chunk of the LDS-staged tile GEMM: long chunks (few, each a full memory round trip) for
  // bf16; fp32 at most 64 (round-3 A/B: 32 -> 64 cut fc_fwd 18.2 -> 14.0 us and
  // conv3_fwd 28.3 -> 27.0 us; 128 / 256 lost on conv3_fwd's LDS footprint)
#define BK(kb) (sizeof(T) == 4 ? ((kb) < 64 ? (kb) : 64) : (kb))
  const T* sw = reinterpret_cast<const T*>(h->shadow);
  const Shadow& sh = h->sh;
  const float* vv = h->vecs;
  // conv1 + conv2 per frame (act1 consumed from LDS)
  const int fpw = h->c12f_fpw > 0 ? h->c12f_fpw : std::max(1, cdiv(n, h->n_cu));
  // at most c3t_fmax<T>() frames per workgroup (bf16 6, fp32 5): conv3 + ReLU + LayerNorm
  // run as the kernel's tail (one launch for the whole conv trunk)
  C3Tail<T> c3{};
  bool conv3_done = false;
  if (h->c3_tail && fpw <= c3t_fmax<T>()) {
    c3.w3 = sw + sh.w3; c3.b3 = vv + Vecs::b3; c3.gam = vv + Vecs::lng; c3.bet = vv + Vecs::lnb;
    c3.act3 = (T*)h->act3; c3.y = (T*)h->y; c3.stats = h->lnstat;
    conv3_done = true;
  }
  // the frames from the batch arrays, or (impala_train_step_rows) from a replay ring in place
  auto fwd = [&](const auto& rm) {
    using O = std::decay_t<decltype(rm)>;
    return klaunch(h, conv3_done ? K_CONV123_FWD : K_CONV12_FWD, "conv12_fwd", conv12_fwd_s2d<T, O>,
                   dim3(cdiv(n, fpw)), dim3(c12f_threads<T>()), st, obs, sw + sh.w1,
                   vv + Vecs::b1, sw + sh.w2, vv + Vecs::b2, (T*)h->act1, h->mask1,
                   (T*)h->act2, n, fpw, c3, with_heads ? nullptr : step_stamp(h), rm);
  };
  if (h->keys_on && !with_heads) {  // (instantiated in dqn_inplace.hip)
    if (int r = klaunch(h, conv3_done ? K_CONV123_FWD : K_CONV12_FWD, "conv12_fwd",
                        dqn_inplace_dev::fwd_keys_kernel<T>(), dim3(cdiv(n, fpw)), dim3(c12f_threads<T>()), st,
                        obs, sw + sh.w1, vv + Vecs::b1, sw + sh.w2, vv + Vecs::b2, (T*)h->act1, h->mask1,
                        (T*)h->act2, n, fpw, c3, step_stamp(h), h->obs_keys))
      return r;
  } else if (int r = h->rows_on && !with_heads ? fwd(h->obs_rows) : fwd(ObsDirect{})) return r;
  if (!conv3_done) {  // more frames per workgroup than the tail takes, or IMPALA_C3_TAIL=0
    Conv3LnFwd<T> op{};
    op.C = n * P3; op.w = sw + sh.w3; op.b = vv + Vecs::b3; op.x = (const T*)h->act2;
    op.out = (T*)h->act3; op.gam = vv + Vecs::lng; op.bet = vv + Vecs::lnb; op.y = (T*)h->y;
    op.stats = h->lnstat;
    op.frames_per_tile = 64 / P3;
    if (int r = klaunch(h, K_CONV3_FWD, "conv3_fwd", gemm_tile<T, 64, 64, BK(96), 2, 2, Conv3LnFwd<T>>,
                        dim3(persist_grid(h, cdiv((long)n * P3, 64))), dim3(256), st, op, 1))
      return r;
  }
  // (the conv tail's own y and LayerNorm statistics are computed and unused)
  if (h->trunk_only) return 0;
  {
    FcFwd<T, HID> op{n, sw + sh.wfc, vv + Vecs::bfc, (const T*)h->y, h->zg, (T*)h->h};
    using C = FcFwdCfg<T>;
    if (int r = klaunch(h, K_FC_FWD, "fc_fwd",
                        gemm_tile<T, C::BR, C::BC, C::BK, 2, C::NW / 2, FcFwd<T, HID>, C::PF, C::KW>,
                        dim3(persist_grid(h, (long)cdiv(n, C::BC) * (HID / C::BR))), dim3(64 * C::NW), st,
                        op, HID / C::BR))
      return r;
  }
  if (with_heads) {  // inference; in training the fused head kernel computes the heads
    HeadsFwd<T, HID> op{n, sw + sh.wh, vv + Vecs::bh, (const T*)h->h, h->heads};
    if (int r = klaunch(h, K_HEADS_FWD, "heads_fwd", gemm_rc<T, 1, 1, HeadsFwd<T, HID>>,
                        dim3(cdiv(n, 64), 1), dim3(256), st, op))
      return r;
  }
  return 0;
}

// slab-reduction segment groups (indices into RedArgs::seg, in the order create() adds them)
enum { RS_CONV1 = 0, RS_CONV2 = 2, RS_CONV3 = 4, RS_LN = 6, RS_FC = 7, RS_END = 11 };

template <int HID>
int reduce_segments(impala_learner* h, int s_lo, int s_hi, hipStream_t st, int fin) {
  const int n = h->red.wg_start[s_hi] - h->red.wg_start[s_lo];
  return klaunch(h, K_REDUCE, "reduce_grads", reduce_grads_kernel<HID>, dim3(n), dim3(256), st, h->red,
                 s_lo, fin);
}

// The backward is three stages on one stream:
//   head_fc  head_step_kernel (heads forward, loss, dz, heads weight gradient), then the FC
//            weight and input gradients (fc_bwd_kernel)
//   ln_c3    LayerNorm backward + conv3 dgrad, and the conv3 weight gradient
//   c2_c1    conv2 weight gradient, and conv2 dgrad + conv1 wgrad
// A part runs a range of stages, then one reduction of the slab segments those stages (and no
// earlier part) completed; `fin` also finalises the loss metrics and the step counter.  -1 is
// the whole backward.  Data-parallel replicas all-reduce a reduced gradient bucket while the
// next part runs: 0 then 1 (buckets [cn.w3, total) and [0, cn.w3)), 2 / 3 / 4 (FC + heads,
// conv3 + LayerNorm, conv1 + conv2), or 2 then 6 (the native step: [cn.wfc, total) and
// [0, cn.wfc)).  Any split gives bit-identical gradients (each reduction workgroup owns a
// fixed sum-of-squares slot).
enum BwdStage { BS_HEAD_FC = 0, BS_LN_C3, BS_C2_C1 };
struct BwdPart {
  int part, first, last, red_lo, red_hi, fin;
};
constexpr BwdPart kBwdParts[] = {
    {-1, BS_HEAD_FC, BS_C2_C1, RS_CONV1, RS_END, 1},
    {0, BS_HEAD_FC, BS_LN_C3, RS_CONV3, RS_END, 0},
    {1, BS_C2_C1, BS_C2_C1, RS_CONV1, RS_CONV3, 1},
    {2, BS_HEAD_FC, BS_HEAD_FC, RS_FC, RS_END, 0},
    {3, BS_LN_C3, BS_LN_C3, RS_CONV3, RS_FC, 0},
    {4, BS_C2_C1, BS_C2_C1, RS_CONV1, RS_CONV3, 1},
    {6, BS_LN_C3, BS_C2_C1, RS_CONV1, RS_FC, 1},
};
const BwdPart* bwd_part(int part) {
  for (const BwdPart& p : kBwdParts)
    if (p.part == part) return &p;
  return nullptr;
}

template <typename T>
int launch_dqn_head(impala_learner* h, const impala_batch* b, hipStream_t st);

template <typename T, int HID>
int launch_backward(impala_learner* h, const impala_batch* b, hipStream_t st, const BwdPart* bp) {
  using namespace net;
  using Vecs = VecsT<HID>;
  const int N = h->N, B = h->cfg.batch_size, Tl = h->cfg.rollout_length;
  const T* sw = reinterpret_cast<const T*>(h->shadow);
  const Shadow& sh = h->sh;
  // gemm_wg: 32-row m-chunks, several 4-wave groups per workgroup on interleaved chunks (more
  // chunk loads in flight per CU); fp32 keeps one group for its LDS budget.  The bf16 conv
  // weight gradients run 2 groups (56 KB of LDS: two workgroups per CU) rather than 4 (112 KB:
  // one, so the merged launch's 508 workgroups ran in two rounds): 17.1 -> 14.0 us, step 0.1029
  // -> 0.1000 ms (profiles/r05bg).  The bf16 FC weight gradient keeps 2
  // (one group: 8.2 -> 8.9 us).
  constexpr int WG4 = sizeof(T) == 2 ? 2 : 1, WG2 = sizeof(T) == 2 ? 2 : 1;
  // The two cross-stage fusions need ln_c3 and c2_c1 in one range (the data-parallel parts 0 / 1
  // and 3 / 4 end a gradient bucket between them): conv3 + conv2 weight gradients in one launch,
  // and the two per-frame chains in one launch (same frame runs)
  const bool both = bp->first <= BS_LN_C3 && bp->last == BS_C2_C1;
  const bool wg23 = h->wg23_merged && both;
  const bool lc12 = h->lc12 && h->ln_fpw == h->c1_fpw && both;

  // ---- head_fc: heads fwd, log-softmax / V-trace / loss, dz, heads weight gradient; then the
  // FC weight and input gradients ----
  auto head_fc = [&]() -> int {
    HeadArgs ha{};
    ha.h = h->h; ha.zg = h->zg; ha.wh = sw + sh.wh; ha.wht = sw + sh.wht;
    ha.bh = h->vecs + Vecs::bh;
    ha.act = b->actions; ha.rew = b->rewards; ha.disc = b->discounts; ha.mu = b->behaviour_logits;
    ha.B = B; ha.T = Tl; ha.A = h->A; ha.S = h->S_seg; ha.TPW = 64 / h->S_seg;
    ha.lam = h->cfg.vtrace_lambda; ha.crho = h->cfg.clip_rho_threshold;
    ha.cpg = h->cfg.clip_pg_rho_threshold; ha.ent_coef = h->cfg.entropy_coeff;
    ha.vt_mode = h->cfg.vtrace_grad_mode;
    ha.dz = h->dz; ha.partials = h->loss_part; ha.slab_h = h->s_h; ha.slab_bh = h->s_bh;
    ha.heads_out = h->heads;
    ha.vt_dbg = h->cfg.algo == IMPALA_ALGO_PPO ? nullptr : h->vt_dbg;
    // torch.clamp(ratio, 1 - clip, 1 + clip): the bounds are python floats cast to fp32
    ha.clip_lo = (float)(1.0 - (double)h->cfg.ppo_clip);
    ha.clip_hi = (float)(1.0 + (double)h->cfg.ppo_clip);
    const dim3 hg(h->n_loss_wg, head_split<T>());
    if constexpr (HID == HID_DQN) {  // the dueling head in head_step's slot (dqn_head.h)
      if (int r = launch_dqn_head<T>(h, b, st)) return r;
    } else if (int r = h->cfg.algo == IMPALA_ALGO_PPO
                    ? (h->rows_on ? klaunch(h, K_HEAD_STEP, "head_step",
                                            ppo_replay_dev::head_rows_kernel(sizeof(T) == 2), hg, dim3(256),
                                            st, ha, h->obs_rows)  // (instantiated in ppo_replay.hip)
                                  : klaunch(h, K_HEAD_STEP, "head_step", head_step_kernel<T, true>, hg, dim3(256),
                                            st, ha, ObsDirect{}))
                    : h->rows_on
                    ? klaunch(h, K_HEAD_STEP, "head_step", head_step_kernel<T, false, ObsRows>, hg, dim3(256),
                              st, ha, h->obs_rows)
                    : klaunch(h, K_HEAD_STEP, "head_step", head_step_kernel<T, false>, hg, dim3(256), st, ha,
                              ObsDirect{}))
      return r;
    FcWgrad<T, HID> ow{};
    ow.M = N; ow.x = (const T*)h->dz; ow.y = (const T*)h->y;
    FcDgrad<T, HID> od{N, sw + sh.wfc, (const T*)h->dz, h->dy};
    using C = FcBwdCfg<T, WG2, HID>;
    const int gx = FLAT / C::WBC, gy = HID / 64, gz = h->spfc.S;
    const int n_rt = FLAT / C::DR, n_dt = n_rt * cdiv(N, C::DC);
    return klaunch(h, K_FC_BWD, "fc_wgrad_fc_dgrad", fc_bwd_kernel<T, WG2, HID>,
                   dim3(gx * gy * gz + n_dt), dim3(256 * WG2), st, ow, h->s_fc, h->s_bfc,
                   h->spfc.mps, gx, gy, gz, od, n_rt);
  };

  // ---- ln_c3: LayerNorm backward + conv3 dgrad (with lc12, c2_c1's per-frame kernel too), and
  // the conv3 weight gradient (with wg23, conv2's too) ----
  auto ln_c3 = [&]() -> int {
    if (lc12) {
      auto bwd = [&](const auto& rm) {
        using O = std::decay_t<decltype(rm)>;
        return klaunch(h, K_LNC12_BWD, "ln_conv3_conv2_dgrad_conv1_wgrad", lnc3_conv12_bwd<T, O>,
                       dim3(h->n_ln_wg), dim3(lnc3_threads<T>()), st, (const float*)h->dy,
                       (const T*)h->act3, (const float*)h->lnstat,
                       (const float*)(h->vecs + Vecs::lng), sw + sh.w3, sw + sh.w3t,
                       (const T*)h->act2, (T*)h->dact3, (T*)h->dact2, h->s_ln, b->obs,
                       sw + sh.w2, sw + sh.w2t, (const uint32_t*)h->mask1, h->s_w1, h->s_b1, N,
                       h->ln_fpw, rm);
      };
      if (h->keys_on) {  // (instantiated in dqn_inplace.hip)
        if (int r = klaunch(h, K_LNC12_BWD, "ln_conv3_conv2_dgrad_conv1_wgrad",
                            dqn_inplace_dev::bwd_keys_kernel<T>(), dim3(h->n_ln_wg), dim3(lnc3_threads<T>()), st,
                            (const float*)h->dy, (const T*)h->act3, (const float*)h->lnstat,
                            (const float*)(h->vecs + Vecs::lng), sw + sh.w3, sw + sh.w3t, (const T*)h->act2,
                            (T*)h->dact3, (T*)h->dact2, h->s_ln, b->obs, sw + sh.w2, sw + sh.w2t,
                            (const uint32_t*)h->mask1, h->s_w1, h->s_b1, N, h->ln_fpw, h->obs_keys))
          return r;
      } else if (int r = h->rows_on ? bwd(h->obs_rows) : bwd(ObsDirect{})) return r;
    } else {  // LayerNorm backward + conv3 dgrad per frame
      if (int r = klaunch(h, K_LNC3_BWD, "ln_bwd_conv3_dgrad", lnc3_bwd<T>, dim3(h->n_ln_wg),
                          dim3(lnc3_threads<T>()), st, (const float*)h->dy, (const T*)h->act3,
                          (const float*)h->lnstat, (const float*)(h->vecs + Vecs::lng), sw + sh.w3,
                          sw + sh.w3t, (const T*)h->act2, (T*)h->dact3, (T*)h->dact2, h->s_ln, N,
                          h->ln_fpw))
        return r;
    }
    Conv3Wgrad<T> o3{};
    o3.M = N * P3; o3.x = (const T*)h->dact3; o3.in = (const T*)h->act2;
    if (wg23) {  // conv2's weight gradient reads dact2, which the per-frame kernel has written
      Conv2Wgrad<T> o2{};
      o2.M = N * P2; o2.x = (const T*)h->dact2; o2.in = (const T*)h->act1;
      const int g3x = K3 / 64, g3z = h->sp3.S, g2x = K2 / Wg2Tile<T>::BC, g2z = h->sp2.S;
      return klaunch(h, K_WGRAD23, "conv3_wgrad_conv2_wgrad", wgrad23_kernel<T, WG4>,
                     dim3(g3x * g3z + g2x * g2z), dim3(256 * WG4), st, o3, h->s_w3, h->s_b3,
                     h->sp3.mps, g3x, g3z, o2, h->s_w2, h->s_b2, h->sp2.mps, g2x, g2z);
    }
    // 64 x 64 tiles (9 column tiles x ~28 splits): 4.1 MB of partial slabs instead of 9.4 MB
    // for 64 x 192 tiles x 64 splits, and 9.1 vs 9.8 us (profiles/r02b)
    return klaunch(h, K_CONV3_WGRAD, "conv3_wgrad", gemm_wg<T, 64, 64, 2, 2, 32, WG4, Conv3Wgrad<T>>,
                   dim3(K3 / 64, 1, h->sp3.S), dim3(256 * WG4), st, o3, h->s_w3, h->s_b3,
                   h->sp3.mps);
  };

  // ---- c2_c1: conv2 weight gradient (unless wg23 ran it), then conv2 input gradient
  // (ReLU-masked) + conv1 weight gradient fused per frame (unless lc12 ran it) ----
  auto c2_c1 = [&]() -> int {
    if (!wg23) {
      Conv2Wgrad<T> op{};
      op.M = N * P2; op.x = (const T*)h->dact2; op.in = (const T*)h->act1;
      if (int r = klaunch(h, K_CONV2_WGRAD, "conv2_wgrad", gemm_wg<T, 64, 128, 1, 4, 32, WG4, Conv2Wgrad<T>>,
                          dim3(K2 / 128, 1, h->sp2.S), dim3(256 * WG4), st, op, h->s_w2, h->s_b2,
                          h->sp2.mps))
        return r;
    }
    if (lc12) return 0;
    return klaunch(h, K_CONV12_BWD, "conv2_dgrad_conv1_wgrad", conv12_bwd_s2d<T>, dim3(h->c1_wg),
                   dim3(256 * C12_GROUPS), st, b->obs, sw + sh.w2, sw + sh.w2t,
                   (const T*)h->dact2, (const uint32_t*)h->mask1, h->s_w1, h->s_b1, N, h->c1_fpw);
  };

  for (int s = bp->first; s <= bp->last; ++s) {
    int r = 0;
    switch (s) {
      case BS_HEAD_FC: r = head_fc(); break;
      case BS_LN_C3: r = ln_c3(); break;
      case BS_C2_C1: r = c2_c1(); break;
    }
    if (r) return r;
  }
  return reduce_segments<HID>(h, bp->red_lo, bp->red_hi, st, bp->fin);
}

template <typename T, int HID>
int launch_adam(impala_learner* h, hipStream_t st) {
  AdamArgs aa{};
  aa.params = h->params; aa.grads = h->grads; aa.m = h->exp_avg; aa.v = h->exp_avg_sq;
  aa.metrics = h->metrics; aa.sumsq_part = h->sumsq_part; aa.n_part = h->n_red_wg;
  aa.metrics_host = h->metrics_host;
  aa.step = h->step;
  aa.sc = h->adam_sc; aa.b1 = dec(h->cfg.adam_beta1); aa.b2 = dec(h->cfg.adam_beta2);
  aa.eps = h->cfg.adam_eps; aa.max_norm = h->cfg.max_grad_norm;
  aa.inv_world = 1.f / (float)h->cfg.world_size;
  aa.sp = ShadowPtrs{h->shadow, h->vecs, h->A};
  aa.cn = h->cn; aa.sh = h->sh;
  // HID blocks for the FC weight rows, then the other parameters (adam_kernel)
  const long rest = (long)h->cn.total - (long)(h->cn.bfc - h->cn.wfc);
  return klaunch(h, K_ADAM, "adam", adam_kernel<T, HID>, dim3(HID + cdiv(rest, 256)),
                 dim3(256), st, aa);
}

template <typename T, int HID>
int launch_pack(impala_learner* h, hipStream_t st) {
  pack_params_kernel<T, HID><<<cdiv((long)h->cn.total, 256), 256, 0, st>>>(h->params, ShadowPtrs{h->shadow, h->vecs, h->A},
                                                     h->cn, h->sh);
  CK_LAUNCH("pack_params");
  return 0;
}

int check_bound(impala_learner* h, bool train = true) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->params) return fail(IMPALA_E_STATE, "impala_bind_state() not called");
  if (train && (!h->grads || !h->exp_avg || !h->exp_avg_sq || !h->metrics))
    return fail(IMPALA_E_STATE, "training needs grads, exp_avg, exp_avg_sq and metrics bound");
  return 0;
}

int check_batch(const impala_batch* b, bool ppo = false) {
  if (!b || !b->obs || !b->actions || !b->rewards || (!ppo && !b->discounts) ||
      !b->behaviour_logits)
    return fail(IMPALA_E_INVALID, "null batch pointer");
  if (((uintptr_t)b->obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  return 0;
}

}  // namespace

extern "C" {

int impala_abi_version(void) { return IMPALA_ABI_VERSION; }
const char* impala_last_error(void) { return g_err.c_str(); }

int impala_config_default(impala_config* c) {
  if (!c) return fail(IMPALA_E_INVALID, "null cfg");
  c->batch_size = 8;
  c->rollout_length = 20;
  c->num_actions = 15;
  c->dtype = IMPALA_DTYPE_F32;
  c->lr = 1e-4f;
  c->adam_beta1 = 0.9f;
  c->adam_beta2 = 0.999f;
  c->adam_eps = 1e-5f;
  c->max_grad_norm = 0.5f;
  c->entropy_coeff = 0.01f;
  c->vtrace_lambda = 1.f;
  c->clip_rho_threshold = 1.f;
  c->clip_pg_rho_threshold = 1.f;
  c->world_size = 1;
  c->algo = IMPALA_ALGO_IMPALA;
  c->ppo_clip = 0.1f;
  c->vtrace_grad_mode = IMPALA_VTRACE_SG_ADVANTAGE;
  return 0;
}

size_t impala_param_count(int num_actions) { return net::canon(num_actions).total; }

int impala_create(const impala_config* cfg, int device, impala_learner** out) {
  using namespace net;
  if (!cfg || !out) return fail(IMPALA_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->batch_size < 1) return fail(IMPALA_E_INVALID, "batch_size must be >= 1");
  if (cfg->algo != IMPALA_ALGO_IMPALA && cfg->algo != IMPALA_ALGO_PPO)
    return fail(IMPALA_E_INVALID, "unknown algo");
  if (cfg->algo == IMPALA_ALGO_PPO && cfg->rollout_length != 1)
    return fail(IMPALA_E_UNSUPPORTED, "PPO handles take flat transitions: rollout_length must be 1");
  if (cfg->algo == IMPALA_ALGO_IMPALA && (cfg->rollout_length < 2 || cfg->rollout_length > 64))
    return fail(IMPALA_E_UNSUPPORTED, "rollout_length must be in [2, 64]");
  if (!(cfg->ppo_clip >= 0.f && cfg->ppo_clip < 1.f))
    return fail(IMPALA_E_INVALID, "ppo_clip must be in [0, 1)");
  if (cfg->num_actions < 1 || cfg->num_actions > MAX_A)
    return fail(IMPALA_E_UNSUPPORTED, "num_actions must be in [1, 15]");
  if (cfg->vtrace_grad_mode < IMPALA_VTRACE_SG_ADVANTAGE || cfg->vtrace_grad_mode > IMPALA_VTRACE_SG_NONE)
    return fail(IMPALA_E_INVALID, "unknown vtrace_grad_mode");
  if (cfg->dtype != IMPALA_DTYPE_F32 && cfg->dtype != IMPALA_DTYPE_BF16)
    return fail(IMPALA_E_INVALID, "unknown dtype");
  if (cfg->world_size < 1) return fail(IMPALA_E_INVALID, "world_size must be >= 1");
  return impala_internal::create_learner(cfg, device, net::HID_AC, out);
}

extern "C++" {
// The handle behind impala_create, and behind dqn_create (dqn.h) with the 512-wide projection and
// cfg->algo = ALGO_DQN (flat transitions, rollout_length 1).  The configuration is the caller's
// to validate.
int impala_internal::create_learner(const impala_config* cfg, int device, int hid,
                                    impala_learner** out) {
  using namespace net;
  const int HID = hid;
  const bool dqn = cfg->algo == ALGO_DQN;
  CK(hipSetDevice(device));
  impala_learner* h = new (std::nothrow) impala_learner();
  if (!h) return fail(IMPALA_E_INVALID, "out of host memory");
  // ---- every environment read of this function; nothing below depends on the environment ----
  // separate launches of stages the default step fuses (=0): the kernels the host falls back to
  // at large frame runs and in the data-parallel parts, selectable so small tests can run them
  if (const char* e = std::getenv("IMPALA_C3_TAIL")) h->c3_tail = e[0] != '0';
  if (const char* e = std::getenv("IMPALA_LC12")) h->lc12 = e[0] != '0';
  if (const char* e = std::getenv("IMPALA_WG23_MERGED")) h->wg23_merged = e[0] != '0';
  // hipGraph replay of whole steps (opt-in): it cuts the host enqueue cost of a step ~3x, but
  // on MI355X / ROCm 7 the replayed step ran slower on the device than direct launches
  // (174 vs 165 us), so direct launches are the default
  if (const char* g = std::getenv("IMPALA_GRAPH")) h->use_graph = g[0] == '1';
  // workgroup targets of the FC and conv weight-gradient splits (0: the defaults below)
  int fc_wg = 0, wg3 = 256, wg2 = 256;
  if (const char* e = std::getenv("IMPALA_FC_WG")) fc_wg = std::max(16, std::atoi(e));
  if (const char* e = std::getenv("IMPALA_WG3_TARGET")) wg3 = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("IMPALA_WG2_TARGET")) wg2 = std::max(1, std::atoi(e));
  // frames per workgroup: conv2 dgrad + conv1 wgrad, conv1 + conv2 forward (0: N / CUs)
  int c1_fpw = 0;
  if (const char* e = std::getenv("IMPALA_C1_FPW")) c1_fpw = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("IMPALA_C12F_FPW")) h->c12f_fpw = std::max(0, std::atoi(e));
  // split loads per thread the slab reduction's split-group count aims for
  int lpt = 16;
  if (const char* e = std::getenv("IMPALA_RED_LPT")) lpt = std::max(1, std::atoi(e));

  h->cfg = *cfg;
  h->device = device;
  h->A = cfg->num_actions;
  h->bf16 = cfg->dtype == IMPALA_DTYPE_BF16;
  h->N = cfg->batch_size * cfg->rollout_length;
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        cu > 0)
      h->n_cu = cu;
  }
  h->hid = hid;
  h->cn = hid == HID_DQN ? canon_dqn(h->A) : canon(h->A);
  h->sh = hid == HID_DQN ? shadow_dqn() : shadow();
  const int N = h->N;
  const size_t es = h->bf16 ? 2 : 4;
  h->S_seg = next_pow2(cfg->rollout_length);
  h->n_loss_wg = cdiv(cfg->batch_size, 64 / h->S_seg);  // fused head: 64/S trajectories per WG
  if (dqn) h->n_loss_wg = cdiv(N, DQN_F);               // dueling head: DQN_F transitions per WG
  // frames per workgroup of the LayerNorm backward + conv3 dgrad kernels (one slab each)
  h->ln_fpw = std::max(1, cdiv(N, h->n_cu));
  h->n_ln_wg = cdiv(N, h->ln_fpw);

  // upper bound on the reduce workgroups (each segment: count/4 float4 columns, >= 16 per WG)
  h->n_red_wg = 11 + (OC1 * K1 + OC1 + OC2 * K2 + OC2 + OC3 * K3 + OC3 + 2 * FLAT + HID * FLAT +
                      HID + HEADS * HID + HEADS) / 4 / 16;
  h->sph.S = h->n_loss_wg;  // heads weight-gradient partials: one slab per head workgroup
  // FC weight-gradient splits: 96 workgroups for bf16; fp32 128 (8 splits: fc_bwd 20.3 us and
  // the reduction 7.55 against 20.7 / 7.75 for 256 workgroups, 27.8 us for 64;
  // tools/var_specs/{fc32b,spfc32}.py)
  if (fc_wg == 0) fc_wg = h->bf16 ? 96 : 128;
  h->spfc = plan_split(N, (FLAT / 256) * (HID / 64), fc_wg);
  // the conv weight gradients' m splits: ~256 workgroups each (IMPALA_WG3_TARGET /
  // IMPALA_WG2_TARGET override the count for A/B runs; more splits, more slab bytes to reduce)
  h->sp3 = plan_split((long)N * P3, K3 / 64, wg3);
  h->sp2 = plan_split((long)N * P2, K2 / 128, wg2);
  h->c1_fpw = c1_fpw > 0 ? c1_fpw : std::max(1, cdiv(N, h->n_cu));
  h->c1_wg = cdiv(N, h->c1_fpw);
  h->sp1.S = h->c1_wg;  // slab splits of conv1 (one per workgroup)

  // ---- one workspace allocation, 256-byte aligned carve (arena.h: sized on a null base) ----
  auto carve = [&](Arena a) {
    auto F = [&](size_t bytes) { return (float*)a.take(bytes); };
    h->shadow = a.take(h->sh.total * es);
    h->vecs = F((hid == HID_DQN ? VecsDqn::total : Vecs::total) * 4);
    h->act1 = a.take((size_t)N * P1 * OC1 * es);
    h->act2 = a.take((size_t)N * P2 * OC2 * es);
    h->act3 = a.take((size_t)N * FLAT * es);
    h->y = a.take((size_t)N * YLD * es);
    h->h = a.take((size_t)N * HID * es);
    h->dz = a.take((size_t)N * HID * es);
    h->dact3 = a.take((size_t)N * FLAT * es);
    h->dact2 = a.take((size_t)N * P2 * OC2 * es);
    h->mask1 = (uint32_t*)a.take((size_t)N * P1 * 4);
    h->lnstat = F((size_t)N * 2 * 4);
    h->zg = F((size_t)N * HID * 4);
    h->heads = F((size_t)N * HEADS * 4);
    h->dy = F((size_t)N * FLAT * 4);
    h->s_w1 = F((size_t)h->sp1.S * OC1 * K1 * 4);
    h->s_b1 = F((size_t)h->sp1.S * OC1 * 4);
    h->s_w2 = F((size_t)h->sp2.S * OC2 * K2 * 4);
    h->s_b2 = F((size_t)h->sp2.S * OC2 * 4);
    h->s_w3 = F((size_t)h->sp3.S * OC3 * K3 * 4);
    h->s_b3 = F((size_t)h->sp3.S * OC3 * 4);
    h->s_ln = F((size_t)h->n_ln_wg * 2 * FLAT * 4);
    h->s_fc = F((size_t)h->spfc.S * HID * FLAT * 4);
    h->s_bfc = F((size_t)h->spfc.S * HID * 4);
    h->s_h = F((size_t)h->sph.S * HEADS * HID * 4);
    h->s_bh = F((size_t)h->sph.S * HEADS * 4);
    h->loss_part = F((size_t)h->n_loss_wg * 8 * 4);
    h->sumsq_part = F((size_t)(h->n_red_wg + 3) / 4 * 16);  // zero tail: float4 reads
    h->adam_sc = F(2 * 4);
    h->step = (int64_t*)a.take(8);
    return Arena::align(a.used);
  };
  h->ws_bytes = carve(Arena{});
  hipError_t e = hipMalloc(&h->ws, h->ws_bytes);
  if (e != hipSuccess) {
    delete h;
    return fail((int)e, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
  }
  e = hipMemset(h->ws, 0, h->ws_bytes);
  if (e != hipSuccess) {
    (void)hipFree(h->ws);
    delete h;
    return fail((int)e, std::string("hipMemset workspace: ") + hipGetErrorString(e));
  }
  carve(Arena{h->ws});
  // the capture stream exists only for graph replay: every stream a process creates takes a
  // share of its GPU_MAX_HW_QUEUES hardware queues (profiles/r06w)
  if (h->use_graph && hipStreamCreateWithFlags(&h->graphs.cap, hipStreamNonBlocking) != hipSuccess) {
    impala_destroy(h);
    return fail(IMPALA_E_STATE, "hipStreamCreate (capture stream) failed");
  }
  {
    RedArgs& ra = h->red;
    int ns = 0;
    // split loads per thread the split-group count aims for (lpt, IMPALA_RED_LPT): 16 -> 10.3 us,
    // 8 -> 10.7, 4 -> 11.2, 2 -> 11.6 (rocprof, B=64 T=20 bf16, profiles/r01k)
    auto add = [&](const float* slab, int S, int count, int kind, long long canon) {
      int sg = 1;
      while (sg < 16 && sg * lpt < S) sg <<= 1;  // ~lpt+ loads per thread, <= 16 groups
      ra.seg[ns] = RedSeg{slab, S, count, kind, canon, sg};
      ra.wg_start[ns + 1] = ra.wg_start[ns] + cdiv(count / 4, 256 / sg);
      ++ns;
    };
    ra.wg_start[0] = 0;
    add(h->s_w1, h->sp1.S, OC1 * K1, RK_CONV1, (long long)h->cn.w1);
    add(h->s_b1, h->sp1.S, OC1, RK_ID, (long long)h->cn.b1);
    add(h->s_w2, h->sp2.S, OC2 * K2, RK_CONV2, (long long)h->cn.w2);
    add(h->s_b2, h->sp2.S, OC2, RK_ID, (long long)h->cn.b2);
    add(h->s_w3, h->sp3.S, OC3 * K3, RK_CONV3, (long long)h->cn.w3);
    add(h->s_b3, h->sp3.S, OC3, RK_ID, (long long)h->cn.b3);
    add(h->s_ln, h->n_ln_wg, 2 * FLAT, RK_LN, (long long)h->cn.lng);
    add(h->s_fc, h->spfc.S, HID * FLAT, RK_FC, (long long)h->cn.wfc);
    add(h->s_bfc, h->spfc.S, HID, RK_ID, (long long)h->cn.bfc);
    add(h->s_h, h->sph.S, HEADS * HID, RK_HEADS_W, 0);
    add(h->s_bh, h->sph.S, HEADS, RK_HEADS_B, 0);
    h->n_red_wg = ra.wg_start[ns];
    if (ns != RS_END) {
      impala_destroy(h);
      return fail(IMPALA_E_STATE, "reduce segment table out of sync");
    }
    ra.cn = h->cn;
    ra.sumsq_part = h->sumsq_part;
    ra.loss_part = h->loss_part;
    ra.n_loss_part = h->n_loss_wg;
    ra.B = cfg->batch_size;
    ra.T = cfg->rollout_length;
    ra.A = h->A;
    ra.ent_coef = cfg->entropy_coeff;
    ra.algo = cfg->algo;
    ra.step = h->step;
    ra.lr = dec(cfg->lr); ra.b1 = dec(cfg->adam_beta1); ra.b2 = dec(cfg->adam_beta2);
    ra.adam_sc = h->adam_sc;
  }
  *out = h;
  return 0;
}
}  // extern "C++"

extern "C++" {
namespace {
// RCCL entry points, resolved by dlopen on first use: the library has no link-time RCCL
// dependency, and inside a torch process the loader hands back torch's already-loaded copy
// (same SONAME), so the handle's communicator and torch's live in one RCCL instance.
struct RcclApi {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  decltype(&ncclCommCount) comm_count = nullptr;
  std::string err;
};
const RcclApi& rccl() {
  static const RcclApi api = [] {
    RcclApi a;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW);
    if (!lib) {
      const char* e = dlerror();
      a.err = std::string("dlopen librccl: ") + (e ? e : "not found");
      return a;
    }
    a.get_unique_id = (decltype(a.get_unique_id))dlsym(lib, "ncclGetUniqueId");
    a.comm_init_rank = (decltype(a.comm_init_rank))dlsym(lib, "ncclCommInitRank");
    a.all_reduce = (decltype(a.all_reduce))dlsym(lib, "ncclAllReduce");
    a.comm_destroy = (decltype(a.comm_destroy))dlsym(lib, "ncclCommDestroy");
    a.error_string = (decltype(a.error_string))dlsym(lib, "ncclGetErrorString");
    a.comm_count = (decltype(a.comm_count))dlsym(lib, "ncclCommCount");
    if (!a.get_unique_id || !a.comm_init_rank || !a.all_reduce || !a.comm_destroy ||
        !a.error_string || !a.comm_count)
      a.err = "librccl lacks an expected entry point";
    return a;
  }();
  return api;
}
int rccl_fail(const char* what, ncclResult_t r) {
  return fail(IMPALA_E_RCCL, std::string(what) + ": " + rccl().error_string(r));
}
void dp_release(impala_learner* h) {
  if (h->dp_comm) (void)rccl().comm_destroy(h->dp_comm);
  h->dp_comm = nullptr;
  if (h->dp_stream) (void)hipStreamDestroy(h->dp_stream);
  h->dp_stream = nullptr;
  for (auto& e : h->dp_ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  h->dp_nranks = 0;
  h->dp_rank = -1;
}
}  // namespace
}  // extern "C++"

int impala_destroy(impala_learner* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();  // replays may still be in flight on the caller's streams
  h->graphs.drop();
  stage_destroy(h->stage);
  for (auto& t : h->timers) {
    for (int i = 0; i < 2 * t.cap; ++i) (void)hipEventDestroy(t.ev[i]);
    delete[] t.ev;
  }
  if (h->graphs.cap) (void)hipStreamDestroy(h->graphs.cap);
  dp_release(h);
  if (h->ws) (void)hipFree(h->ws);
  delete h;
  return 0;
}

int impala_bind_state(impala_learner* h, float* params, float* grads, float* exp_avg,
                      float* exp_avg_sq, float* metrics, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!params) return fail(IMPALA_E_INVALID, "null params pointer");
  h->params = params; h->grads = grads; h->exp_avg = exp_avg; h->exp_avg_sq = exp_avg_sq;
  h->metrics = metrics;
  h->graphs.drop();  // captured launches hold the previous state pointers
  h->red.grads = grads;
  h->red.metrics = metrics;
  return impala_refresh_weights(h, stream);
}

int impala_set_metrics(impala_learner* h, float* metrics) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!metrics) return fail(IMPALA_E_INVALID, "null metrics pointer");
  if (h->metrics != metrics) {
    h->metrics = metrics;
    h->red.metrics = metrics;
    if (h->use_graph) h->graphs.drop();  // captured launches hold the previous pointer
  }
  return 0;
}

int impala_set_metrics_host(impala_learner* h, float* host) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (host) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, host) != hipSuccess || at.type != hipMemoryTypeHost) {
      (void)hipGetLastError();
      return fail(IMPALA_E_INVALID, "impala_set_metrics_host: not page-locked host memory");
    }
    if (((uintptr_t)host & 3) != 0) return fail(IMPALA_E_INVALID, "impala_set_metrics_host: misaligned");
  }
  if (h->metrics_host != host) {
    h->metrics_host = host;
    if (h->use_graph) h->graphs.drop();  // captured launches hold the previous pointer
  }
  return 0;
}

int impala_set_debug_vtrace(impala_learner* h, float* out) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (h->vt_dbg != out) h->graphs.drop();  // captured launches hold the previous pointer
  h->vt_dbg = out;
  return 0;
}

int impala_debug_read(impala_learner* h, int which, void* dst, size_t bytes, void* stream) {
  using namespace net;
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!dst) return fail(IMPALA_E_INVALID, "null destination");
  const size_t N = (size_t)h->N, es = h->bf16 ? 2 : 4, hid = (size_t)h->hid;
  const void* src = nullptr;
  size_t size = 0;
  switch (which) {  // the sizes of the workspace carve-up in create_learner
    case IMPALA_DBG_ACT1: src = h->act1; size = N * P1 * OC1 * es; break;
    case IMPALA_DBG_ACT2: src = h->act2; size = N * P2 * OC2 * es; break;
    case IMPALA_DBG_ACT3: src = h->act3; size = N * FLAT * es; break;
    case IMPALA_DBG_Y: src = h->y; size = N * FLAT * es; break;  // (dense: the row pitch is dropped)
    case IMPALA_DBG_H: src = h->h; size = N * hid * es; break;
    case IMPALA_DBG_DZ: src = h->dz; size = N * hid * es; break;
    case IMPALA_DBG_DACT3: src = h->dact3; size = N * FLAT * es; break;
    case IMPALA_DBG_DACT2: src = h->dact2; size = N * P2 * OC2 * es; break;
    case IMPALA_DBG_MASK1: src = h->mask1; size = N * P1 * 4; break;
    case IMPALA_DBG_LNSTAT: src = h->lnstat; size = N * 2 * 4; break;
    case IMPALA_DBG_ZG: src = h->zg; size = N * hid * 4; break;
    case IMPALA_DBG_HEADS: src = h->heads; size = N * HEADS * 4; break;
    case IMPALA_DBG_DY: src = h->dy; size = N * FLAT * 4; break;
    default: return fail(IMPALA_E_INVALID, "unknown debug tensor");
  }
  if (bytes == 0 || bytes > size) return fail(IMPALA_E_INVALID, "bytes must be in (0, the tensor's size]");
  CK(hipSetDevice(h->device));
  if (which == IMPALA_DBG_Y && YLD != FLAT) {  // rows of FLAT elements at a pitch of YLD
    const size_t row = FLAT * es;
    if (bytes % row) return fail(IMPALA_E_INVALID, "y is read in whole rows");
    CK(hipMemcpy2DAsync(dst, row, src, YLD * es, row, bytes / row, hipMemcpyDefault, (hipStream_t)stream));
    return 0;
  }
  CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

int impala_refresh_weights(impala_learner* h, void* stream) {
  if (int r = check_bound(h, false)) return r;
  CK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  return BY_NET(h, launch_pack, h, st);
}

int impala_set_step(impala_learner* h, int64_t step, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (step < 0) return fail(IMPALA_E_INVALID, "negative step");
  CK(hipSetDevice(h->device));
  static thread_local int64_t host_step;
  host_step = step;
  CK(hipMemcpyAsync(h->step, &host_step, 8, hipMemcpyHostToDevice, (hipStream_t)stream));
  CK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int impala_forward(impala_learner* h, const uint8_t* obs, int n, float* logits, float* values,
                   void* stream) {
  if (int r = check_bound(h, false)) return r;
  if (!obs || !logits || !values) return fail(IMPALA_E_INVALID, "null pointer");
  if (n < 1 || n > h->N) return fail(IMPALA_E_INVALID, "n must be in [1, B*T]");
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  CK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  int r = BY_NET(h, launch_forward, h, obs, n, st, true);
  if (r) return r;
  split_heads_kernel<<<cdiv((long)n * net::HEADS, 256), 256, 0, st>>>(h->heads, n, h->A, logits,
                                                                       values);
  CK_LAUNCH("split_heads");
  return 0;
}

int impala_act(impala_learner* h, const uint8_t* obs, int n, const uint8_t* deterministic,
               int deterministic_all, uint64_t seed, uint64_t counter, int64_t* actions,
               float* logits, float* values, void* stream) {
  if (int r = check_bound(h, false)) return r;
  if (!obs || !actions || !logits || !values) return fail(IMPALA_E_INVALID, "null pointer");
  if (n < 1 || n > h->N) return fail(IMPALA_E_INVALID, "n must be in [1, B*T]");
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  CK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  int r = BY_NET(h, launch_forward, h, obs, n, st, true);
  if (r) return r;
  act_heads_kernel<<<cdiv(n, 256), 256, 0, st>>>(h->heads, n, h->A, deterministic,
                                                 deterministic_all, seed, counter, actions,
                                                 logits, values);
  CK_LAUNCH("act_heads");
  return 0;
}

extern "C++" {
namespace {
int enqueue_grads(impala_learner* h, const impala_batch* b, hipStream_t st, int part = -1) {
  const BwdPart* bp = bwd_part(part);
  if (!bp) return fail(IMPALA_E_INVALID, "unknown backward part");
  if (bp->first == BS_HEAD_FC) {  // (the other parts continue a backward)
    int r = BY_NET(h, launch_forward, h, b->obs, h->N, st, false);
    if (r) return r;
  }
  return BY_NET(h, launch_backward, h, b, st, bp);
}

int enqueue_update(impala_learner* h, hipStream_t st) {
  if (h->cfg.world_size > 1) {
    if (int r = klaunch(h, K_SUMSQ, "sumsq", sumsq_kernel, dim3(h->n_red_wg), dim3(256), st,
                        (const float*)h->grads, (size_t)h->cn.total, h->sumsq_part))
      return r;
  }
  return BY_NET(h, launch_adam, h, st);
}

// A step's launches through the handle's graph cache (GraphCache::run, host.h).  With the live
// timer armed (its events must be recorded per launch), the step clock armed or IMPALA_GRAPH=0 the
// launches go straight to `st`.
template <class Body>
int run_graphed(impala_learner* h, int kind, const impala_batch* b, hipStream_t st, Body&& body) {
  const bool bypass = !h->use_graph || h->timers_armed > 0 || h->clock_buf;
  return h->graphs.run(!bypass, kind, b ? *b : impala_batch{}, st, body);
}
enum { G_GRADS = 0, G_UPDATE = 1, G_STEP = 2, G_GRADS0 = 3 };  // G_GRADS0 + part (0..4, 6)
}  // namespace
}  // extern "C++"

int impala_compute_grads(impala_learner* h, const impala_batch* b, void* stream) {
  if (int r = check_bound(h)) return r;
  if (int r = check_batch(b, h->cfg.algo == IMPALA_ALGO_PPO)) return r;
  CK(hipSetDevice(h->device));
  return run_graphed(h, G_GRADS, b, (hipStream_t)stream,
                     [&](hipStream_t s) { return enqueue_grads(h, b, s); });
}

int impala_compute_grads_part(impala_learner* h, const impala_batch* b, int part, void* stream) {
  if (part < 0 || part > 6 || part == 5) return fail(IMPALA_E_INVALID, "part must be 0..4 or 6");
  if (int r = check_bound(h)) return r;
  if (int r = check_batch(b, h->cfg.algo == IMPALA_ALGO_PPO)) return r;
  CK(hipSetDevice(h->device));
  return run_graphed(h, G_GRADS0 + part, b, (hipStream_t)stream,
                     [&](hipStream_t s) { return enqueue_grads(h, b, s, part); });
}

size_t impala_grad_bucket_offset(const impala_learner* h) { return h ? h->cn.w3 : 0; }
size_t impala_grad_bucket_offset_fc(const impala_learner* h) { return h ? h->cn.wfc : 0; }

int impala_apply_update(impala_learner* h, void* stream) {
  if (int r = check_bound(h)) return r;
  CK(hipSetDevice(h->device));
  return run_graphed(h, G_UPDATE, nullptr, (hipStream_t)stream,
                     [&](hipStream_t s) { return enqueue_update(h, s); });
}

int impala_dp_unique_id(void* out) {
  if (!out) return fail(IMPALA_E_INVALID, "null unique-id buffer");
  const RcclApi& api = rccl();
  if (!api.err.empty()) return fail(IMPALA_E_RCCL, api.err);
  ncclUniqueId id;
  if (ncclResult_t r = api.get_unique_id(&id)) return rccl_fail("ncclGetUniqueId", r);
  static_assert(sizeof(ncclUniqueId) == IMPALA_DP_ID_BYTES, "unique id size");
  std::memcpy(out, &id, sizeof(id));
  return 0;
}

int impala_dp_init(impala_learner* h, const void* unique_id, int nranks, int rank) {
  if (!h || !unique_id) return fail(IMPALA_E_INVALID, "null argument");
  if (nranks != h->cfg.world_size || rank < 0 || rank >= nranks)
    return fail(IMPALA_E_INVALID, "nranks must equal the handle's world_size and 0 <= rank < nranks");
  const RcclApi& api = rccl();
  if (!api.err.empty()) return fail(IMPALA_E_RCCL, api.err);
  CK(hipSetDevice(h->device));
  dp_release(h);
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof(id));
  // collective over the nranks processes (each blocks until all have joined)
  if (ncclResult_t r = api.comm_init_rank(&h->dp_comm, nranks, id, rank)) {
    h->dp_comm = nullptr;
    return rccl_fail("ncclCommInitRank", r);
  }
  // the rest cannot leave a half-initialised handle: any failure releases the communicator
  // (impala_dp_train_step then reports that impala_dp_init has not run)
  hipError_t e = hipStreamCreateWithFlags(&h->dp_stream, hipStreamNonBlocking);
  for (auto& ev : h->dp_ev)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    dp_release(h);
    return fail((int)e, std::string("impala_dp_init: ") + hipGetErrorString(e));
  }
  int count = 0;
  if (ncclResult_t r = api.comm_count(h->dp_comm, &count)) {
    dp_release(h);
    return rccl_fail("ncclCommCount", r);
  }
  if (count != nranks) {
    dp_release(h);
    return fail(IMPALA_E_RCCL, "ncclCommCount disagrees with nranks");
  }
  h->dp_nranks = count;
  h->dp_rank = rank;
  return 0;
}

int impala_dp_nranks(const impala_learner* h, int* nranks) {
  if (!h || !nranks) return fail(IMPALA_E_INVALID, "null argument");
  *nranks = 0;
  if (!h->dp_comm) return 0;
  const RcclApi& api = rccl();
  if (!api.err.empty()) return fail(IMPALA_E_RCCL, api.err);
  if (ncclResult_t r = api.comm_count(h->dp_comm, nranks)) return rccl_fail("ncclCommCount", r);
  return 0;
}

int impala_dp_train_step(impala_learner* h, const impala_batch* b, int buckets, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->dp_comm || !h->dp_stream || !h->dp_ev[2])
    return fail(IMPALA_E_STATE, "impala_dp_init has not run on this handle");
  if (buckets != 1 && buckets != 2) return fail(IMPALA_E_INVALID, "buckets must be 1 or 2");
  if (int r = check_bound(h)) return r;
  if (int r = check_batch(b, h->cfg.algo == IMPALA_ALGO_PPO)) return r;
  CK(hipSetDevice(h->device));
  const hipStream_t st = (hipStream_t)stream;
  const RcclApi& api = rccl();
  float* g = h->grads;
  const size_t n = (size_t)h->cn.total, off_fc = (size_t)h->cn.wfc;
  if (buckets == 1) {  // the whole backward, one all-reduce on the compute stream, the update
    if (int r = enqueue_grads(h, b, st)) return r;
    if (ncclResult_t r = api.all_reduce(g, g, n, ncclFloat32, ncclSum, h->dp_comm, st))
      return rccl_fail("ncclAllReduce", r);
    return enqueue_update(h, st);
  }
  // two buckets: part 2 (forward, heads step, FC gradients) leaves grads[off_fc ..] final; its
  // all-reduce runs on dp_stream while part 6 (the per-frame backward, the conv weight
  // gradients) runs on `st`; then grads[.. off_fc] follow on dp_stream and `st` waits for both
  if (int r = enqueue_grads(h, b, st, 2)) return r;
  CK(hipEventRecord(h->dp_ev[0], st));
  CK(hipStreamWaitEvent(h->dp_stream, h->dp_ev[0], 0));
  if (ncclResult_t r = api.all_reduce(g + off_fc, g + off_fc, n - off_fc, ncclFloat32, ncclSum,
                                      h->dp_comm, h->dp_stream))
    return rccl_fail("ncclAllReduce (FC + heads bucket)", r);
  if (int r = enqueue_grads(h, b, st, 6)) return r;
  CK(hipEventRecord(h->dp_ev[1], st));
  CK(hipStreamWaitEvent(h->dp_stream, h->dp_ev[1], 0));
  if (ncclResult_t r = api.all_reduce(g, g, off_fc, ncclFloat32, ncclSum, h->dp_comm, h->dp_stream))
    return rccl_fail("ncclAllReduce (conv + LayerNorm bucket)", r);
  CK(hipEventRecord(h->dp_ev[2], h->dp_stream));
  CK(hipStreamWaitEvent(st, h->dp_ev[2], 0));
  return enqueue_update(h, st);
}

int impala_ppo_train_step(impala_learner* h, const impala_ppo_batch* pb, void* stream) {
  if (!h || !pb) return fail(IMPALA_E_INVALID, "null argument");
  if (h->cfg.algo != IMPALA_ALGO_PPO) return fail(IMPALA_E_STATE, "not a PPO handle");
  const impala_batch b{pb->obs, pb->actions, pb->targets, nullptr, pb->behaviour_logits};
  return impala_train_step(h, &b, stream);
}

int impala_train_step(impala_learner* h, const impala_batch* b, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (h->cfg.world_size != 1)
    return fail(IMPALA_E_STATE, "world_size > 1: use compute_grads + all-reduce + apply_update");
  if (int r = check_bound(h)) return r;
  if (int r = check_batch(b, h->cfg.algo == IMPALA_ALGO_PPO)) return r;
  CK(hipSetDevice(h->device));
  return run_graphed(h, G_STEP, b, (hipStream_t)stream, [&](hipStream_t s) {
    if (int r = enqueue_grads(h, b, s)) return r;
    return enqueue_update(h, s);
  });
}

namespace {
// impala_train_step_rows / impala_ppo_train_step_rows: the step on n ring slots read in place.
// What needs no handle is refused first (null pointers, n, the row range), then what the handle
// cannot run (IMPALA_E_UNSUPPORTED), then the sizes that depend on it.
int step_rows(impala_learner* h, const impala_batch* ring, const int64_t* rows, int n, int64_t capacity,
              void* stream, int algo, const char* entry) {
  const std::string who = std::string(entry) + ": ";
  if (!ring || !rows) return fail(IMPALA_E_INVALID, who + "null argument");
  if (n < 1 || n > kObsRowsMax)
    return fail(IMPALA_E_INVALID, who + "n must equal batch_size (at most 256)");
  if (capacity < 1) return fail(IMPALA_E_INVALID, who + "bad capacity");
  for (int i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= capacity)
      return fail(IMPALA_E_INVALID, who + "row index out of range");
  if (!h) return fail(IMPALA_E_INVALID, who + "null handle");
  const bool ppo = algo == IMPALA_ALGO_PPO;
  if (h->cfg.world_size != 1 || h->cfg.algo != algo)
    return fail(IMPALA_E_UNSUPPORTED, who + (ppo ? "PPO" : "IMPALA") + " handles of world_size 1");
  // only the default launches read the batch through the row map: the fused forward
  // (conv12_fwd_s2d), the fused head and the fused per-frame backward (lnc3_conv12_bwd)
  const bool default_path = h->lc12 && h->ln_fpw == h->c1_fpw;
  if (!default_path) return fail(IMPALA_E_UNSUPPORTED, who + "not on the default kernel path");
  if (n != h->cfg.batch_size)
    return fail(IMPALA_E_INVALID, who + "n must equal batch_size (at most 256)");
  if (capacity > INT32_MAX / h->cfg.rollout_length) return fail(IMPALA_E_INVALID, who + "bad capacity");
  if (int r = check_bound(h)) return r;
  if (int r = check_batch(ring, ppo)) return r;
  CK(hipSetDevice(h->device));
  h->obs_rows.T = h->cfg.rollout_length;  // (1 on PPO handles: flat transitions)
  for (int i = 0; i < n; ++i) h->obs_rows.rows[i] = (int)rows[i];
  h->rows_on = true;
  // direct launches: the rows change every step, a captured graph would hold the first ones
  int r = enqueue_grads(h, ring, (hipStream_t)stream);
  if (r == 0) r = enqueue_update(h, (hipStream_t)stream);
  h->rows_on = false;
  return r;
}
}  // namespace

int impala_train_step_rows(impala_learner* h, const impala_batch* ring, const int64_t* rows, int n,
                           int64_t capacity, void* stream) {
  return step_rows(h, ring, rows, n, capacity, stream, IMPALA_ALGO_IMPALA, "impala_train_step_rows");
}

int impala_ppo_train_step_rows(impala_learner* h, const impala_ppo_batch* ring, const int64_t* rows, int n,
                               int64_t capacity, void* stream) {
  if (!ring) return fail(IMPALA_E_INVALID, "impala_ppo_train_step_rows: null argument");
  const impala_batch b{ring->obs, ring->actions, ring->targets, nullptr, ring->behaviour_logits};
  return step_rows(h, &b, rows, n, capacity, stream, IMPALA_ALGO_PPO, "impala_ppo_train_step_rows");
}

int impala_ppo_extend_rollout(const impala_ppo_ring* ring, int64_t cursor, const uint8_t* obs,
                              const int64_t* actions, const float* rewards, const uint8_t* done,
                              const float* logits, const float* values, int64_t L, float gamma,
                              float lambda, void* stream) {
  const char* who = "impala_ppo_extend_rollout: ";
  if (!ring || !ring->obs || !ring->actions || !ring->targets || !ring->behaviour_logits || !obs ||
      !actions || !rewards || !done || !logits || !values)
    return fail(IMPALA_E_INVALID, std::string(who) + "null pointer");
  if (L < 2 || L > ppo_replay_dev::kMaxRollout)
    return fail(IMPALA_E_INVALID, std::string(who) + "L must be in [2, 1025]");
  if (!(gamma >= 0.f && gamma <= 1.f) || !(lambda >= 0.f && lambda <= 1.f))
    return fail(IMPALA_E_INVALID, std::string(who) + "gamma and lambda must be in [0, 1]");
  if (ring->num_actions < 1 || ring->num_actions > net::MAX_A)
    return fail(IMPALA_E_INVALID, std::string(who) + "num_actions must be in [1, 15]");
  const int64_t K = L - 1, cap = ring->capacity;
  if (cap < 1 || K > cap)
    return fail(IMPALA_E_INVALID, std::string(who) + "K = L - 1 transitions exceed the capacity");
  if (cursor < 0 || cursor >= cap) return fail(IMPALA_E_INVALID, std::string(who) + "cursor out of range");
  hipStream_t st = (hipStream_t)stream;
  // the obs rows: the ring wraps at most once, so one or two copies
  constexpr size_t kRow = 3 * 64 * 64;
  const int64_t first = std::min(K, cap - cursor);
  CK(hipMemcpyAsync(ring->obs + (size_t)cursor * kRow, obs, (size_t)first * kRow, hipMemcpyDeviceToDevice, st));
  if (first < K)
    CK(hipMemcpyAsync(ring->obs, obs + (size_t)first * kRow, (size_t)(K - first) * kRow,
                      hipMemcpyDeviceToDevice, st));
  hipError_t e = ppo_replay_dev::launch_rollout(actions, rewards, done, logits, values, L, ring->num_actions,
                                                gamma, lambda, cursor, cap, ring->actions, ring->targets,
                                                ring->behaviour_logits, st);
  if (e != hipSuccess) return fail((int)e, std::string("launch ppo_rollout: ") + hipGetErrorString(e));
  return 0;
}

namespace {
int gather_launch(const void* const* src, void* const* dst, const size_t* row_bytes, int nfields,
                  const int64_t* idx, const int64_t* host_idx, int n, void* stream) {
  if (nfields < 1 || nfields > 8 || n < 0 || !src || !dst || !row_bytes ||
      (n > 0 && !idx && !host_idx))
    return fail(IMPALA_E_INVALID, "bad gather arguments");
  if (n == 0) return 0;
  GatherArgs ga{};
  int units = 0;
  for (int f = 0; f < nfields; ++f) {
    if (!src[f] || !dst[f] || row_bytes[f] % 4 != 0 || row_bytes[f] == 0)
      return fail(IMPALA_E_INVALID, "gather: null field or row size not a positive multiple of 4");
    ga.src[f] = (const char*)src[f];
    ga.dst[f] = (char*)dst[f];
    ga.row_bytes[f] = (long long)row_bytes[f];
    ga.pieces[f] = (int)((row_bytes[f] + GATHER_PIECE - 1) / GATHER_PIECE);
    ga.unit0[f] = units;
    units += ga.pieces[f] * n;
  }
  ga.unit0[nfields] = units;
  ga.nfields = nfields;
  ga.idx = idx;
  ga.n = n;
  if (!idx)
    for (int i = 0; i < n; ++i) ga.hidx[i] = (int)host_idx[i];
  gather_rows_kernel<<<dim3(units), 256, 0, (hipStream_t)stream>>>(ga);
  CK_LAUNCH("gather_rows");
  return 0;
}
}  // namespace

int impala_gather_rows(const void* const* src, void* const* dst, const size_t* row_bytes,
                       int nfields, const int64_t* idx, int n, void* stream) {
  if (n > 0 && !idx) return fail(IMPALA_E_INVALID, "bad gather arguments");
  return gather_launch(src, dst, row_bytes, nfields, idx, nullptr, n, stream);
}

int impala_gather_rows_hidx(const void* const* src, void* const* dst, const size_t* row_bytes,
                            int nfields, const int64_t* host_idx, int n, void* stream) {
  if (n > 0 && !host_idx) return fail(IMPALA_E_INVALID, "bad gather arguments");
  for (int i = 0; i < n; ++i)
    if (host_idx[i] < 0 || host_idx[i] > INT32_MAX)
      return fail(IMPALA_E_INVALID, "gather: host index out of range");
  // GATHER_HIDX rows per launch, their indices in the launch's arguments
  for (int i0 = 0; i0 < n; i0 += GATHER_HIDX) {
    const int m = std::min(GATHER_HIDX, n - i0);
    void* d[8];
    for (int f = 0; f < nfields && f < 8; ++f)
      d[f] = dst && dst[f] ? (char*)dst[f] + (size_t)i0 * row_bytes[f] : nullptr;
    if (int r = gather_launch(src, dst ? d : nullptr, row_bytes, nfields, nullptr, host_idx + i0, m,
                              stream))
      return r;
  }
  return 0;
}

int impala_stage_init(impala_learner* h, int nslots) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (nslots < 1 || nslots > StageRing::kMaxSlots)
    return fail(IMPALA_E_INVALID, "nslots must be in [1, 8]");
  return stage_init(h->stage, h->device, h->cfg, nslots);
}

int impala_stage(impala_learner* h, const impala_batch* b, int slot) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (slot < 0 || slot >= h->stage.n_slots)
    return fail(IMPALA_E_INVALID, "slot out of range (impala_stage_init not called?)");
  if (int r = wait_staged(h->stage, -1)) return r;  // one staging at a time per handle
  return stage_now(h->stage, b, slot);
}

namespace {
int check_rows(impala_learner* h, const impala_rows* rows, int n, int slot) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (slot < 0 || slot >= h->stage.n_slots)
    return fail(IMPALA_E_INVALID, "slot out of range (impala_stage_init not called?)");
  const bool ppo = h->cfg.algo == IMPALA_ALGO_PPO;
  if (!rows || n != h->cfg.batch_size)
    return fail(IMPALA_E_INVALID, "impala_stage_rows: n must equal the handle's batch_size");
  if (!rows->obs || !rows->actions || !rows->rewards || (!ppo && !rows->discounts) ||
      !rows->behaviour_logits)
    return fail(IMPALA_E_INVALID, "impala_stage_rows: null row array");
  for (int b = 0; b < n; ++b)
    if (!rows->obs[b] || !rows->actions[b] || !rows->rewards[b] ||
        (!ppo && !rows->discounts[b]) || !rows->behaviour_logits[b])
      return fail(IMPALA_E_INVALID, "impala_stage_rows: null row pointer");
  return 0;
}
}  // namespace

int impala_stage_rows(impala_learner* h, const impala_rows* rows, int n, int slot) {
  if (int r = check_rows(h, rows, n, slot)) return r;
  if (int r = wait_staged(h->stage, -1)) return r;  // one staging at a time per handle
  return stage_rows_now(h->stage, rows, n, slot);
}

int impala_stage_rows_async(impala_learner* h, const impala_rows* rows, int n, int slot) {
  if (int r = check_rows(h, rows, n, slot)) return r;
  StageRing* ring = &h->stage;
  if (int r = wait_staged(*ring, slot)) return r;  // the slot's previous job
  if (!ring->stager) {
    ring->stager = new (std::nothrow) impala_host::Stager(stage_cpus(ring->device));
    if (!ring->stager) return fail(IMPALA_E_STATE, "impala_stage_rows_async: staging thread");
  }
  // the job owns copies of the five pointer arrays; the rows themselves stay the caller's
  auto p = std::make_shared<std::vector<const void*>>();
  p->reserve(5 * (size_t)n);
  const void* const* f[5] = {rows->obs, rows->actions, rows->rewards, rows->discounts,
                             rows->behaviour_logits};
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < n; ++b) p->push_back(f[k] ? f[k][b] : nullptr);
  ring->stager->submit(slot, [ring, p, n, slot](std::string& msg) {
    const void* const* d = p->data();
    const impala_rows r{d, d + n, d + 2 * n, d[3 * n] ? d + 3 * n : nullptr, d + 4 * n};
    const int st = stage_rows_now(*ring, &r, n, slot);
    if (st) msg = impala_last_error();
    return st;
  });
  return 0;
}

int impala_stage_wait(impala_learner* h, int slot) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (slot < 0 || slot >= h->stage.n_slots) return fail(IMPALA_E_INVALID, "slot out of range");
  if (int r = wait_staged(h->stage, slot)) return r;
  CK(hipEventSynchronize(h->stage.slots[slot].ready));
  return 0;
}

int impala_slot_batch(impala_learner* h, int slot, void* stream, impala_batch* out) {
  if (!h || !out) return fail(IMPALA_E_INVALID, "null argument");
  if (slot < 0 || slot >= h->stage.n_slots) return fail(IMPALA_E_INVALID, "slot out of range");
  if (int r = wait_staged(h->stage, slot)) return r;  // its copies are enqueued (ready recorded)
  CK(hipSetDevice(h->device));
  CK(hipStreamWaitEvent((hipStream_t)stream, h->stage.slots[slot].ready, 0));
  *out = h->stage.slots[slot].dev;
  return 0;
}

int impala_slot_release(impala_learner* h, int slot, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (slot < 0 || slot >= h->stage.n_slots) return fail(IMPALA_E_INVALID, "slot out of range");
  CK(hipSetDevice(h->device));
  CK(hipEventRecord(h->stage.slots[slot].done, (hipStream_t)stream));
  return 0;
}

int impala_kernel_count(void) { return K_COUNT; }
const char* impala_kernel_name(int kernel_id) {
  return (kernel_id >= 0 && kernel_id < K_COUNT) ? kKernelNames[kernel_id] : "";
}

int impala_timer_start(impala_learner* h, int kernel_id, int max_launches) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (kernel_id < -1 || kernel_id >= K_COUNT || max_launches < 0)
    return fail(IMPALA_E_INVALID, "bad kernel id / capacity");
  CK(hipSetDevice(h->device));
  if (kernel_id < 0) {  // disarm every timer
    for (auto& t : h->timers) t.armed = false;
    h->timers_armed = 0;
    return 0;
  }
  auto& t = h->timers[kernel_id];
  if (max_launches > t.cap) {
    for (int i = 0; i < 2 * t.cap; ++i) (void)hipEventDestroy(t.ev[i]);
    delete[] t.ev;
    t.ev = new hipEvent_t[2 * max_launches]();
    t.cap = 0;
    for (int i = 0; i < 2 * max_launches; ++i) CK(hipEventCreate(&t.ev[i]));
    t.cap = max_launches;
  }
  if (!t.armed) h->timers_armed++;
  t.armed = true;
  t.n = 0;
  h->timer_last = kernel_id;
  return 0;
}

int impala_timer_read_kernel(impala_learner* h, int kernel_id, float* total_ms, int* launches) {
  if (!h || !total_ms || !launches) return fail(IMPALA_E_INVALID, "null argument");
  if (kernel_id < 0 || kernel_id >= K_COUNT) return fail(IMPALA_E_INVALID, "bad kernel id");
  CK(hipSetDevice(h->device));
  auto& t = h->timers[kernel_id];
  float tot = 0.f;
  for (int i = 0; i < t.n; ++i) {
    CK(hipEventSynchronize(t.ev[2 * i + 1]));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = t.n;
  if (t.armed) h->timers_armed--;
  t.armed = false;
  t.n = 0;
  return 0;
}

int impala_step_clock(impala_learner* h, unsigned long long* stamps, int n) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (n < 0 || (n > 0 && !stamps)) return fail(IMPALA_E_INVALID, "bad step clock buffer / count");
  h->clock_buf = n > 0 ? stamps : nullptr;
  h->clock_n = n;
  h->clock_i = 0;
  return 0;
}

int impala_step_clock_end(impala_learner* h, void* stream, int* steps) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->clock_buf) return fail(IMPALA_E_STATE, "step clock not armed");
  CK(hipSetDevice(h->device));
  unsigned long long* out = h->clock_buf + h->clock_i;
  if (steps) *steps = h->clock_i;
  h->clock_buf = nullptr;
  h->clock_n = h->clock_i = 0;
  if (int r = klaunch(h, -1, "clock_stamp", clock_stamp_kernel, dim3(1), dim3(64),
                      (hipStream_t)stream, out))
    return r;
  return 0;
}

int impala_timer_read(impala_learner* h, float* total_ms, int* launches) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (h->timer_last < 0) {
    if (!total_ms || !launches) return fail(IMPALA_E_INVALID, "null argument");
    *total_ms = 0.f;
    *launches = 0;
    return 0;
  }
  return impala_timer_read_kernel(h, h->timer_last, total_ms, launches);
}

int impala_vtrace(const float* v_tm1, const float* v_t, const float* r_t, const float* discount_t,
                  const float* rho_tm1, int B, int L, float lambda_, float clip_rho_threshold,
                  float clip_pg_rho_threshold, float* pg_advantage, float* td_error,
                  float* q_estimate, void* stream) {
  if (B < 1 || L < 1 || L > 64) return fail(IMPALA_E_INVALID, "need B >= 1 and 1 <= L <= 64");
  if (!v_tm1 || !v_t || !r_t || !discount_t || !rho_tm1 || !pg_advantage || !td_error ||
      !q_estimate)
    return fail(IMPALA_E_INVALID, "null pointer");
  const int S = next_pow2(L);
  const int wgs = cdiv(B, 4 * (64 / S));
  vtrace_kernel<<<wgs, 256, 0, (hipStream_t)stream>>>(v_tm1, v_t, r_t, discount_t, rho_tm1, B, L, S,
                                                      lambda_, clip_rho_threshold,
                                                      clip_pg_rho_threshold, pg_advantage,
                                                      td_error, q_estimate);
  CK_LAUNCH("vtrace");
  return 0;
}

int impala_loss_head(const float* logits, const float* values, const int64_t* actions,
                     const float* rewards, const float* discounts, const float* behaviour_logits,
                     int B, int T, int A, float entropy_coeff, float lambda_, float clip_rho,
                     float clip_pg_rho, int vtrace_grad_mode, float* dlogits, float* dvalues,
                     float* metrics6, float* adv, float* err, float* q, float* rho, void* stream) {
  if (B < 1 || T < 2 || T > 64 || A < 1 || A > net::MAX_A)
    return fail(IMPALA_E_INVALID, "need B >= 1, 2 <= T <= 64, 1 <= A <= 15");
  if (vtrace_grad_mode < IMPALA_VTRACE_SG_ADVANTAGE || vtrace_grad_mode > IMPALA_VTRACE_SG_NONE)
    return fail(IMPALA_E_INVALID, "unknown vtrace_grad_mode");
  if (!logits || !values || !actions || !rewards || !discounts || !behaviour_logits || !dlogits ||
      !dvalues || !metrics6)
    return fail(IMPALA_E_INVALID, "null pointer");
  const bool dbg = adv && err && q;
  hipStream_t st = (hipStream_t)stream;
  const int S = next_pow2(T);
  const int wgs = cdiv(B, 4 * (64 / S));
  float* part = nullptr;
  CK(hipMallocAsync((void**)&part, (size_t)wgs * 8 * 4, st));
  LossArgs la{};
  la.logits = logits; la.lg_ld = A; la.values = values; la.v_ld = 1;
  la.act = actions; la.rew = rewards; la.disc = discounts; la.mu = behaviour_logits;
  la.B = B; la.T = T; la.A = A; la.S = S; la.vt_mode = vtrace_grad_mode;
  la.lam = lambda_; la.crho = clip_rho; la.cpg = clip_pg_rho; la.ent_coef = entropy_coeff;
  la.partials = part;
  la.dbg_adv = dbg ? adv : nullptr; la.dbg_err = dbg ? err : nullptr; la.dbg_q = dbg ? q : nullptr;
  la.dbg_rho = rho;
  loss_head_kernel<float><<<wgs, 256, 0, st>>>(la, dlogits, A, dvalues, 1, 0);
  CK_LAUNCH("loss_head");
  finalize_loss_kernel<<<1, 64, 0, st>>>(part, wgs, B, T, entropy_coeff, metrics6);
  CK_LAUNCH("finalize_loss");
  CK(hipFreeAsync(part, st));
  return 0;
}

int impala_ppo_loss_head(const float* logits, const float* values, const int64_t* actions,
                         const float* targets, const float* behaviour_logits, int N, int A,
                         float entropy_coeff, float clip_coeff, float* dlogits, float* dvalues,
                         float* metrics7, void* stream) {
  if (N < 1 || A < 1 || A > net::MAX_A) return fail(IMPALA_E_INVALID, "need N >= 1, 1 <= A <= 15");
  if (!logits || !values || !actions || !targets || !behaviour_logits || !dlogits || !dvalues ||
      !metrics7)
    return fail(IMPALA_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int wgs = cdiv(N, 256);
  float *part = nullptr, *m9 = nullptr;
  CK(hipMallocAsync((void**)&part, (size_t)wgs * 8 * 4, st));
  CK(hipMallocAsync((void**)&m9, IMPALA_NUM_METRICS * 4, st));
  ppo_loss_head_kernel<<<wgs, 256, 0, st>>>(logits, values, actions, targets, behaviour_logits, N,
                                            A, entropy_coeff, (float)(1.0 - (double)clip_coeff),
                                            (float)(1.0 + (double)clip_coeff), dlogits, dvalues,
                                            part);
  CK_LAUNCH("ppo_loss_head");
  finalize_ppo_kernel<<<1, 64, 0, st>>>(part, wgs, N, entropy_coeff, m9);
  CK_LAUNCH("finalize_ppo");
  CK(hipMemcpyAsync(metrics7, m9, 6 * 4, hipMemcpyDeviceToDevice, st));
  CK(hipMemcpyAsync(metrics7 + 6, m9 + IMPALA_M_TARGET, 4, hipMemcpyDeviceToDevice, st));
  CK(hipFreeAsync(part, st));
  CK(hipFreeAsync(m9, st));
  return 0;
}

}  // extern "C"

// the Ape-X DQN entry points (include/dqn_hip.h) on the launchers above
#include "dqn.h"
#include "dqn_replay.h"
#include "iqn.h"
#include "iqn_replay.h"
