// Where things are in the IMPALA ResNet unit (resnet.hip, resnet_bwd.h): the convolutions' geometry,
// the stage-tensor and pool-winner tables, the side vector, the flat parameter buffer's offsets and the
// handle's workspace carve.  Plain C++ for host and device: tests/resnet_layout_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/resnet_hip.h"
#include "arena.h"
#include "net.h"

#if defined(__HIPCC__)
#define RN_HD __host__ __device__
#else
#define RN_HD  // a host compiler
#endif

constexpr int RN_FEAT = RESNET_FEATURES, RN_HID = RESNET_HIDDEN;
constexpr int RN_CONVS = 15;
constexpr int RN_KSPLIT = 8;  // the FC's K chunks
// fp32 side vector (floats): conv biases [15][32], LayerNorm affine in kernel order, bfc, wh, bh
constexpr int RV_CB = 0, RV_LNG = RN_CONVS * 32, RV_LNB = RV_LNG + RN_FEAT, RV_BFC = RV_LNB + RN_FEAT,
              RV_WH = RV_BFC + RN_HID, RV_BH = RV_WH + net::HEADS * RN_HID, RV_TOTAL = RV_BH + net::HEADS;

// geometry of conv `id` (5 per stage: the pooled conv, then conv0, conv1 of the two blocks)
struct ConvGeo { int cin, cout; };
RN_HD constexpr ConvGeo conv_geo(int id) { return id == 0 ? ConvGeo{3, 16} : id < 5 ? ConvGeo{16, 16} : id == 5 ? ConvGeo{16, 32} : ConvGeo{32, 32}; }
RN_HD constexpr int kernel_cin(int cin) { return cin == 3 ? 4 : cin; }  // the stem's pixels are 4 bytes
inline int conv_nks_rt(int cin, int kstep) { return (9 * cin + kstep - 1) / kstep; }

// stage tensors (what debug = 1 exports and train = 1 saves for the backward; the backward's gws has the
// same layout): elements per frame of id 0..14, and the element offset of an id's block (x frames)
RN_HD constexpr int dbg_size(int id) { return id < 5 ? 32 * 32 * 16 : id < 10 ? 16 * 16 * 32 : 8 * 8 * 32; }
RN_HD constexpr int dbg_off(int id) {
  return id < 5 ? id * 16384 : id < 10 ? 81920 + (id - 5) * 8192 : 122880 + (id - 10) * 2048;
}
constexpr int RN_DBG_FRAME = 133120;
static_assert(dbg_off(14) + dbg_size(14) == RN_DBG_FRAME, "a frame's stage tensors");
// element offset of stage tensor `id` of frame f in a block of B frames, [id][B][H][H][C]
RN_HD constexpr size_t stage_at(int B, int id, int f) { return (size_t)B * dbg_off(id) + (size_t)f * dbg_size(id); }

// the pools' winning taps: bytes per frame, and a stage's offset in a frame's block ([HO][HO][C] each)
constexpr int RN_AMAX_FRAME = 16384 + 8192 + 2048;
RN_HD constexpr int amax_off(int stage) { return stage == 0 ? 0 : stage == 1 ? 16384 : 24576; }

// offsets in the flat parameter buffer (state_dict order)
struct GradOff {
  int w[RN_CONVS], b[RN_CONVS];
  int lng, lnb, wfc, bfc, wa, ba, wc, bc;
};
inline size_t body_offsets(int (&w)[RN_CONVS], int (&b)[RN_CONVS]) {
  size_t o = 0;
  for (int id = 0; id < RN_CONVS; ++id) {
    const ConvGeo g = conv_geo(id);
    w[id] = (int)o; o += (size_t)g.cout * g.cin * 9;
    b[id] = (int)o; o += g.cout;
  }
  return o;
}
inline GradOff flat_offsets(int A) {
  GradOff g;
  size_t o = body_offsets(g.w, g.b);
  g.lng = (int)o; o += RN_FEAT;
  g.lnb = (int)o; o += RN_FEAT;
  g.wfc = (int)o; o += (size_t)RN_HID * RN_FEAT;
  g.bfc = (int)o; o += RN_HID;
  g.wa = (int)o; o += (size_t)A * RN_HID;
  g.ba = (int)o; o += A;
  g.wc = (int)o; o += RN_HID;
  g.bc = (int)o;
  return g;
}
inline size_t flat_total(int A) { return (size_t)flat_offsets(A).bc + 1; }

// ---- the handle's workspace: one allocation, carved below
struct ResnetBufs {
  void* w[RN_CONVS];  // fragment-major conv weights of the compute type T
  void* wfc;          // likewise, [nt][ks][s][lane][j]
  float* vecs;        // RV_*
  void* y;            // [B][2048] T, kernel order p*32 + c
  float* part;        // [8][B][256]: the projection's K chunks
  void* h;            // [B][256] T
  float* heads;       // [B][16]
  void* stages;       // debug or train: the stage tensors [15][B][H][H][C] T
  // train only: the pools' winning taps [B][RN_AMAX_FRAME], (mean, rstd) [B][2], the data gradients'
  // weights of convs 1..14 (T, fragment-major), Wfc transposed (fp32, in bf16 mode the rounded values),
  // gz [B][256], gy [B][2048], the gradient at every conv's output (T, the stage tensors' layout), the
  // weight gradients' partial sums per frame group
  uint8_t* amax;
  float* lnstat;
  void* wd[RN_CONVS];
  float *wfct, *gz, *gy;
  void* gws;
  float* slab;
};
// frame groups of the weight-gradient kernels
inline int resnet_wg_groups(int B, int n_cu) { return B < n_cu / 4 ? B : n_cu / 4 > 0 ? n_cu / 4 : 1; }

// arena.h's two-pass carve: on Arena{} it returns the bytes to allocate, on the allocation it points b
inline size_t resnet_carve(ResnetBufs& b, const resnet_config& cfg, int n_cu, Arena a) {
  auto F = [&](size_t bytes) { return (float*)a.take(bytes); };
  const size_t es = cfg.dtype == IMPALA_DTYPE_BF16 ? 2 : 4, B = (size_t)cfg.batch_size;
  const int kstep = es == 2 ? 32 : 16;  // Frag<T>::KSTEP
  const size_t groups = (size_t)resnet_wg_groups(cfg.batch_size, n_cu);
  b = ResnetBufs{};
  for (int id = 0; id < RN_CONVS; ++id)
    b.w[id] = a.take((size_t)conv_geo(id).cout * conv_nks_rt(kernel_cin(conv_geo(id).cin), kstep) * kstep * es);
  b.wfc = a.take((size_t)RN_HID * RN_FEAT * es);
  b.vecs = F((size_t)RV_TOTAL * 4);
  b.y = a.take(B * RN_FEAT * es);
  b.part = F((size_t)RN_KSPLIT * B * RN_HID * 4);
  b.h = a.take(B * RN_HID * es);
  b.heads = F(B * net::HEADS * 4);
  if (cfg.debug || cfg.train) b.stages = a.take(B * RN_DBG_FRAME * es);
  if (cfg.train) {
    b.amax = (uint8_t*)a.take(B * RN_AMAX_FRAME);
    b.lnstat = F(B * 2 * 4);
    for (int id = 1; id < RN_CONVS; ++id)  // rows cin, K = 9 cout up to whole K-steps
      b.wd[id] = a.take((size_t)conv_geo(id).cin * conv_nks_rt(conv_geo(id).cout, kstep) * kstep * es);
    b.wfct = F((size_t)RN_HID * RN_FEAT * 4);
    b.gz = F(B * RN_HID * 4);
    b.gy = F(B * RN_FEAT * 4);
    b.gws = a.take(B * RN_DBG_FRAME * es);
    b.slab = F(groups * RESNET_BODY_PARAMS * 4);
  }
  return Arena::align(a.used);
}

// ---- the learner step's workspace (resnet_step_init): its own allocation, carved the same way.
// B trajectories of T frames, A actions.
constexpr int RN_SUMSQ_WGS = 128;  // workgroups of resnet_sumsq_kernel = clip-norm partial sums
constexpr int RN_TPART = 8;        // floats of a trajectory's metric partial sums (five used)
struct ResnetStepBufs {
  float* dl;      // [B T][A]: d loss / d logits, as resnet_head_bwd_kernel reads it
  float* dv;      // [B T]:    d loss / d values
  float* tpart;   // [B][RN_TPART]: sums over a trajectory of log pi(a) adv, err^2, H, KL, rho
  float* sqpart;  // [RN_SUMSQ_WGS]
  float* sc;      // [4]: Adam's step size lr / (1 - b1^t) and sqrt(1 - b2^t) of the step under way
  int64_t* step;  // Adam's step count
};
inline size_t resnet_step_carve(ResnetStepBufs& b, int B, int T, int A, Arena a) {
  auto F = [&](size_t bytes) { return (float*)a.take(bytes); };
  const size_t n = (size_t)B * T;
  b = ResnetStepBufs{};
  b.dl = F(n * A * 4);
  b.dv = F(n * 4);
  b.tpart = F((size_t)B * RN_TPART * 4);
  b.sqpart = F((size_t)RN_SUMSQ_WGS * 4);
  b.sc = F(4 * 4);
  b.step = (int64_t*)a.take(8);
  return Arena::align(a.used);
}
// the flat buffer as 16-byte vectors and a scalar tail: 626,240 + 257 (A + 1) floats, a multiple of four
// only where A = 3 (mod 4)
inline int flat_tail(int A) { return (int)(flat_total(A) & 3); }
