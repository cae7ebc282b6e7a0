// The IMPALA ResNet actor-critic (include/resnet_hip.h): the actor path's kernels, the launchers and
// the handle (the backward pass's kernels: resnet_bwd.h; the learner step's: resnet_step.h,
// §17), a translation unit of its own -- the other units' code objects are the same with or
// without it.  DESIGN.md §15 has the design and the LDS map.
//
// One forward of n frames is four launches:
//   resnet_trunk_kernel  one frame per workgroup (512 threads, persistent over frames): the 15
//                        convolutions, three max-pools, the residual adds, ReLU and LayerNorm with
//                        every activation in LDS; y [n][2048] is its only output
//   resnet_fc_kernel     Linear(2048, 256) split 16 (N tiles) x 8 (K chunks) over 128 workgroups,
//                        each streaming its own 1/128 of the weights once; partial sums [8][n][256]
//   resnet_heads_kernel  one wave per frame: the K chunks summed in order, bias, GELU, h, the heads
//   act_heads_kernel / split_heads_kernel (act_kernels.h)
//
// Convolutions are implicit GEMMs D[oc][pixel] = sum_k W[oc][k] X[pixel][k], k = tap * Cin + ci:
// the weights are the A operand (fragment-major in HBM, a wave's fragments in registers for the
// whole call), the B operand is read straight from the channels-last LDS tensor, whose one-pixel
// zero halo is the padding.  A lane's four accumulators are four consecutive output channels of
// one pixel: one vector store to a channels-last tensor.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/resnet_hip.h"
#include "arena.h"
#include "common.h"
#include "gemm.h"
#include "host.h"
#include "net.h"

namespace {
// this unit's own copies of act_heads_kernel and split_heads_kernel, and the unit's layout (what the
// two headers include is included above, at global scope)
#include "act_kernels.h"
#include "resnet_layout.h"

constexpr int RN_THREADS = 512, RN_WAVES = 8;
constexpr int RN_KCHUNK = RN_FEAT / RN_KSPLIT;
template <typename T, int CIN> constexpr int conv_nks() { return (9 * CIN + Frag<T>::KSTEP - 1) / Frag<T>::KSTEP; }

// ---- LDS map (bytes) of one frame, T the compute type.  S1..S3: a stage's tensor with its halo.
template <typename T> struct Lds {
  static constexpr int S1 = 34 * 34 * 16 * (int)sizeof(T), S2 = 18 * 18 * 32 * (int)sizeof(T),
                       S3 = 10 * 10 * 32 * (int)sizeof(T);
  static constexpr int IMG = 66 * 66 * 4;                                  // u8 [66][66][4]
  static constexpr int STRIP0 = 9 * 64 * 16 * 4, STRIP1 = 5 * 32 * 32 * 4, STRIP2 = 9 * 16 * 32 * 4;
  // stem: x1 [0, S1), image, strip.  stage 1: x1, t1.  stage 2: conv reads x1, x2 at S1, strip behind
  // it; blocks: t2 at 0.  stage 3: conv reads x2, x3 at 0, t3, strip; blocks in place.
  static constexpr int X1 = 0, IMG_AT = S1, STRIP0_AT = S1 + IMG, T1 = S1;
  static constexpr int X2 = S1, STRIP1_AT = S1 + S2, T2 = 0;
  static constexpr int X3 = 0, T3 = S3, STRIP2_AT = 2 * S3;
  static constexpr int m2(int a, int b) { return a > b ? a : b; }
  static constexpr int RED = m2(m2(2 * S1, STRIP0_AT + STRIP0), STRIP1_AT + STRIP1);
  static constexpr int TOTAL = RED + 64 * 4;
  static_assert(STRIP2_AT + STRIP2 <= S1, "stage 3 lives below x2");
  static_assert(TOTAL <= 160 * 1024, "the CU's LDS");
  static_assert(S1 % 16 == 0 && S2 % 16 == 0 && S3 % 16 == 0 && IMG % 16 == 0, "16-byte zeroing");
};

struct TrunkArgs {
  const uint8_t* obs;
  int n, B;
  const void* w[RN_CONVS];  // fragment-major weights of the compute type
  const float* vecs;
  void* y;        // [n][2048] compute type, kernel order p*32 + c
  void* stages;   // debug / train only: the stage tensors
  uint8_t* amax;  // train only: the winning tap of every pooled element
  float* lnstat;  // train only: (mean, rstd) of the LayerNorm per frame
};

DEV void lds_zero(char* p, int bytes) {
  for (int i = threadIdx.x * 16; i < bytes; i += RN_THREADS * 16) *reinterpret_cast<i32x4*>(p + i) = i32x4{0, 0, 0, 0};
}

// eight per-wave partial sums, in order
DEV float sum8(const float* red) { return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7])); }

// frame f's image into img [66][66] (zeroed): bytes of three planes -> pixels (c0, c1, c2, 0) as dwords
// inside the zero border
DEV void load_image(const uint8_t* __restrict__ obs, int f, uint32_t* img) {
  const int tid = threadIdx.x;
  if (tid < 256) {
    const int yy = tid >> 2, x0 = (tid & 3) * 16;
    const uint8_t* src = obs + (size_t)f * 12288 + yy * 64 + x0;
    const i32x4 p0 = *reinterpret_cast<const i32x4*>(src), p1 = *reinterpret_cast<const i32x4*>(src + 4096),
                p2 = *reinterpret_cast<const i32x4*>(src + 8192);
    uint32_t* dst = img + (yy + 1) * 66 + x0 + 1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int sh = 8 * (j & 3);
      dst[j] = (((uint32_t)p0[j >> 2] >> sh) & 255u) | ((((uint32_t)p1[j >> 2] >> sh) & 255u) << 8) |
               ((((uint32_t)p2[j >> 2] >> sh) & 255u) << 16);
    }
  }
}

DEV f32x4 relu_v(f32x4 v) { return __builtin_elementwise_max(v, f32x4{0.f, 0.f, 0.f, 0.f}); }
// bf16: a negative value is a negative int16; max with 0 as integers (no NaN in an activation)
DEV bf16x8 relu_v(bf16x8 v) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_bit_cast(bf16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, v), z));
}

// element offset, from a pixel's top-left tap, of the lane's slice of K-step s: k0 = s KSTEP + grp KPL
// lies in tap k0 / CIN at channel k0 % CIN; a tap past the ninth (K padded up to a whole K-step,
// where the packed weights are zero) reads the ninth again: any finite value
template <typename T, int CIN, int PITCH> DEV int tap_off(int s, int grp) {
  const int k0 = s * Frag<T>::KSTEP + grp * Frag<T>::KPL;
  const int tap = min(k0 / CIN, 8), ci = k0 % CIN;
  return ((tap / 3) * PITCH + tap % 3) * CIN + ci;
}

// The tiles of ROWS conv rows (H wide, 16 pixels a tile) over the waves, two tiles in flight per wave
// so that MFMA e of one never waits on MFMA e - 1 of the same accumulator.  With two N tiles the
// even waves take output channels 0..15 and the odd ones 16..31.  ld(pixel base, s) returns the B
// fragment of K-step s; epi(y, x, c0, acc) takes channels c0..c0+3 of pixel (y, x).
template <typename T, int NKS, int COUT, int H, int ROWS, class Ld, class Epi>
DEV void conv_tiles(const T* __restrict__ wpk, int y0, Ld ld, Epi epi) {
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int NTL = COUT / 16, WSL = RN_WAVES / NTL, NTILES = ROWS * H / 16;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, grp = lane >> 4;
  const int nt = NTL == 2 ? (wave & 1) : 0, slot = NTL == 2 ? (wave >> 1) : wave;
  V wf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) wf[s] = F::load(wpk + ((size_t)(nt * NKS + s) * 64 + lane) * F::KPL);
  const int c0 = 16 * nt + 4 * grp;
  for (int t = slot; t < NTILES; t += 2 * WSL) {
    const bool two = t + WSL < NTILES;  // (uniform)
    const int pa = 16 * t + col, pb = 16 * (two ? t + WSL : t) + col;
    const int ya = y0 + pa / H, xa = pa % H, yb = y0 + pb / H, xb = pb % H;
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const V v0 = ld(ya, xa, s), v1 = ld(yb, xb, s);
#pragma unroll
      for (int e = 0; e < F::NE; ++e) {
        a0 = F::mma_e(e, wf[s], v0, a0);
        a1 = F::mma_e(e, wf[s], v1, a1);
      }
    }
    epi(ya, xa, c0, a0);
    if (two) epi(yb, xb, c0, a1);
  }
}

// a 3x3 pad-1 convolution of the halo tensor `in` [H+2][H+2][CIN] (ReLU on the operand read if RELU)
template <typename T, int CIN, int COUT, int H, int ROWS, bool RELU, class Epi>
DEV void conv_lds(const T* __restrict__ in, const T* __restrict__ wpk, int y0, Epi epi) {
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int NKS = conv_nks<T, CIN>(), P = H + 2;
  const int grp = (threadIdx.x & 63) >> 4;
  int off[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) off[s] = tap_off<T, CIN, P>(s, grp);
  conv_tiles<T, NKS, COUT, H, ROWS>(
      wpk, y0,
      [&](int y, int x, int s) {
        const V v = *reinterpret_cast<const V*>(in + (y * P + x) * CIN + off[s]);
        return RELU ? relu_v(v) : v;
      },
      epi);
}

// the stem's operand: image pixels as dwords (c0, c1, c2, 0) [66][66], the bytes converted on the
// read (exact in both types); k = tap * 4 + c
DEV f32x4 stem_frag(const uint32_t* __restrict__ px, const int (&o)[2], float) {
  const uint32_t d = px[o[0]];
  return f32x4{(float)(d & 255u), (float)((d >> 8) & 255u), (float)((d >> 16) & 255u), 0.f};
}
DEV bf16x8 stem_frag(const uint32_t* __restrict__ px, const int (&o)[2], __bf16) {
  const uint32_t d = px[o[0]], e = px[o[1]];
  bf16x8 v;
  v[0] = (__bf16)(float)(d & 255u); v[1] = (__bf16)(float)((d >> 8) & 255u);
  v[2] = (__bf16)(float)((d >> 16) & 255u); v[3] = (__bf16)0.f;
  v[4] = (__bf16)(float)(e & 255u); v[5] = (__bf16)(float)((e >> 8) & 255u);
  v[6] = (__bf16)(float)((e >> 16) & 255u); v[7] = (__bf16)0.f;
  return v;
}
template <typename T, int ROWS, class Epi>
DEV void conv_stem(const uint32_t* __restrict__ img, const T* __restrict__ wpk, int y0, Epi epi) {
  using F = Frag<T>;
  constexpr int NKS = conv_nks<T, 4>(), P = 66, TPL = F::KPL / 4;  // taps per lane and K-step
  const int grp = (threadIdx.x & 63) >> 4;
  int off[NKS][2];
#pragma unroll
  for (int s = 0; s < NKS; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int tap = min((s * 4 + grp) * TPL + (j < TPL ? j : 0), 8);
      off[s][j] = (tap / 3) * P + tap % 3;
    }
  conv_tiles<T, NKS, 16, 64, ROWS>(
      wpk, y0, [&](int y, int x, int s) { return stem_frag(img + y * P + x, off[s], T{}); }, epi);
}

// ---- epilogues.  c0 is fixed per lane within a call: the bias is loaded once.
// conv row y of a pooled conv -> the fp32 strip ring [RING][W][C]: acc * scale + b
template <int W, int C, int RING> struct EpiStrip {
  float* strip;
  const float* bias;
  float scale;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c0);
    *reinterpret_cast<f32x4*>(strip + ((y % RING) * W + x) * C + c0) = acc * scale + b;
  }
};
// t = T(acc + b) into the interior of a halo tensor
template <typename T, int H, int C> struct EpiStore {
  T* out;
  const float* bias;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c0);
    const float o[4] = {acc[0] + b[0], acc[1] + b[1], acc[2] + b[2], acc[3] + b[3]};
    store4(out + ((y + 1) * (H + 2) + x + 1) * C + c0, o);
  }
};
// x = T(fp32(x) + (acc + b)), in place (the convolution reads t only)
template <typename T, int H, int C> struct EpiResidual {
  T* x;
  const float* bias;
  DEV void operator()(int y, int xx, int c0, f32x4 acc) const {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c0);
    T* p = x + ((y + 1) * (H + 2) + xx + 1) * C + c0;
    float v[4];
    load4(p, v);
    const float o[4] = {v[0] + (acc[0] + b[0]), v[1] + (acc[1] + b[1]), v[2] + (acc[2] + b[2]),
                        v[3] + (acc[3] + b[3])};
    store4(p, o);
  }
};

// max_pool2d(kernel 3, stride 2, padding 1) of conv rows r0 .. r0 + SR - 1 (and row r0 - 1, still in
// the ring) -> output rows r0/2 .. r0/2 + SR/2 - 1 in the interior of `out`; a tap outside the
// image is left out (-inf padding).  The max is taken in fp32 and rounded once: rounding is monotone.
// TRAIN: amax [HO][HO][C] also takes the window's winning tap 0..8 (row-major; of equal values the first).
template <typename T, int HC, int C, int SR, bool TRAIN = false>
DEV void pool_rows(const float* __restrict__ strip, T* __restrict__ out, int r0, uint8_t* __restrict__ amax = nullptr) {
  constexpr int HO = HC / 2, RING = SR + 1, CV = C / 4, ITEMS = (SR / 2) * HO * CV;
  for (int i = threadIdx.x; i < ITEMS; i += RN_THREADS) {
    const int c0 = 4 * (i % CV), ox = (i / CV) % HO, oy = r0 / 2 + i / (CV * HO);
    f32x4 m = *reinterpret_cast<const f32x4*>(strip + (((2 * oy) % RING) * HC + 2 * ox) * C + c0);
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int r = 2 * oy + dy, cx = 2 * ox + dx;  // (never past HC - 1)
        if ((dy || dx) && r >= 0 && cx >= 0)
          m = __builtin_elementwise_max(m, *reinterpret_cast<const f32x4*>(strip + ((r % RING) * HC + cx) * C + c0));
      }
    const float o[4] = {m[0], m[1], m[2], m[3]};
    store4(out + ((oy + 1) * (HO + 2) + ox + 1) * C + c0, o);
    if constexpr (TRAIN) {
      uint32_t win = 0;  // taps in reverse order: the first of equal values is written last
#pragma unroll
      for (int tap = 8; tap >= 0; --tap) {
        const int r = 2 * oy + tap / 3 - 1, cx = 2 * ox + tap % 3 - 1;
        if (r >= 0 && cx >= 0) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(strip + ((r % RING) * HC + cx) * C + c0);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (v[q] == m[q]) win = (win & ~(255u << (8 * q))) | ((uint32_t)tap << (8 * q));
        }
      }
      *reinterpret_cast<uint32_t*>(amax + (oy * HO + ox) * C + c0) = win;
    }
  }
}

// debug: the interior of a halo tensor -> HBM [H][H][C]
template <typename T, int H, int C> DEV void dump(const T* __restrict__ t, T* __restrict__ dst) {
  for (int i = threadIdx.x; i < H * H * C / 4; i += RN_THREADS) {
    const int c0 = 4 * (i % (C / 4)), p = i / (C / 4);
    float v[4];
    load4(t + ((p / H + 1) * (H + 2) + p % H + 1) * C + c0, v);
    store4(dst + p * C + c0, v);
  }
}

// the two residual blocks of a stage on x (halo tensor) with scratch t; ends on a barrier
template <typename T, bool DEBUG, int C, int H>
DEV void res_blocks(T* x, T* t, const TrunkArgs& a, int id0, int f) {
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const int i0 = id0 + 2 * blk, i1 = i0 + 1;
    conv_lds<T, C, C, H, H, true>(x, reinterpret_cast<const T*>(a.w[i0]), 0,
                                  EpiStore<T, H, C>{t, a.vecs + RV_CB + 32 * i0});
    __syncthreads();
    if constexpr (DEBUG)
      dump<T, H, C>(t, reinterpret_cast<T*>(a.stages) + stage_at(a.B, i0, f));
    conv_lds<T, C, C, H, H, true>(t, reinterpret_cast<const T*>(a.w[i1]), 0,
                                  EpiResidual<T, H, C>{x, a.vecs + RV_CB + 32 * i1});
    __syncthreads();
    if constexpr (DEBUG)
      dump<T, H, C>(x, reinterpret_cast<T*>(a.stages) + stage_at(a.B, i1, f));
  }
}

template <typename T, bool DEBUG, bool TRAIN = false>
__global__ __launch_bounds__(RN_THREADS) void resnet_trunk_kernel(const TrunkArgs a) {
  using L = Lds<T>;
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* const red = reinterpret_cast<float*>(lds + L::RED);
  for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
    auto dbg_at = [&](int id) { return reinterpret_cast<T*>(a.stages) + stage_at(a.B, id, f); };
    auto win_at = [&](int stage) { return TRAIN ? a.amax + (size_t)f * RN_AMAX_FRAME + amax_off(stage) : nullptr; };
    // ---- the image
    T* x1 = reinterpret_cast<T*>(lds + L::X1);
    uint32_t* img = reinterpret_cast<uint32_t*>(lds + L::IMG_AT);
    lds_zero(lds + L::X1, L::S1);
    lds_zero(lds + L::IMG_AT, L::IMG);
    __syncthreads();
    load_image(a.obs, f, img);
    __syncthreads();
    {  // ---- stem: conv 3 -> 16 at 64 x 64 in strips of 8 rows, pooled to x1 [32][32][16]
      float* strip = reinterpret_cast<float*>(lds + L::STRIP0_AT);
      for (int r0 = 0; r0 < 64; r0 += 8) {
        conv_stem<T, 8>(img, reinterpret_cast<const T*>(a.w[0]), r0,
                        EpiStrip<64, 16, 9>{strip, a.vecs + RV_CB, 1.f / 255.f});
        __syncthreads();
        pool_rows<T, 64, 16, 8, TRAIN>(strip, x1, r0, win_at(0));
        __syncthreads();
      }
    }
    if constexpr (DEBUG) dump<T, 32, 16>(x1, dbg_at(0));
    T* t1 = reinterpret_cast<T*>(lds + L::T1);
    lds_zero(lds + L::T1, L::S1);
    __syncthreads();
    res_blocks<T, DEBUG, 16, 32>(x1, t1, a, 1, f);
    // ---- stage 2: conv 16 -> 32 at 32 x 32 in strips of 4 rows, pooled to x2 [16][16][32]
    T* x2 = reinterpret_cast<T*>(lds + L::X2);
    lds_zero(lds + L::X2, L::S2);
    __syncthreads();
    {
      float* strip = reinterpret_cast<float*>(lds + L::STRIP1_AT);
      for (int r0 = 0; r0 < 32; r0 += 4) {
        conv_lds<T, 16, 32, 32, 4, false>(x1, reinterpret_cast<const T*>(a.w[5]), r0,
                                          EpiStrip<32, 32, 5>{strip, a.vecs + RV_CB + 32 * 5, 1.f});
        __syncthreads();
        pool_rows<T, 32, 32, 4, TRAIN>(strip, x2, r0, win_at(1));
        __syncthreads();
      }
    }
    if constexpr (DEBUG) dump<T, 16, 32>(x2, dbg_at(5));
    T* t2 = reinterpret_cast<T*>(lds + L::T2);
    lds_zero(lds + L::T2, L::S2);
    __syncthreads();
    res_blocks<T, DEBUG, 32, 16>(x2, t2, a, 6, f);
    // ---- stage 3: conv 32 -> 32 at 16 x 16 in strips of 8 rows, pooled to x3 [8][8][32]
    T* x3 = reinterpret_cast<T*>(lds + L::X3);
    T* t3 = reinterpret_cast<T*>(lds + L::T3);
    lds_zero(lds + L::X3, 2 * L::S3);
    __syncthreads();
    {
      float* strip = reinterpret_cast<float*>(lds + L::STRIP2_AT);
      for (int r0 = 0; r0 < 16; r0 += 8) {
        conv_lds<T, 32, 32, 16, 8, false>(x2, reinterpret_cast<const T*>(a.w[10]), r0,
                                          EpiStrip<16, 32, 9>{strip, a.vecs + RV_CB + 32 * 10, 1.f});
        __syncthreads();
        pool_rows<T, 16, 32, 8, TRAIN>(strip, x3, r0, win_at(2));
        __syncthreads();
      }
    }
    if constexpr (DEBUG) dump<T, 8, 32>(x3, dbg_at(10));
    res_blocks<T, DEBUG, 32, 8>(x3, t3, a, 11, f);
    // ---- ReLU, LayerNorm over the 2048 features: thread -> pixel tid / 8, channels 4 (tid % 8) ..;
    // two-pass statistics, lanes by DPP / permlane in a fixed order, the 8 waves in order
    {
      const int p = tid >> 3, c0 = 4 * (tid & 7);
      float v[4];
      load4(x3 + (((p >> 3) + 1) * 10 + (p & 7) + 1) * 32 + c0, v);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
      const float s = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
      if (lane == 0) red[wave] = s;
      __syncthreads();
      const float mean = sum8(red) * (1.f / RN_FEAT);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] -= mean;
      const float sq = wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
      if (lane == 0) red[8 + wave] = sq;
      __syncthreads();
      const float var = sum8(red + 8) * (1.f / RN_FEAT);
      const float rstd = 1.f / sqrtf(var + LN_EPS);
      if constexpr (TRAIN) {
        if (tid == 0) {
          a.lnstat[2 * f] = mean;
          a.lnstat[2 * f + 1] = rstd;
        }
      }
      float g[4], b[4], o[4];
      load4(a.vecs + RV_LNG + p * 32 + c0, g);
      load4(a.vecs + RV_LNB + p * 32 + c0, b);
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = v[q] * rstd * g[q] + b[q];
      store4(reinterpret_cast<T*>(a.y) + (size_t)f * RN_FEAT + p * 32 + c0, o);
    }
    __syncthreads();  // x3 and red are rewritten by the next frame
  }
}

// Linear(2048, 256) without bias, as partial sums: workgroup (nt, ks) holds the 16 x 256 slab of
// Wfc (rows 16 nt .., K chunk ks) as A fragments in registers -- every wave the same slab, read from
// HBM once -- and wave w runs the 16-frame tiles w, w + 4, .. of y against it.  part [8][B][256].
template <typename T>
__global__ __launch_bounds__(256) void resnet_fc_kernel(const T* __restrict__ y, const T* __restrict__ wpk,
                                                        float* __restrict__ part, int n, int B) {
  using F = Frag<T>;
  typedef typename F::vec V;
  constexpr int NKS = RN_KCHUNK / F::KSTEP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int nt = blockIdx.x & 15, ks = blockIdx.x >> 4;
  V wf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s)
    wf[s] = F::load(wpk + ((size_t)((nt * RN_KSPLIT + ks) * NKS + s) * 64 + lane) * F::KPL);
  for (int r0 = wave * 16; r0 < n; r0 += 64) {
    const int fr = min(r0 + col, n - 1);
    const T* yr = y + (size_t)fr * RN_FEAT + ks * RN_KCHUNK + grp * F::KPL;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < NKS; s += 2) {
      const V v0 = F::load(yr + s * F::KSTEP), v1 = F::load(yr + (s + 1) * F::KSTEP);
#pragma unroll
      for (int e = 0; e < F::NE; ++e) {
        acc[0] = F::mma_e(e, wf[s], v0, acc[0]);
        acc[1] = F::mma_e(e, wf[s + 1], v1, acc[1]);
      }
    }
    if (r0 + col < n)
      *reinterpret_cast<f32x4*>(part + ((size_t)ks * B + fr) * RN_HID + nt * 16 + 4 * grp) = acc[0] + acc[1];
  }
}

// One wave per frame: z = (sum of the 8 K chunks, in order) + bfc, h = T(GELU(z)), heads = Wh h + bh
// in fp32 -- a lane four of the 256 terms per head, the lanes summed in wave_sum's fixed order.
template <typename T>
__global__ __launch_bounds__(256) void resnet_heads_kernel(const float* __restrict__ part, const float* __restrict__ vecs,
                                                           T* __restrict__ h, float* __restrict__ heads, int n, int B) {
  const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n) return;
  float acc[HEADS];
#pragma unroll
  for (int o = 0; o < HEADS; ++o) acc[o] = 0.f;
#pragma unroll
  for (int i = 0; i < RN_HID / 64; ++i) {
    const int j = lane + 64 * i;
    float z = part[(size_t)f * RN_HID + j];  // (resnet_head_bwd_kernel re-sums z in this order)
#pragma unroll
    for (int ks = 1; ks < RN_KSPLIT; ++ks) z += part[((size_t)ks * B + f) * RN_HID + j];
    z += vecs[RV_BFC + j];
    const T ht = (T)(0.5f * z * (1.f + erff(z * 0.70710678118654752440f)));
    h[(size_t)f * RN_HID + j] = ht;
    const float hf = (float)ht;
#pragma unroll
    for (int o = 0; o < HEADS; ++o) acc[o] = fmaf(vecs[RV_WH + o * RN_HID + j], hf, acc[o]);
  }
  float mine = 0.f;
#pragma unroll
  for (int o = 0; o < HEADS; ++o) {
    const float s = wave_sum(acc[o]);
    mine = lane == o ? s : mine;
  }
  if (lane < HEADS) heads[(size_t)f * HEADS + lane] = mine + vecs[RV_BH + lane];
}

// ---- packing (resnet_refresh_weights).  A conv's canonical [COUT][cin][3][3] -> fragment-major
// [nt][s][lane][j]: row oc = 16 nt + (lane & 15), k = s KSTEP + (lane >> 4) KPL + j = tap * CK + ci
// (CK the kernel's channel count: 4 for the stem); zero where tap > 8 or ci >= cin.
template <typename T>
__global__ __launch_bounds__(256) void resnet_pack_conv_kernel(const float* __restrict__ w, T* __restrict__ dst,
                                                               int cin, int ck, int nks, int total) {
  using F = Frag<T>;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = e % F::KPL, lane = (e / F::KPL) & 63, s = (e / (F::KPL * 64)) % nks, nt = e / (F::KPL * 64 * nks);
  const int oc = 16 * nt + (lane & 15), k = s * F::KSTEP + (lane >> 4) * F::KPL + j;
  const int tap = k / ck, ci = k % ck;
  dst[e] = (T)(tap < 9 && ci < cin ? w[((size_t)oc * cin + ci) * 9 + tap] : 0.f);
}
// Wfc canonical [256][2048] (column c*64 + p) -> [nt][ks][s][lane][j], k' = p*32 + c
template <typename T>
__global__ __launch_bounds__(256) void resnet_pack_fc_kernel(const float* __restrict__ w, T* __restrict__ dst) {
  using F = Frag<T>;
  constexpr int NKS = RN_KCHUNK / F::KSTEP;
  const int e = blockIdx.x * 256 + threadIdx.x;  // < 256 * 2048
  const int j = e % F::KPL, lane = (e / F::KPL) & 63, s = (e / (F::KPL * 64)) % NKS;
  const int ks = (e / (F::KPL * 64 * NKS)) % RN_KSPLIT, nt = e / (F::KPL * 64 * NKS * RN_KSPLIT);
  const int o = 16 * nt + (lane & 15), k = ks * RN_KCHUNK + s * F::KSTEP + (lane >> 4) * F::KPL + j;
  dst[e] = (T)w[(size_t)o * RN_FEAT + (k & 31) * 64 + (k >> 5)];
}
__global__ __launch_bounds__(256) void resnet_pack_vec_kernel(const float* __restrict__ flat, const GradOff o, int A,
                                                              float* __restrict__ vecs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= RV_TOTAL) return;
  float v = 0.f;
  if (i < RV_LNG) {
    const int id = i >> 5, c = i & 31;
    v = c < conv_geo(id).cout ? flat[o.b[id] + c] : 0.f;
  } else if (i < RV_BFC) {  // kernel order p*32 + c <- canonical c*64 + p
    const int k = (i - RV_LNG) & (RN_FEAT - 1);
    v = flat[(i < RV_LNB ? o.lng : o.lnb) + (k & 31) * 64 + (k >> 5)];
  } else if (i < RV_WH) {
    v = flat[o.bfc + i - RV_BFC];
  } else if (i < RV_BH) {
    const int r = (i - RV_WH) / RN_HID, j = (i - RV_WH) % RN_HID;
    v = r < A ? flat[o.wa + r * RN_HID + j] : r == VCOL ? flat[o.wc + j] : 0.f;
  } else {
    const int r = i - RV_BH;
    v = r < A ? flat[o.ba + r] : r == VCOL ? flat[o.bc] : 0.f;
  }
  vecs[i] = v;
}

#include "resnet_bwd.h"
#include "resnet_step.h"

}  // namespace

struct resnet_actor : ResnetBufs {  // the buffers: one allocation, ws (resnet_carve)
  resnet_config cfg;
  int device, n_cu;
  const float* flat = nullptr;
  bool packed = false;
  char* ws = nullptr;
  // train = 1 only
  int trained_n = 0;  // frames of the last resnet_forward_train; 0: none, or the weights were refreshed since
  int wg_groups = 0;  // frame groups of the weight-gradient kernels (resnet_wg_groups)
  // the learner step (resnet_step_init, resnet_bind_state)
  bool step_on = false;
  resnet_step_config sc;
  ResnetStepBufs sb;  // one allocation, step_ws (resnet_step_carve)
  char* step_ws = nullptr;
  float *params = nullptr, *grads = nullptr, *exp_avg = nullptr, *exp_avg_sq = nullptr, *metrics = nullptr;
  float* vt_dbg = nullptr;
};

namespace {

size_t elt(const resnet_actor* h) { return h->cfg.dtype == IMPALA_DTYPE_BF16 ? 2 : 4; }

int check_ready(resnet_actor* h, const uint8_t* obs, int n) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!obs) return fail(IMPALA_E_INVALID, "null pointer");
  if (n < 1 || n > h->cfg.batch_size) return fail(IMPALA_E_INVALID, "n must be in [1, batch_size]");
  if (((uintptr_t)obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  if (!h->flat) return fail(IMPALA_E_STATE, "resnet_bind_params not called");
  if (!h->packed) return fail(IMPALA_E_STATE, "resnet_refresh_weights not called since resnet_bind_params");
  return 0;
}

template <typename T> int launch_pack(resnet_actor* h, hipStream_t st) {
  const int A = h->cfg.num_actions;
  const GradOff go = flat_offsets(A);
  for (int id = 0; id < RN_CONVS; ++id) {
    const ConvGeo g = conv_geo(id);
    const int ck = kernel_cin(g.cin), nks = conv_nks_rt(ck, Frag<T>::KSTEP);
    const int total = g.cout * nks * Frag<T>::KSTEP;
    resnet_pack_conv_kernel<T><<<cdiv(total, 256), 256, 0, st>>>(h->flat + go.w[id], (T*)h->w[id], g.cin, ck, nks, total);
    CK_LAUNCH("resnet_pack_conv");
  }
  resnet_pack_fc_kernel<T><<<RN_HID * RN_FEAT / 256, 256, 0, st>>>(h->flat + go.wfc, (T*)h->wfc);
  CK_LAUNCH("resnet_pack_fc");
  resnet_pack_vec_kernel<<<cdiv(RV_TOTAL, 256), 256, 0, st>>>(h->flat, go, A, h->vecs);
  CK_LAUNCH("resnet_pack_vec");
  if (h->cfg.train) {  // the data gradients' layouts: taps flipped, Cin / Cout swapped; Wfc transposed
    for (int id = 1; id < RN_CONVS; ++id) {
      const ConvGeo g = conv_geo(id);
      const int nks = conv_nks_rt(g.cout, Frag<T>::KSTEP), total = g.cin * nks * Frag<T>::KSTEP;
      resnet_pack_dgrad_kernel<T><<<cdiv(total, 256), 256, 0, st>>>(h->flat + go.w[id], (T*)h->wd[id], g.cin, g.cout, nks, total);
      CK_LAUNCH("resnet_pack_dgrad");
    }
    resnet_pack_fct_kernel<T><<<RN_HID * RN_FEAT / 256, 256, 0, st>>>(h->flat + go.wfc, h->wfct);
    CK_LAUNCH("resnet_pack_fct");
  }
  return 0;
}

template <typename T, bool TRAIN = false> int launch_forward(resnet_actor* h, const uint8_t* obs, int n, hipStream_t st) {
  TrunkArgs a;
  a.obs = obs;
  a.n = n;
  a.B = h->cfg.batch_size;
  for (int id = 0; id < RN_CONVS; ++id) a.w[id] = h->w[id];
  a.vecs = h->vecs;
  a.y = h->y;
  a.stages = h->stages;
  a.amax = h->amax;
  a.lnstat = h->lnstat;
  h->trained_n = 0;  // this call rewrites y and the projection's sums
  const int grid = n < h->n_cu ? n : h->n_cu;
  if (TRAIN) resnet_trunk_kernel<T, true, TRAIN><<<grid, RN_THREADS, 0, st>>>(a);
  else if (h->cfg.debug) resnet_trunk_kernel<T, true><<<grid, RN_THREADS, 0, st>>>(a);
  else resnet_trunk_kernel<T, false><<<grid, RN_THREADS, 0, st>>>(a);
  CK_LAUNCH("resnet_trunk");
  resnet_fc_kernel<T><<<16 * RN_KSPLIT, 256, 0, st>>>((const T*)h->y, (const T*)h->wfc, h->part, n, a.B);
  CK_LAUNCH("resnet_fc");
  resnet_heads_kernel<T><<<cdiv(n, 4), 256, 0, st>>>(h->part, h->vecs, (T*)h->h, h->heads, n, a.B);
  CK_LAUNCH("resnet_heads");
  return 0;
}

// one weight-gradient launch: the fp32 or the bf16 kernel of the same geometry
template <typename T, int CIN, int COUT, int H, int R, bool POOLED, bool RELU, bool STEM>
void launch_wgrad(const WgArgs<T>& w, int G, int convs, int id0, hipStream_t st) {
  if constexpr (sizeof(T) == 2)
    resnet_wgrad_bf16_kernel<CIN, COUT, H, R, POOLED, RELU, STEM><<<dim3(G, convs), RN_THREADS, 0, st>>>(w, id0);
  else
    resnet_wgrad_kernel<CIN, COUT, H, R, POOLED, RELU, STEM><<<dim3(G, convs), RN_THREADS, 0, st>>>(w, id0);
}

template <typename T>
int launch_backward(resnet_actor* h, const uint8_t* obs, int n, const float* dl, const float* dv, float* grad, int acc,
                    hipStream_t st) {
  const int A = h->cfg.num_actions, B = h->cfg.batch_size;
  const GradOff go = flat_offsets(A);
  const T* sav = (const T*)h->stages;
  resnet_head_bwd_kernel<<<cdiv(n, 4), 256, 0, st>>>(h->part, h->vecs, dl, dv, h->gz, n, B, A);
  CK_LAUNCH("resnet_head_bwd");
  resnet_head_wgrad_kernel<T><<<HEADS + 1, 256, 0, st>>>((const T*)h->h, h->gz, dl, dv, grad, go, n, A, acc);
  CK_LAUNCH("resnet_head_wgrad");
  resnet_fc_wgrad_kernel<T><<<16 * (RN_FEAT / 256), 256, 0, st>>>(h->gz, (const T*)h->y, grad, go.wfc, n, acc);
  CK_LAUNCH("resnet_fc_wgrad");
  resnet_fc_dgrad_kernel<<<RN_FEAT / 16, 256, 0, st>>>(h->gz, h->wfct, h->gy, n);
  CK_LAUNCH("resnet_fc_dgrad");
  resnet_ln_affine_kernel<T><<<RN_FEAT / 256, 256, 0, st>>>(h->gy, sav + stage_at(B, 14, 0), h->lnstat, grad, go.lng,
                                                            go.lnb, n, acc);
  CK_LAUNCH("resnet_ln_affine");
  BwdArgs<T> b;
  b.n = n;
  b.B = B;
  for (int id = 0; id < RN_CONVS; ++id) b.wd[id] = (const T*)h->wd[id];
  b.vecs = h->vecs;
  b.sav = sav;
  b.amax = h->amax;
  b.lnstat = h->lnstat;
  b.gy = h->gy;
  b.gws = (T*)h->gws;
  if constexpr (sizeof(T) == 2)  // two workgroups a CU
    resnet_trunk_bwd_bf16_kernel<<<n < 2 * h->n_cu ? n : 2 * h->n_cu, RN_THREADS, 0, st>>>(b);
  else
    resnet_trunk_bwd_kernel<<<n < h->n_cu ? n : h->n_cu, RN_THREADS, 0, st>>>(b);
  CK_LAUNCH("resnet_trunk_bwd");
  WgArgs<T> w;
  w.obs = obs;
  w.n = n;
  w.B = B;
  w.sav = sav;
  w.gws = (const T*)h->gws;
  w.amax = h->amax;
  w.slab = h->slab;
  w.go = go;
  const int G = n < h->wg_groups ? n : h->wg_groups;
  //             CIN COUT  H  R  pooled relu  stem
  launch_wgrad<T, 4, 16, 64, 8, true, false, true>(w, G, 1, 0, st);
  CK_LAUNCH("resnet_wgrad stem");
  launch_wgrad<T, 16, 16, 32, 8, false, true, false>(w, G, 4, 1, st);
  CK_LAUNCH("resnet_wgrad stage 1");
  launch_wgrad<T, 16, 32, 32, 8, true, false, false>(w, G, 1, 5, st);
  CK_LAUNCH("resnet_wgrad conv 5");
  launch_wgrad<T, 32, 32, 16, 16, false, true, false>(w, G, 4, 6, st);
  CK_LAUNCH("resnet_wgrad stage 2");
  launch_wgrad<T, 32, 32, 16, 16, true, false, false>(w, G, 1, 10, st);
  CK_LAUNCH("resnet_wgrad conv 10");
  launch_wgrad<T, 32, 32, 8, 8, false, true, false>(w, G, 4, 11, st);
  CK_LAUNCH("resnet_wgrad stage 3");
  resnet_wreduce_kernel<<<cdiv(RESNET_BODY_PARAMS, 256), 256, 0, st>>>(h->slab, G, grad, acc);
  CK_LAUNCH("resnet_wreduce");
  return 0;
}

#define RN_BY_TYPE(h, fn, ...) \
  ((h)->cfg.dtype == IMPALA_DTYPE_BF16 ? fn<__bf16>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

// ---- the learner step
// what every step entry refuses before its first launch; `batch`: the entry reads one
int check_step(resnet_actor* h, const impala_batch* b, bool batch) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->cfg.train) return fail(IMPALA_E_INVALID, "the learner step needs a handle created with train = 1");
  if (!h->step_on) return fail(IMPALA_E_STATE, "resnet_step_init not called");
  if (!h->grads) return fail(IMPALA_E_STATE, "resnet_bind_state not called");
  if (batch) {
    if (!b || !b->obs || !b->actions || !b->rewards || !b->discounts || !b->behaviour_logits)
      return fail(IMPALA_E_INVALID, "null pointer");
    if (((uintptr_t)b->obs & 15) != 0) return fail(IMPALA_E_INVALID, "obs must be 16-byte aligned");
  }
  if (!h->packed) return fail(IMPALA_E_STATE, "resnet_refresh_weights not called since the parameters were bound");
  return 0;
}

int launch_loss_head(resnet_actor* h, const impala_batch* b, hipStream_t st) {
  const resnet_step_config& c = h->sc;
  VtHeadArgs a;
  a.heads = h->heads;
  a.act = b->actions; a.rew = b->rewards; a.disc = b->discounts; a.mu = b->behaviour_logits;
  a.B = c.batch_size; a.T = c.rollout_length; a.A = h->cfg.num_actions; a.vt_mode = c.vtrace_grad_mode;
  a.lam = c.vtrace_lambda; a.crho = c.clip_rho_threshold; a.cpg = c.clip_pg_rho_threshold;
  a.ent_coef = c.entropy_coeff;
  a.dl = h->sb.dl; a.dv = h->sb.dv; a.tpart = h->sb.tpart; a.vt_dbg = h->vt_dbg;
  resnet_vtrace_head_kernel<<<cdiv(a.B, 4), 256, 0, st>>>(a);
  CK_LAUNCH("resnet_vtrace_head");
  return 0;
}

int launch_compute_grads(resnet_actor* h, const impala_batch* b, hipStream_t st) {
  const int n = h->sc.batch_size * h->sc.rollout_length;
  if (int r = h->cfg.dtype == IMPALA_DTYPE_BF16 ? launch_forward<__bf16, true>(h, b->obs, n, st)
                                                : launch_forward<float, true>(h, b->obs, n, st))
    return r;
  h->trained_n = n;
  if (int r = launch_loss_head(h, b, st)) return r;
  return RN_BY_TYPE(h, launch_backward, h, b->obs, n, h->sb.dl, h->sb.dv, h->grads, 0, st);
}

int launch_apply_update(resnet_actor* h, hipStream_t st) {
  const resnet_step_config& c = h->sc;
  const int n = (int)flat_total(h->cfg.num_actions), nv = n >> 2;
  resnet_sumsq_kernel<<<RN_SUMSQ_WGS, 256, 0, st>>>(h->grads, n, h->sb.sqpart, h->sb.step, h->sb.sc, dec8(c.lr),
                                                    dec8(c.adam_beta1), dec8(c.adam_beta2));
  CK_LAUNCH("resnet_sumsq");
  RsAdamArgs a;
  a.params = h->params; a.grads = h->grads; a.m = h->exp_avg; a.v = h->exp_avg_sq; a.metrics = h->metrics;
  a.sqpart = h->sb.sqpart; a.sc = h->sb.sc; a.tpart = h->sb.tpart; a.step = h->sb.step;
  a.n = n; a.B = c.batch_size; a.T = c.rollout_length;
  a.b1 = dec8(c.adam_beta1); a.b2 = dec8(c.adam_beta2);
  a.eps = c.adam_eps; a.max_norm = c.max_grad_norm; a.ent_coef = c.entropy_coeff;
  resnet_adam_kernel<<<cdiv(nv + (flat_tail(h->cfg.num_actions) ? 1 : 0), 256), 256, 0, st>>>(a);
  CK_LAUNCH("resnet_adam");
  if (int r = RN_BY_TYPE(h, launch_pack, h, st)) return r;
  h->trained_n = 0;  // what the last resnet_forward_train saved belongs to the parameters before the update
  return 0;
}

}  // namespace

extern "C" {

int resnet_abi_version(void) { return RESNET_ABI_VERSION; }
const char* resnet_last_error(void) { return impala_last_error(); }

int resnet_config_default(resnet_config* cfg) {
  if (!cfg) return fail(IMPALA_E_INVALID, "null config");
  *cfg = resnet_config{128, RESNET_MAX_ACTIONS, IMPALA_DTYPE_F32, 0, 0, IMPALA_DTYPE_F32};
  return 0;
}

size_t resnet_param_count(int A) { return flat_total(A); }

int resnet_create(const resnet_config* cfg, int device, resnet_actor** out) {
  if (!cfg || !out) return fail(IMPALA_E_INVALID, "null pointer");
  if (cfg->batch_size < 1) return fail(IMPALA_E_INVALID, "batch_size must be >= 1");
  if (cfg->num_actions < 1 || cfg->num_actions > RESNET_MAX_ACTIONS)
    return fail(IMPALA_E_INVALID, "num_actions must be in [1, 15]");
  if (cfg->dtype != IMPALA_DTYPE_F32 && cfg->dtype != IMPALA_DTYPE_BF16) return fail(IMPALA_E_INVALID, "unknown dtype");
  if (cfg->debug != 0 && cfg->debug != 1) return fail(IMPALA_E_INVALID, "debug must be 0 or 1");
  if (cfg->train != 0 && cfg->train != 1) return fail(IMPALA_E_INVALID, "train must be 0 or 1");
  if (cfg->train_dtype != IMPALA_DTYPE_F32 && cfg->train_dtype != IMPALA_DTYPE_BF16)
    return fail(IMPALA_E_INVALID, "unknown train_dtype");
  if (cfg->train && cfg->train_dtype != cfg->dtype)
    return fail(IMPALA_E_INVALID, "train = 1 needs train_dtype == dtype: resnet_forward_train is resnet_forward, the same bits");
  CK(hipSetDevice(device));
  int cu = 0;
  CK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device));
  resnet_actor* h = new (std::nothrow) resnet_actor();
  if (!h) return fail(IMPALA_E_INVALID, "out of host memory");
  h->cfg = *cfg;
  h->device = device;
  h->n_cu = cu > 0 ? cu : 1;
  h->wg_groups = resnet_wg_groups(cfg->batch_size, h->n_cu);
  const hipError_t e = hipMalloc((void**)&h->ws, resnet_carve(*h, *cfg, h->n_cu, Arena{}));
  if (e != hipSuccess) {
    delete h;
    return fail((int)e, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  resnet_carve(*h, *cfg, h->n_cu, Arena{h->ws});
  *out = h;
  return 0;
}

int resnet_destroy(resnet_actor* h) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(h->ws);
  (void)hipFree(h->step_ws);
  delete h;
  return 0;
}

int resnet_bind_params(resnet_actor* h, const float* flat) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!flat) return fail(IMPALA_E_INVALID, "null pointer");
  if (((uintptr_t)flat & 15) != 0) return fail(IMPALA_E_INVALID, "the flat buffer must be 16-byte aligned");
  h->flat = flat;
  h->packed = false;
  return 0;
}

int resnet_refresh_weights(resnet_actor* h, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->flat) return fail(IMPALA_E_STATE, "resnet_bind_params not called");
  CK(hipSetDevice(h->device));
  const int r = RN_BY_TYPE(h, launch_pack, h, (hipStream_t)stream);
  if (r) return r;
  h->packed = true;
  h->trained_n = 0;
  return 0;
}

// resnet_forward and, with `train`, resnet_forward_train.  (Here, behind resnet_refresh_weights, and the
// TRAIN launch named last: the kernels lie in the code object in the order the templates are first used.)
static int forward_entry(resnet_actor* h, const uint8_t* obs, int n, float* logits, float* values, void* stream, bool train) {
  if (int r = check_ready(h, obs, n)) return r;
  if (!logits || !values) return fail(IMPALA_E_INVALID, "null pointer");
  if (train && !h->cfg.train) return fail(IMPALA_E_INVALID, "resnet_forward_train needs a handle created with train = 1");
  CK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (int r = !train                                ? RN_BY_TYPE(h, launch_forward, h, obs, n, st)
              : h->cfg.dtype == IMPALA_DTYPE_BF16 ? launch_forward<__bf16, true>(h, obs, n, st)
                                                  : launch_forward<float, true>(h, obs, n, st))
    return r;
  split_heads_kernel<<<cdiv((long)n * HEADS, 256), 256, 0, st>>>(h->heads, n, h->cfg.num_actions, logits, values);
  CK_LAUNCH("split_heads");
  if (train) h->trained_n = n;
  return 0;
}

int resnet_forward(resnet_actor* h, const uint8_t* obs, int n, float* logits, float* values, void* stream) {
  return forward_entry(h, obs, n, logits, values, stream, false);
}

int resnet_forward_train(resnet_actor* h, const uint8_t* obs, int n, float* logits, float* values, void* stream) {
  return forward_entry(h, obs, n, logits, values, stream, true);
}

int resnet_backward(resnet_actor* h, const uint8_t* obs, int n, const float* dlogits, const float* dvalues,
                    float* grad_flat, int accumulate, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->cfg.train) return fail(IMPALA_E_INVALID, "resnet_backward needs a handle created with train = 1");
  if (h->trained_n == 0)
    return fail(IMPALA_E_INVALID, "resnet_backward needs a resnet_forward_train since the last refresh or forward");
  if (n != h->trained_n) return fail(IMPALA_E_INVALID, "n differs from the last resnet_forward_train's");
  if (int r = check_ready(h, obs, n)) return r;
  if (!dlogits || !dvalues || !grad_flat) return fail(IMPALA_E_INVALID, "null pointer");
  if (accumulate != 0 && accumulate != 1) return fail(IMPALA_E_INVALID, "accumulate must be 0 or 1");
  CK(hipSetDevice(h->device));
  return RN_BY_TYPE(h, launch_backward, h, obs, n, dlogits, dvalues, grad_flat, accumulate, (hipStream_t)stream);
}

int resnet_act(resnet_actor* h, const uint8_t* obs, int n, const uint8_t* deterministic, int deterministic_all,
               uint64_t seed, uint64_t counter, int64_t* actions, float* logits, float* values, void* stream) {
  if (int r = check_ready(h, obs, n)) return r;
  if (!actions || !logits || !values) return fail(IMPALA_E_INVALID, "null pointer");
  CK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (int r = RN_BY_TYPE(h, launch_forward, h, obs, n, st)) return r;
  act_heads_kernel<<<cdiv(n, 256), 256, 0, st>>>(h->heads, n, h->cfg.num_actions, deterministic, deterministic_all,
                                                 seed, counter, actions, logits, values);
  CK_LAUNCH("act_heads");
  return 0;
}

int resnet_step_config_default(resnet_step_config* cfg) {
  if (!cfg) return fail(IMPALA_E_INVALID, "null config");
  *cfg = resnet_step_config{8, 20, 1e-4f, 0.9f, 0.999f, 1e-5f, 0.5f, 0.01f, 1.f, 1.f, 1.f, IMPALA_VTRACE_SG_ADVANTAGE};
  return 0;
}

int resnet_step_init(resnet_actor* h, const resnet_step_config* cfg) {
  if (!cfg) return fail(IMPALA_E_INVALID, "null config");
  if (cfg->rollout_length < 2 || cfg->rollout_length > 64) return fail(IMPALA_E_INVALID, "rollout_length must be in [2, 64]");
  if (cfg->batch_size < 1) return fail(IMPALA_E_INVALID, "batch_size must be >= 1");
  if (cfg->vtrace_grad_mode < IMPALA_VTRACE_SG_ADVANTAGE || cfg->vtrace_grad_mode > IMPALA_VTRACE_SG_NONE)
    return fail(IMPALA_E_INVALID, "unknown vtrace_grad_mode");
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->cfg.train) return fail(IMPALA_E_INVALID, "the learner step needs a handle created with train = 1");
  if ((long long)cfg->batch_size * cfg->rollout_length > h->cfg.batch_size)
    return fail(IMPALA_E_INVALID, "batch_size * rollout_length exceeds the handle's batch_size");
  CK(hipSetDevice(h->device));
  if (h->step_ws) {
    CK(hipDeviceSynchronize());
    CK(hipFree(h->step_ws));
    h->step_ws = nullptr;
    h->step_on = false;
  }
  const int A = h->cfg.num_actions;
  CK(hipMalloc((void**)&h->step_ws, resnet_step_carve(h->sb, cfg->batch_size, cfg->rollout_length, A, Arena{})));
  resnet_step_carve(h->sb, cfg->batch_size, cfg->rollout_length, A, Arena{h->step_ws});
  const int64_t zero = 0;
  CK(hipMemcpy(h->sb.step, &zero, 8, hipMemcpyHostToDevice));
  h->sc = *cfg;
  h->step_on = true;
  return 0;
}

int resnet_bind_state(resnet_actor* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                      float* metrics, void*) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->cfg.train) return fail(IMPALA_E_INVALID, "the learner step needs a handle created with train = 1");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !metrics) return fail(IMPALA_E_INVALID, "null pointer");
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)
    return fail(IMPALA_E_INVALID, "the flat buffers must be 16-byte aligned");
  if (params != h->flat) {
    h->flat = params;
    h->packed = false;
  }
  h->params = params; h->grads = grads; h->exp_avg = exp_avg; h->exp_avg_sq = exp_avg_sq; h->metrics = metrics;
  return 0;
}

int resnet_set_step(resnet_actor* h, int64_t step, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->step_on) return fail(IMPALA_E_STATE, "resnet_step_init not called");
  if (step < 0) return fail(IMPALA_E_INVALID, "step must be >= 0");
  CK(hipSetDevice(h->device));
  // (the source is read before the call returns: pageable host memory)
  CK(hipMemcpyAsync(h->sb.step, &step, 8, hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}

int resnet_set_debug_vtrace(resnet_actor* h, float* out) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  h->vt_dbg = out;
  return 0;
}

int resnet_loss_head(resnet_actor* h, const impala_batch* batch, void* stream) {
  if (int r = check_step(h, batch, true)) return r;
  if (h->trained_n != h->sc.batch_size * h->sc.rollout_length)
    return fail(IMPALA_E_STATE, "resnet_loss_head needs a resnet_forward_train of batch_size * rollout_length frames");
  CK(hipSetDevice(h->device));
  return launch_loss_head(h, batch, (hipStream_t)stream);
}

int resnet_compute_grads(resnet_actor* h, const impala_batch* batch, void* stream) {
  if (int r = check_step(h, batch, true)) return r;
  CK(hipSetDevice(h->device));
  return launch_compute_grads(h, batch, (hipStream_t)stream);
}

int resnet_apply_update(resnet_actor* h, void* stream) {
  if (int r = check_step(h, nullptr, false)) return r;
  CK(hipSetDevice(h->device));
  return launch_apply_update(h, (hipStream_t)stream);
}

int resnet_train_step(resnet_actor* h, const impala_batch* batch, void* stream) {
  if (int r = check_step(h, batch, true)) return r;
  CK(hipSetDevice(h->device));
  if (int r = launch_compute_grads(h, batch, (hipStream_t)stream)) return r;
  return launch_apply_update(h, (hipStream_t)stream);
}

int resnet_debug_read(resnet_actor* h, int which, void* dst, size_t bytes, void* stream) {
  if (!h) return fail(IMPALA_E_INVALID, "null handle");
  if (!h->cfg.debug && !h->cfg.train)
    return fail(IMPALA_E_INVALID, "resnet_debug_read needs a handle created with debug = 1 or train = 1");
  if (!dst) return fail(IMPALA_E_INVALID, "null pointer");
  const size_t es = elt(h), B = (size_t)h->cfg.batch_size;
  const char* src;
  size_t cap;
  if (which >= 0 && which < RESNET_DBG_STAGES) {
    src = (const char*)h->stages + stage_at((int)B, which, 0) * es;
    cap = B * dbg_size(which) * es;
  } else if (which == RESNET_DBG_Y) {
    src = (const char*)h->y; cap = B * RN_FEAT * es;
  } else if (which == RESNET_DBG_H) {
    src = (const char*)h->h; cap = B * RN_HID * es;
  } else if (which == RESNET_DBG_HEADS) {
    src = (const char*)h->heads; cap = B * HEADS * 4;
  } else if (which >= RESNET_DBG_GRAD0 && which <= RESNET_DBG_PART && !h->cfg.train) {
    return fail(IMPALA_E_INVALID, "the backward's tensors need a handle created with train = 1");
  } else if (which >= RESNET_DBG_GRAD0 && which < RESNET_DBG_GRAD0 + RN_CONVS) {
    src = (const char*)h->gws + stage_at((int)B, which - RESNET_DBG_GRAD0, 0) * es;
    cap = B * dbg_size(which - RESNET_DBG_GRAD0) * es;
  } else if (which == RESNET_DBG_GY) {
    src = (const char*)h->gy; cap = B * RN_FEAT * 4;
  } else if (which == RESNET_DBG_GZ) {
    src = (const char*)h->gz; cap = B * RN_HID * 4;
  } else if (which == RESNET_DBG_AMAX) {
    src = (const char*)h->amax; cap = B * RN_AMAX_FRAME;
  } else if (which == RESNET_DBG_LNSTAT) {
    src = (const char*)h->lnstat; cap = B * 2 * 4;
  } else if (which == RESNET_DBG_PART) {
    src = (const char*)h->part; cap = (size_t)RN_KSPLIT * B * RN_HID * 4;
  } else if (which >= RESNET_DBG_DLOGITS && which <= RESNET_DBG_TPART && !h->step_on) {
    return fail(IMPALA_E_STATE, "the step's tensors need a resnet_step_init");
  } else if (which == RESNET_DBG_DLOGITS) {
    src = (const char*)h->sb.dl; cap = (size_t)h->sc.batch_size * h->sc.rollout_length * h->cfg.num_actions * 4;
  } else if (which == RESNET_DBG_DVALUES) {
    src = (const char*)h->sb.dv; cap = (size_t)h->sc.batch_size * h->sc.rollout_length * 4;
  } else if (which == RESNET_DBG_TPART) {
    src = (const char*)h->sb.tpart; cap = (size_t)h->sc.batch_size * RN_TPART * 4;
  } else {
    return fail(IMPALA_E_INVALID, "unknown debug tensor");
  }
  if (bytes == 0 || bytes > cap) return fail(IMPALA_E_INVALID, "bytes must be in (0, batch_size frames]");
  CK(hipSetDevice(h->device));
  CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
