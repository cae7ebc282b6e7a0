// Operand definitions plugged into gemm_rc / gemm_tile / gemm_wg for each layer of the step.
// Output-side ops of gemm_tile split their epilogue into epi(r, c) -- the epilogue's own global
// reads (bias, ReLU mask), issued at the start of the tile so they land under the K loop -- and
// store(r, c, v, e).
// Activations are channels-last (pixel-major, channel-contiguous); frame n = b*T + t
// (batch-major flatten of agents/impala/learning.py:143).
#pragma once
#include "conv1.h"
#include "gemm.h"
#include "lnorm.h"
#include "net.h"

using namespace net;

// conv3: rows oc (64), cols (n, oh, ow) in N*16, k = (kh*3+kw)*64 + ci over act2.
// act3 row n is the flattened feature vector in (p*64 + c) order.
template <typename T> struct Conv3Fwd {
  static constexpr bool A_KMAJOR = false;
  static constexpr bool TILE_EPI = false;
  static constexpr int K = K3;
  int C;
  const T* w;
  const float* b;
  const T* x;
  T* out;
  struct ColCtx { const T* p; };
  DEV ColCtx col_ctx(int c) const {
    const int n = c / P3, p = c - n * P3, oh = p / H3, ow = p - oh * H3;
    return ColCtx{x + ((size_t)(n * H2 + oh) * H2 + ow) * OC2};
  }
  DEV const T* a_row(int r, int) const { return w + r * K; }
  DEV typename Frag<T>::vec load_b(const ColCtx& cc, int k) const {
    const int tap = k >> 6, ci = k & 63, kh = tap / 3, kw = tap - kh * 3;
    return Frag<T>::load(cc.p + (kh * H2 + kw) * OC2 + ci);
  }
  struct Epi { float b[4]; };
  DEV Epi epi(int r, int) const { return Epi{{b[r], b[r + 1], b[r + 2], b[r + 3]}}; }
  DEV void store(int r, int c, float v[4], const Epi& e) const {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fmaxf(v[i] + e.b[i], 0.f);
    store4(out + (size_t)c * OC3 + r, o);
  }
};

// projection Linear(1024 -> HID) + exact GELU (models/models.py:67-68).
// rows o (HID), cols frame n, k = p*64 + c over the LayerNorm output y.
template <typename T, int HID> struct FcFwd {
  static constexpr bool A_KMAJOR = false;
  static constexpr bool TILE_EPI = false;
  static constexpr int K = FLAT;
  int C;
  const T* w;
  const float* b;
  const T* y;
  float* zg;  // gelu'(pre-activation), fp32: the GELU backward's factor (head_step phase 3)
  T* h;
  struct ColCtx { const T* p; };
  DEV ColCtx col_ctx(int c) const { return ColCtx{y + (size_t)c * YLD}; }
  DEV const T* a_row(int r, int) const { return w + r * K; }
  DEV typename Frag<T>::vec load_b(const ColCtx& cc, int k) const { return Frag<T>::load(cc.p + k); }
  struct Epi { float b[4]; };
  DEV Epi epi(int r, int) const { return Epi{{b[r], b[r + 1], b[r + 2], b[r + 3]}}; }
  DEV void store(int r, int c, float v[4], const Epi& e) const {
    float gg[4], hh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gelu_fwd_grad(v[i] + e.b[i], hh[i], gg[i]);
    store4(zg + (size_t)c * HID + r, gg);
    store4(h + (size_t)c * HID + r, hh);
  }
};

// actor ‖ critic heads fused into one 16-row GEMM (models/models.py:69-70, 76).
template <typename T, int HID> struct HeadsFwd {
  static constexpr bool A_KMAJOR = false;
  static constexpr bool TILE_EPI = false;
  static constexpr int K = HID;
  int C;
  const T* w;
  const float* b;
  const T* h;
  float* out;  // [n][16]: logits 0..A-1, value at 15
  struct ColCtx { const T* p; };
  DEV ColCtx col_ctx(int c) const { return ColCtx{h + (size_t)c * HID}; }
  DEV const T* a_row(int r, int) const { return w + r * K; }
  DEV typename Frag<T>::vec load_b(const ColCtx& cc, int k) const { return Frag<T>::load(cc.p + k); }
  DEV void store(int r, int c, float v[4]) const {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = v[i] + b[r + i];
    store4(out + (size_t)c * HEADS + r, o);
  }
};

// conv3 + ReLU + LayerNorm(1024) fused (models/common.py:117-119, models/models.py:66):
// a 64(oc) x 64(pixel) tile holds 4 whole frames; wave w normalises frame w of the tile.
// Writes act3 (post-ReLU, kept for the mask and the LN backward), y = LN(act3), mean/rstd.
template <typename T> struct Conv3LnFwd : Conv3Fwd<T> {
  static constexpr bool TILE_EPI = true;
  const float* gam;  // permuted to p*64 + c
  const float* bet;
  T* y;
  float* stats;
  int frames_per_tile;  // tile width / 16 (<= 4: one wave per frame)
  typedef LnLane EpiConst;  // loaded once per workgroup (gemm_tile)
  DEV EpiConst epi_const(int tid) const { return ln_lane_consts(tid & 63, this->b, gam, bet); }
  DEV void tile_epilogue(const float* et, int ldt, int, int cc0, int tid,
                         const EpiConst& k) const {
    const int lane = tid & 63, wave = tid >> 6;
    const int frame = cc0 / P3 + wave;
    if (wave >= frames_per_tile || (frame + 1) * P3 > this->C) return;
    ln_frame_epilogue<T>(et + wave * P3 * ldt, ldt, frame, lane, k, this->out, y, stats);
  }
};

// dy = dz . Wfc  (rows j in p*64+c order, cols frame), fp32 out for the LayerNorm backward.
// A[j][o] = wfc[o][j]: read k-major from the forward weight (no transposed copy).
template <typename T, int HID> struct FcDgrad {
  static constexpr bool A_KMAJOR = true;
  static constexpr bool TILE_EPI = false;
  static constexpr int K = HID;
  int C;
  const T* w;   // wfc [HID][1024]
  const T* dz;
  float* dy;
  struct ColCtx { const T* p; };
  DEV ColCtx col_ctx(int c) const { return ColCtx{dz + (size_t)c * HID}; }
  DEV const T* a_row(int, int) const { return nullptr; }
  DEV const T* a_kptr(int k, int r, int) const { return w + (size_t)k * FLAT + r; }
  DEV typename Frag<T>::vec load_b(const ColCtx& cc, int k) const { return Frag<T>::load(cc.p + k); }
  struct Epi {};
  DEV Epi epi(int, int) const { return Epi{}; }
  DEV void store(int r, int c, float v[4], const Epi&) const { store4(dy + (size_t)c * FLAT + r, v); }
};

template <typename T, int HID> struct FcWgrad {  // dWfc[o][j] = sum_n dz[n][o] y[n][j]
  static constexpr int R = HID, C = FLAT;
  int M;
  float out_scale = 1.f;
  const T* x;  // dz
  int x_ld = HID;
  const T* y;
  // Y gather as element offsets from y (buffer loads: out-of-range rows read as zero)
  DEV int y_roff(int m) const { return m * YLD; }
  DEV int y_coff(int c) const { return c; }
  DEV int y_bytes() const { return M * YLD * (int)sizeof(T); }
  DEV const T* ybase() const { return y; }
  // gemm_wg_body: elements the Y row offset advances for a stride of D rows, where that is a
  // constant (> 0); 0 where it is not (the op then has a row cursor, YCUR)
  template <int D> static constexpr int y_stride() { return D * YLD; }
};

template <typename T> struct Conv3Wgrad {  // m = (n, oy, ox) in N*16; c = (kh*3+kw)*64 + ci
  static constexpr int R = OC3, C = K3;
  int M;
  float out_scale = 1.f;
  const T* x;  // dact3
  int x_ld = OC3;
  const T* in;  // act2
  DEV int y_roff(int m) const {  // top-left input pixel of the 3x3 patch
    const int n = m / P3, p = m - n * P3, oy = p / H3, ox = p - oy * H3;
    return ((n * H2 + oy) * H2 + ox) * OC2;
  }
  DEV int y_coff(int c) const {
    const int tap = c >> 6, ci = c & 63, kh = tap / 3, kw = tap - kh * 3;
    return (kh * H2 + kw) * OC2 + ci;
  }
  DEV int y_bytes() const { return (M / P3) * (H2 * H2 * OC2) * (int)sizeof(T); }
  DEV const T* ybase() const { return in; }
  // a stride of whole frames keeps the pixel and moves the frame: the row offset advances by a
  // constant wherever the row starts (the chunk strides in use, 32 and 64 rows, are 2 and 4
  // frames), so y_roff's divisions run once per thread, in the prologue
  template <int D> static constexpr int y_stride() {
    static_assert(D % P3 == 0, "conv3 weight gradient: the chunk stride must be whole frames");
    return (D / P3) * (H2 * H2 * OC2);
  }
};
template <typename T> struct Conv2Wgrad {  // m = (n, oy, ox) in N*36; c = (kh*4+kw)*32 + ci
  static constexpr int R = OC2, C = K2;
  int M;
  float out_scale = 1.f;
  const T* x;  // dact2
  int x_ld = OC2;
  const T* in;  // act1
  DEV int y_roff(int m) const {
    const int n = m / P2, p = m - n * P2, oy = p / H2, ox = p - oy * H2;
    return ((n * H1 + ST2 * oy) * H1 + ST2 * ox) * OC1;
  }
  DEV int y_coff(int c) const {
    const int tap = c >> 5, ci = c & 31, kh = tap >> 2, kw = tap & 3;
    return (kh * H1 + kw) * OC1 + ci;
  }
  DEV int y_bytes() const { return (M / P2) * (H1 * H1 * OC1) * (int)sizeof(T); }
  DEV const T* ybase() const { return in; }
  // 36 pixels per frame: no chunk stride is whole frames, so each staged row keeps a cursor
  // (gemm_wg_body YCUR): the running byte offset (column included) with the pixel index p and
  // its column ox.  A stride of D = (dn, dy, dx) in (frame, row, column) adds the constant
  // offset of (dn, dy, dx) plus one correction where ox wraps (a carry into the row) and one
  // where p wraps (a carry into the frame): p + D % 36 >= 36 exactly when the row carries,
  // whatever the column did.  Two compares and selects per advance; y_roff's divisions run
  // once per thread, in ycur().  ycur_peek gives the same delta for a row D further down
  // without moving the cursor (a thread's other staging rows of the same chunk).
  template <int D> static constexpr int y_stride() { return 0; }
  static constexpr bool YCUR = true;
  struct YCur { int off, p, ox; };
  DEV YCur ycur(int m, int c) const {
    const int n = m / P2, p = m - n * P2;
    return YCur{(y_roff(m) + y_coff(c)) * (int)sizeof(T), p, p % H2};
  }
  // byte offset of the row D (a constant once inlined) after the cursor's, less the cursor's
  DEV int ycur_peek(const YCur& c, int D) const {
    constexpr int ES = (int)sizeof(T);
    constexpr int RX = ST2 * OC1 * ES, RY = ST2 * H1 * OC1 * ES, FR = H1 * H1 * OC1 * ES;
    const int dn = D / P2, r = D % P2, dy = r / H2, dx = r % H2;
    return dn * FR + dy * RY + dx * RX + (c.ox + dx >= H2 ? RY - H2 * RX : 0) +
           (c.p + r >= P2 ? FR - H2 * RY : 0);
  }
  template <int D> DEV void ycur_adv(YCur& c) const {
    constexpr int r = D % P2, dx = r % H2;
    c.off += ycur_peek(c, D);
    c.ox += dx;
    c.ox -= c.ox >= H2 ? H2 : 0;
    c.p += r;
    c.p -= c.p >= P2 ? P2 : 0;
  }
};

// FC forward tiles (gemm_tile<FcFwd>: BR hidden units x BC frames, K chunk BK, NW waves).
// bf16: 32 x 32 tiles on 4 waves, 320 workgroups at N = 1280 (5.9 vs 6.7 us for 64 x 32).
// fp32: 16 x 80 tiles whose 8 waves split each chunk's k-steps (gemm_tile_body KW; K chunk 128 =
// one k-step per wave per chunk): 256 tiles at N = 1280, one per CU, two waves per SIMD (the
// 32 x 32 tiles put two on 64 CUs, whose MFMA time bounds the kernel; 32 x 48 on 4 / 8 waves:
// 12.3 / 11.7 us, 16 x 80 on 8: 11.4 us; profiles/r05kw), and two K chunks held in registers
// ahead of the MFMAs (PF 1: 13.97 us, 2: 13.40, on the 32 x 32 tiles; a second accumulator
// chain per fragment lost at either, 14.20 / 13.67-13.69; profiles/r04v).  PF keeps the
// summation order, so the output bits do not depend on it.
template <typename T> struct FcFwdCfg {
  static constexpr bool KW = sizeof(T) == 4;
  static constexpr int BR = KW ? 16 : 32, BC = KW ? 80 : 32, BK = KW ? 128 : 256;
  static constexpr int NW = KW ? 8 : 4, PF = KW ? 2 : 1;
};

// FC weight gradient and FC input gradient in ONE launch.  Both read only dz (with y / Wfc), so
// they are independent: blocks [0, gx*gy*gz) run the split weight-gradient body (gemm_wg, G
// 4-wave groups) and the rest run the input-gradient tiles (gemm_tile with 4*G waves: 64 x 64
// tiles for G = 1, 128 x 64 for G = 2).  The weight gradient's 96 workgroups leave most CUs
// idle for its ~7 us; the dgrad tiles fill them instead of running after it.  Same per-tile
// arithmetic as the two separate kernels (same tile shapes for the weight gradient).
// dgrad tiles DR (flat) x DC (frames) on DWR x DWC waves, weight-gradient tiles 64 x WBC.
// fp32: 64 x 80 dgrad tiles (256 at N = 1280, 78 KB of LDS) beside 256 weight-gradient
// workgroups of 64 x 128 (the same 8 splits, 51 KB): 512 workgroups of about the same MFMA
// work, two per CU -- two waves per SIMD (profiles/r05kw: 64 x 64 dgrad tiles beside 64 x 256
// weight-gradient tiles ran ~1.75 rounds at one workgroup per CU, 20.6 us; 128 x 80 one round
// at one per CU, 19.7; this 16.7)
// bf16 (G = 2, 8 waves): 64 x 64 dgrad tiles on 2 x 4 waves (320) beside 64 x 128 weight-gradient
// workgroups (192 at the same 6 splits), 78 KB: 512 workgroups, two per CU (8.4 -> 6.8 us)
// With the weight-gradient loop's staging offsets advanced instead of recomputed (gemm.h):
// fp32 17.89 -> 17.49 us, bf16 7.31 -> 7.23 (profiles/wgloop, parent -> this tree)
template <typename T, int G, int HID> struct FcBwdCfg {
  static constexpr int DR = 64, DWR = G == 2 ? 2 : 4;
  static constexpr int DC = G == 2 ? 64 : 80, DWC = G == 2 ? 4 : 1;
  static constexpr int DBK = sizeof(T) == 2 ? 128 : 64;
  static constexpr int WBC = 128;
  static constexpr int SW = gemm_wg_smem<T, 64, WBC, 32, G>();
  static constexpr int SD = gemm_tile_smem<T, DR, DC, DBK, DWR, DWC, FcDgrad<T, HID>>();
  static constexpr int SMEM = SW > SD ? SW : SD;
};
template <typename T, int G, int HID>
__global__ __launch_bounds__(256 * G) void fc_bwd_kernel(const FcWgrad<T, HID> ow, float* __restrict__ slab,
                                                         float* __restrict__ slab_bias, int mps,
                                                         int gx, int gy, int gz,
                                                         const FcDgrad<T, HID> od, int n_rtiles) {
  using C = FcBwdCfg<T, G, HID>;
  __shared__ __attribute__((aligned(16))) T smem[C::SMEM];
  const int nw = gx * gy * gz;
  if ((int)blockIdx.x < nw)
    gemm_wg_body<T, 64, C::WBC, 1, 4, 32, G, FcWgrad<T, HID>>(ow, slab, slab_bias, mps, (int)blockIdx.x,
                                                         gx, gy, gz, smem);
  else
    gemm_tile_body<T, C::DR, C::DC, C::DBK, C::DWR, C::DWC, FcDgrad<T, HID>>(od, n_rtiles, (int)blockIdx.x - nw,
                                                                (int)gridDim.x - nw, smem);
}

// conv3 and conv2 weight gradients in ONE launch (both depend only on the LayerNorm backward's
// outputs): blocks [0, n3) run the conv3 split weight-gradient body, the rest conv2's -- the
// same tiles, splits and group order as the two separate launches (bitwise-equal slabs), with
// one kernel boundary fewer and conv3's tail overlapping conv2's ramp.
// conv2 weight-gradient tile of the merged launch: fp32 64 x 64 on 2 x 2 waves -- 512 workgroups
// of conv3's size (64 splits as before, so the same slab and per-element sums), three per CU
// beside conv3's 252, instead of 256 64 x 128 workgroups of twice conv3's MFMA work; bf16 64 x 128
// Per 32-row chunk a wave issues 32 (fp32) MFMAs and, beside them, 16 (conv2) or 4 (conv3) VALU
// of staging addresses (40 and 44 before the offsets were advanced instead of recomputed):
// fp32 51.77 -> 47.90 us, bf16 15.04 -> 14.07 (profiles/wgloop, parent -> this tree)
template <typename T> struct Wg2Tile {
  static constexpr int BC = sizeof(T) == 4 ? 64 : 128, WR = sizeof(T) == 4 ? 2 : 1, WC = 4 / WR;
};
template <typename T, int G> struct Wg23Cfg {
  static constexpr int S3 = gemm_wg_smem<T, 64, 64, 32, G>(), S2 = gemm_wg_smem<T, 64, Wg2Tile<T>::BC, 32, G>();
  static constexpr int SMEM = S3 > S2 ? S3 : S2;
};
template <typename T, int G>
__global__ __launch_bounds__(256 * G) void wgrad23_kernel(const Conv3Wgrad<T> o3, float* __restrict__ s_w3,
                                                          float* __restrict__ s_b3, int mps3, int g3x, int g3z,
                                                          const Conv2Wgrad<T> o2, float* __restrict__ s_w2,
                                                          float* __restrict__ s_b2, int mps2, int g2x, int g2z) {
  __shared__ __attribute__((aligned(16))) T smem[Wg23Cfg<T, G>::SMEM];
  const int n3 = g3x * g3z;
  if ((int)blockIdx.x < n3)
    gemm_wg_body<T, 64, 64, 2, 2, 32, G, Conv3Wgrad<T>>(o3, s_w3, s_b3, mps3, (int)blockIdx.x, g3x, 1,
                                                        g3z, smem);
  else
    gemm_wg_body<T, 64, Wg2Tile<T>::BC, Wg2Tile<T>::WR, Wg2Tile<T>::WC, 32, G, Conv2Wgrad<T>>(
        o2, s_w2, s_b2, mps2, (int)blockIdx.x - n3, g2x, 1, g2z, smem);
}
