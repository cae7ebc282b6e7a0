// The backward pass of the IMPALA ResNet actor-critic, fp32 and bf16, included by
// resnet.hip inside its unnamed namespace, after the forward's helpers.  T is the compute type: the
// type of the saved stage tensors, of the data gradients' weights and of the gradient between the
// layers, in LDS and in HBM; every accumulation and the flat gradient are fp32.
//
// One resnet_backward of n frames, from what resnet_forward_train left in the handle:
//   resnet_head_bwd_kernel     one wave per frame: gz = GELU'(z) * (Wh^T dheads), z re-summed from the
//                              projection's K chunks in the forward's order
//   resnet_head_wgrad_kernel   d Wh, d bh, d bfc: one thread per element, the frames in order
//   resnet_fc_wgrad_kernel     d Wfc [256][2048] = gz^T y on the fp32 MFMAs, the contraction over frames
//   resnet_fc_dgrad_kernel     gy [n][2048] = gz Wfc on the fp32 MFMAs (Wfc packed transposed)
//   resnet_ln_affine_kernel    d gamma, d beta: one thread per feature, the frames in order
//   resnet_trunk_bwd_kernel    one frame per workgroup: LayerNorm and ReLU backward, then the data
//                              gradients of the 14 non-stem convolutions as pad-1 convolutions of
//                              the gradient with the flipped, Cin/Cout-swapped weights (the
//                              forward's conv_tiles), masks from the saved tensors in L2, the
//                              max-pools as gathers; the gradient at every convolution's output
//                              goes to HBM
//   resnet_wgrad_kernel        d W, d b of the 15 convolutions: workgroup (frame group, conv)
//   resnet_wgrad_bf16_kernel   holds the whole d W of its conv in accumulators over its frames;
//                              D[oc][tap, ci] = sum_pixel g[pixel][oc] relu(in)[pixel + tap][ci]
//   resnet_wreduce_kernel      the frame groups' partial d W, d b summed in order into the flat gradient
// The tail's arithmetic is fp32 in both modes: it reads h, y and x14 in T and converts on the read.
// No floating-point atomics: every sum over frames has one fixed order.
#pragma once

template <typename T> struct BwdArgs {
  int n, B;
  const T* wd[RN_CONVS];  // data-gradient weights of convs 1..14, fragment-major
  const float* vecs;
  const T* sav;          // the handle's stages, amax, lnstat as resnet_forward_train left them
  const uint8_t* amax;
  const float* lnstat;
  const float* gy;       // [n][2048], kernel order
  T* gws;                // the gradient at every conv's output (post-pool for 0, 5, 10), the stage tensors' layout
};

template <typename T> DEV const T* sav_at(const BwdArgs<T>& a, int id, int f) { return a.sav + stage_at(a.B, id, f); }
template <typename T> DEV T* gws_at(const BwdArgs<T>& a, int id, int f) { return a.gws + stage_at(a.B, id, f); }

// d heads of frame f, output o: the logits' cotangent, the value's at VCOL, 0 between
DEV float dhead(const float* __restrict__ dl, const float* __restrict__ dv, int A, int f, int o) {
  return o < A ? dl[(size_t)f * A + o] : o == VCOL ? dv[f] : 0.f;
}

// ---- the tail ----
__global__ __launch_bounds__(256) void resnet_head_bwd_kernel(const float* __restrict__ part, const float* __restrict__ vecs,
                                                              const float* __restrict__ dl, const float* __restrict__ dv,
                                                              float* __restrict__ gz, int n, int B, int A) {
  const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n) return;
  float dh[HEADS];
#pragma unroll
  for (int o = 0; o < HEADS; ++o) dh[o] = dhead(dl, dv, A, f, o);
#pragma unroll
  for (int i = 0; i < RN_HID / 64; ++i) {
    const int j = lane + 64 * i;
    float z = part[(size_t)f * RN_HID + j];  // (resnet_heads_kernel's sum, term for term)
#pragma unroll
    for (int ks = 1; ks < RN_KSPLIT; ++ks) z += part[((size_t)ks * B + f) * RN_HID + j];
    z += vecs[RV_BFC + j];
    float hh, gp;
    gelu_fwd_grad(z, hh, gp);
    float gh = 0.f;
#pragma unroll
    for (int o = 0; o < HEADS; ++o) gh = fmaf(vecs[RV_WH + o * RN_HID + j], dh[o], gh);
    gz[(size_t)f * RN_HID + j] = gh * gp;
  }
}

DEV void grad_out(float* __restrict__ g, int i, float v, int accumulate) { g[i] = accumulate ? g[i] + v : v; }

// block o < 16: d Wh[o][:] and d bh[o]; block 16: d bfc
template <typename T>
__global__ __launch_bounds__(256) void resnet_head_wgrad_kernel(const T* __restrict__ h, const float* __restrict__ gz,
                                                                const float* __restrict__ dl, const float* __restrict__ dv,
                                                                float* __restrict__ grad, const GradOff go, int n, int A,
                                                                int accumulate) {
  const int o = blockIdx.x, j = threadIdx.x;
  if (o == HEADS) {
    float s = 0.f;
    for (int f = 0; f < n; ++f) s += gz[(size_t)f * RN_HID + j];
    grad_out(grad, go.bfc + j, s, accumulate);
    return;
  }
  if (o >= A && o != VCOL) return;
  float s = 0.f, sb = 0.f;
  for (int f = 0; f < n; ++f) {
    const float d = dhead(dl, dv, A, f, o);
    s = fmaf(d, (float)h[(size_t)f * RN_HID + j], s);
    sb += d;
  }
  grad_out(grad, (o < A ? go.wa + o * RN_HID : go.wc) + j, s, accumulate);
  if (j == 0) grad_out(grad, o < A ? go.ba + o : go.bc, sb, accumulate);
}

// d Wfc[o][k'] = sum_f gz[f][o] y[f][k']: workgroup (o tile, 256 features), a wave 16 x 64 of it.  Both
// operands are read along the frames from L2: lane (col, grp) takes frames f0 + 4 e + grp, so a wave
// instruction reads four 64-byte runs (32-byte runs of a bf16 y, converted on the read).  Frames past n
// contribute zero.
template <typename T>
__global__ __launch_bounds__(256) void resnet_fc_wgrad_kernel(const float* __restrict__ gz, const T* __restrict__ y,
                                                              float* __restrict__ grad, int wfc_off, int n, int accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int ot = blockIdx.x & 15, k0 = (blockIdx.x >> 4) * 256 + wave * 64;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int f0 = 0; f0 < n; f0 += 16) {
    f32x4 av, bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f0 + 4 * e + grp, fc = min(f, n - 1);
      const float a = gz[(size_t)fc * RN_HID + ot * 16 + col];
      av[e] = f < n ? a : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j][e] = (float)y[(size_t)fc * RN_FEAT + k0 + 16 * j + col];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][e], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + 16 * j + col, canon = (k & 31) * 64 + (k >> 5);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      grad_out(grad, wfc_off + (ot * 16 + 4 * grp + q) * RN_FEAT + canon, acc[j][q], accumulate);
  }
}

// gy[f][k'] = sum_o gz[f][o] Wfc[o][k']: workgroup kt holds the 16 features' rows of Wfc^T as A fragments
// (wfct [128][16][64][4]: row k' = 16 kt + (lane & 15), k = o = 16 s + 4 (lane >> 4) + j), a wave the
// 16-frame tiles w, w + 4, ..
__global__ __launch_bounds__(256) void resnet_fc_dgrad_kernel(const float* __restrict__ gz, const float* __restrict__ wfct,
                                                              float* __restrict__ gy, int n) {
  constexpr int NKS = RN_HID / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int kt = blockIdx.x;
  f32x4 wf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) wf[s] = *reinterpret_cast<const f32x4*>(wfct + ((size_t)(kt * NKS + s) * 64 + lane) * 4);
  for (int r0 = wave * 16; r0 < n; r0 += 64) {
    const int fr = min(r0 + col, n - 1);
    const float* zr = gz + (size_t)fr * RN_HID + 4 * grp;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < NKS; s += 2) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(zr + s * 16), v1 = *reinterpret_cast<const f32x4*>(zr + (s + 1) * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s][e], v0[e], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s + 1][e], v1[e], acc[1], 0, 0, 0);
      }
    }
    if (r0 + col < n) *reinterpret_cast<f32x4*>(gy + (size_t)fr * RN_FEAT + kt * 16 + 4 * grp) = acc[0] + acc[1];
  }
}
// Wfc as the forward uses it (rounded to T), transposed
template <typename T>
__global__ __launch_bounds__(256) void resnet_pack_fct_kernel(const float* __restrict__ w, float* __restrict__ dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // < 2048 * 256
  const int j = e & 3, lane = (e >> 2) & 63, s = (e >> 8) & 15, kt = e >> 12;
  const int k = 16 * kt + (lane & 15), o = 16 * s + 4 * (lane >> 4) + j;
  dst[e] = (float)(T)w[(size_t)o * RN_FEAT + (k & 31) * 64 + (k >> 5)];
}
// data-gradient weights of a conv, canonical [COUT][CIN][3][3] -> fragment-major as the forward's with
// row ci and k = tap' * COUT + oc, tap' = 8 - tap: the gradient's convolution runs on conv_tiles.  K is
// padded to nks whole K-steps with zeros (bf16 at COUT = 16: 144 -> 160).
template <typename T>
__global__ __launch_bounds__(256) void resnet_pack_dgrad_kernel(const float* __restrict__ w, T* __restrict__ dst,
                                                                int cin, int cout, int nks, int total) {
  using F = Frag<T>;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = e % F::KPL, lane = (e / F::KPL) & 63, s = (e / (F::KPL * 64)) % nks, nt = e / (F::KPL * 64 * nks);
  const int ci = 16 * nt + (lane & 15), k = s * F::KSTEP + (lane >> 4) * F::KPL + j;
  const int tap = k / cout, oc = k % cout;
  dst[e] = (T)(tap < 9 ? w[((size_t)oc * cin + ci) * 9 + (8 - tap)] : 0.f);
}

// d gamma[k'] = sum_f gy xhat, d beta[k'] = sum_f gy, xhat from the saved x (stage tensor 14) and statistics
template <typename T>
__global__ __launch_bounds__(256) void resnet_ln_affine_kernel(const float* __restrict__ gy, const T* __restrict__ x14,
                                                               const float* __restrict__ lnstat, float* __restrict__ grad,
                                                               int lng, int lnb, int n, int accumulate) {
  const int k = blockIdx.x * 256 + threadIdx.x, canon = (k & 31) * 64 + (k >> 5);
  float sg = 0.f, sb = 0.f;
  for (int f = 0; f < n; ++f) {
    const float g = gy[(size_t)f * RN_FEAT + k];
    const float xh = (fmaxf((float)x14[(size_t)f * RN_FEAT + k], 0.f) - lnstat[2 * f]) * lnstat[2 * f + 1];
    sg = fmaf(g, xh, sg);
    sb += g;
  }
  grad_out(grad, lng + canon, sg, accumulate);
  grad_out(grad, lnb + canon, sb, accumulate);
}

// ---- the max-pools' backward as a gather.  Rows of the gradient at a pooled conv's output (HC x HC x C)
// from the gradient g [HO][HO][C] at the pool's output and the winning taps: pixel (r, cx) collects from
// the windows (oy, ox) with |r - 2 oy| <= 1, |cx - 2 ox| <= 1 whose byte names it, in a fixed order, in
// fp32, rounded to T once.
// HALO: rows r0 - 1 .. r0 + R as a halo tensor [R + 2][HC + 2][C], zero outside the image; else rows
// r0 .. r0 + R - 1 as [R][HC][C].
template <typename T, int HC, int C, int R, bool HALO>
DEV void pool_gather(const T* __restrict__ g, const uint8_t* __restrict__ am, T* __restrict__ dst, int r0) {
  constexpr int HO = HC / 2, NR = HALO ? R + 2 : R, W = HALO ? HC + 2 : HC, CV = C / 4, ITEMS = NR * W * CV;
  for (int i = threadIdx.x; i < ITEMS; i += RN_THREADS) {
    const int c0 = 4 * (i % CV), px = (i / CV) % W, j = i / (CV * W);
    const int r = r0 + j - (HALO ? 1 : 0), cx = px - (HALO ? 1 : 0);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < HC && cx >= 0 && cx < HC) {
#pragma unroll
      for (int ay = 0; ay < 2; ++ay)
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
          const int oy = (r + ay) >> 1, ox = (cx + ax) >> 1;
          if ((ay == 0 || (r & 1)) && (ax == 0 || (cx & 1)) && oy < HO && ox < HO) {
            const uint32_t tap = (uint32_t)((r - 2 * oy + 1) * 3 + (cx - 2 * ox + 1));
            const int at = (oy * HO + ox) * C + c0;
            const uint32_t win = *reinterpret_cast<const uint32_t*>(am + at);
            float gv[4];
            load4(g + at, gv);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (((win >> (8 * q)) & 255u) == tap) s[q] += gv[q];
          }
        }
    }
    store4(dst + (j * W + px) * C + c0, s);
  }
}

// [x > 0] of four saved values; bf16 by the sign bit of a nonzero value, as relu_v (no NaN in an activation)
DEV void pos4(const float* __restrict__ p, bool (&m)[4]) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] = v[q] > 0.f;
}
DEV void pos4(const __bf16* __restrict__ p, bool (&m)[4]) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  const s16x4 v = *reinterpret_cast<const s16x4*>(p);
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] = v[q] > 0;
}

// ---- epilogues of the gradient's convolutions: the mask from the saved tensor in L2, the result into
// the interior of an LDS halo tensor and to gws, rounded to T once
template <typename T, int H, int C> struct EpiMaskStore {  // gt = [t > 0] acc
  T* out;
  const T* sav;
  T* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const int at = (y * H + x) * C + c0;
    bool m[4];
    pos4(sav + at, m);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = m[q] ? acc[q] : 0.f;
    store4(out + ((y + 1) * (H + 2) + x + 1) * C + c0, v);
    store4(gout + at, v);
  }
};
template <typename T, int H, int C> struct EpiMaskAdd {  // g = T(fp32(g) + [x > 0] acc), in place (the convolution reads gt only)
  T* g;
  const T* sav;
  T* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const int at = (y * H + x) * C + c0;
    bool m[4];
    pos4(sav + at, m);
    T* p = g + ((y + 1) * (H + 2) + x + 1) * C + c0;
    float v[4];
    load4(p, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += m[q] ? acc[q] : 0.f;
    store4(p, v);
    store4(gout + at, v);
  }
};
template <typename T, int H, int C> struct EpiPlain {
  T* out;
  T* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const float v[4] = {acc[0], acc[1], acc[2], acc[3]};
    store4(out + ((y + 1) * (H + 2) + x + 1) * C + c0, v);
    store4(gout + (y * H + x) * C + c0, v);
  }
};

// output rows r0 .. r0 + R - 1 of a pad-1 convolution whose operand is a halo strip [R + 2][H + 2][CIN]
// (row 0 = image row r0 - 1)
template <typename T, int CIN, int COUT, int H, int R, class Epi>
DEV void conv_strip(const T* __restrict__ strip, const T* __restrict__ wpk, int r0, Epi epi) {
  typedef typename Frag<T>::vec V;
  constexpr int NKS = conv_nks<T, CIN>(), P = H + 2;
  const int grp = (threadIdx.x & 63) >> 4;
  int off[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) off[s] = tap_off<T, CIN, P>(s, grp);
  conv_tiles<T, NKS, COUT, H, R>(
      wpk, r0, [&](int y, int x, int s) { return *reinterpret_cast<const V*>(strip + ((y - r0) * P + x) * CIN + off[s]); },
      epi);
}

// the two residual blocks of a stage, backwards: g (the gradient at the stage's output, a halo tensor)
// becomes the gradient at the pool's output; gt is scratch with a zero halo.  P0: the stage's pooled conv.
template <typename T, int C, int H> DEV void res_blocks_bwd(T* g, T* gt, const BwdArgs<T>& a, int P0, int f) {
#pragma unroll
  for (int blk = 1; blk >= 0; --blk) {
    const int xin = P0 + 2 * blk, i0 = xin + 1, i1 = xin + 2;
    conv_lds<T, C, C, H, H, false>(g, a.wd[i1], 0, EpiMaskStore<T, H, C>{gt, sav_at(a, i0, f), gws_at(a, i0, f)});
    __syncthreads();
    conv_lds<T, C, C, H, H, false>(gt, a.wd[i0], 0, EpiMaskAdd<T, H, C>{g, sav_at(a, xin, f), gws_at(a, xin, f)});
    __syncthreads();
  }
}

// g and gt: two halo tensors of the stage's size.  fp32: 2 x 73,984 bytes at stage 1, one workgroup a CU;
// bf16: 2 x 36,992, two.
template <typename T> struct LdsBwd {
  static constexpr int S1 = Lds<T>::S1, S2 = Lds<T>::S2, S3 = Lds<T>::S3;
  static constexpr int G = 0, GT = S1, RED = 2 * S1, TOTAL = RED + 64 * 4;
  static_assert(10 * 34 * 32 * (int)sizeof(T) <= S1 && 18 * 18 * 32 * (int)sizeof(T) <= S1,
                "the pools' gradient strips live in gt's place");
  static_assert(TOTAL <= 160 * 1024, "the CU's LDS");
};

template <typename T> DEV void trunk_bwd(const BwdArgs<T>& a) {
  using L = LdsBwd<T>;
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T* const g = reinterpret_cast<T*>(lds + L::G);
  T* const gt = reinterpret_cast<T*>(lds + L::GT);
  float* const red = reinterpret_cast<float*>(lds + L::RED);
  for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
    const uint8_t* am = a.amax + (size_t)f * RN_AMAX_FRAME;
    // ---- LayerNorm and the final ReLU, backwards: thread -> pixel tid / 8, channels 4 (tid % 8) ..
    lds_zero(lds + L::G, L::S3);
    lds_zero(lds + L::GT, L::S3);
    __syncthreads();
    {
      const int p = tid >> 3, c0 = 4 * (tid & 7), k = p * 32 + c0;
      const float mean = a.lnstat[2 * f], rstd = a.lnstat[2 * f + 1];
      float x[4];
      load4(sav_at(a, 14, f) + k, x);
      const f32x4 gyv = *reinterpret_cast<const f32x4*>(a.gy + (size_t)f * RN_FEAT + k);
      const f32x4 gam = *reinterpret_cast<const f32x4*>(a.vecs + RV_LNG + k);
      f32x4 gg, xh;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        gg[q] = gyv[q] * gam[q];
        xh[q] = (fmaxf(x[q], 0.f) - mean) * rstd;
      }
      const float s1 = wave_sum((gg[0] + gg[1]) + (gg[2] + gg[3]));
      const float s2 = wave_sum((gg[0] * xh[0] + gg[1] * xh[1]) + (gg[2] * xh[2] + gg[3] * xh[3]));
      if (lane == 0) {
        red[wave] = s1;
        red[8 + wave] = s2;
      }
      __syncthreads();
      const float m1 = sum8(red) * (1.f / RN_FEAT), m2 = sum8(red + 8) * (1.f / RN_FEAT);
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = x[q] > 0.f ? rstd * (gg[q] - m1 - xh[q] * m2) : 0.f;
      store4(g + (((p >> 3) + 1) * 10 + (p & 7) + 1) * 32 + c0, v);
      store4(gws_at(a, 14, f) + k, v);
    }
    __syncthreads();
    res_blocks_bwd<T, 32, 8>(g, gt, a, 10, f);
    // ---- stage 3's pool and conv 10 (32 -> 32 at 16 x 16): the gathered gradient whole in gt's place
    lds_zero(lds + L::G, L::S2);
    pool_gather<T, 16, 32, 16, true>(gws_at(a, 10, f), am + amax_off(2), gt, 0);
    __syncthreads();
    conv_strip<T, 32, 32, 16, 16>(gt, a.wd[10], 0, EpiPlain<T, 16, 32>{g, gws_at(a, 9, f)});
    __syncthreads();
    lds_zero(lds + L::GT, L::S2);
    __syncthreads();
    res_blocks_bwd<T, 32, 16>(g, gt, a, 5, f);
    // ---- stage 2's pool and conv 5 (16 -> 32 at 32 x 32): strips of 8 rows of the gathered gradient
    lds_zero(lds + L::G, L::S1);
    for (int r0 = 0; r0 < 32; r0 += 8) {
      pool_gather<T, 32, 32, 8, true>(gws_at(a, 5, f), am + amax_off(1), gt, r0);
      __syncthreads();
      conv_strip<T, 32, 16, 32, 8>(gt, a.wd[5], r0, EpiPlain<T, 32, 16>{g, gws_at(a, 4, f)});
      __syncthreads();
    }
    lds_zero(lds + L::GT, L::S1);
    __syncthreads();
    res_blocks_bwd<T, 16, 32>(g, gt, a, 0, f);  // ends on a barrier; the stem has no data gradient
  }
}
// fp32: one workgroup a CU (148 KB of LDS).  bf16: 74 KB, and four waves per SIMD asked of the register
// allocator, so that two workgroups share a CU and one's barriers and epilogues run under the other's MFMAs.
__global__ __launch_bounds__(RN_THREADS) void resnet_trunk_bwd_kernel(const BwdArgs<float> a) { trunk_bwd<float>(a); }
__global__ __launch_bounds__(RN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void resnet_trunk_bwd_bf16_kernel(const BwdArgs<__bf16> a) { trunk_bwd<__bf16>(a); }

// ---- the convolutions' weight and bias gradients.  Workgroup (frame group fg, conv id0 + blockIdx.y)
// runs its frames fg, fg + G, ..; per frame the conv's input is a halo tensor in LDS (ReLU applied on
// the way in where the forward applies it; the stem's is the image) and the gradient comes in strips of
// R rows [R][H][COUT] (a pooled conv's through pool_gather).  The contraction index is the pixel.
// Wave w: output channels 16 (w % NTL) .., K-steps w / NTL, + KSPL, ..; all 9 CIN / 16 column tiles, so
// an A fragment is read once for 9 or 18 tiles.  The KSPL waves' tiles are summed in wave order at the end.
template <typename T> struct WgArgs {
  const uint8_t* obs;
  int n, B;
  const T* sav;
  const T* gws;
  const uint8_t* amax;
  float* slab;  // [G][RESNET_BODY_PARAMS]
  GradOff go;
};

// the end of both weight-gradient kernels: the KSPL waves of an output-channel tile summed in wave order
// through the (reused) LDS, then the frame group's slab in the canonical order.  Lane (col, grp) holds
// rows oc = 16 nt + 4 grp + q of column col of tile j; bsum the lane's share of d b[16 nt + col].
template <int NTL, int NN, int CIN, bool STEM>
DEV void wgrad_finish(f32x4 (&acc)[NN], float bsum, float* lds, float* slab, const GradOff& go, int id) {
  constexpr int KSPL = RN_WAVES / NTL;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, grp = lane >> 4, nt = wave % NTL, ks = wave / NTL;
  bsum = xor32_sum(xor16_sum(bsum));  // the four pixel groups of a lane's channel
  f32x4* redt = reinterpret_cast<f32x4*>(lds);
  float* redb = lds + NTL * NN * 256;
  for (int s = 1; s < KSPL; ++s) {
    __syncthreads();
    if (ks == s) {
#pragma unroll
      for (int j = 0; j < NN; ++j) redt[(nt * NN + j) * 64 + lane] = acc[j];
      redb[nt * 64 + lane] = bsum;
    }
    __syncthreads();
    if (ks == 0) {
#pragma unroll
      for (int j = 0; j < NN; ++j) acc[j] += redt[(nt * NN + j) * 64 + lane];
      bsum += redb[nt * 64 + lane];
    }
  }
  if (ks != 0) return;
  constexpr int CR = STEM ? 3 : CIN;  // the canonical tensor's input channels
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    int tap, ci;
    if constexpr (STEM) {
      tap = (16 * j + col) >> 2;
      ci = col & 3;
    } else {
      tap = j / (CIN / 16);
      ci = 16 * (j % (CIN / 16)) + col;
    }
    if (tap < 9 && ci < CR) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int oc = 16 * nt + 4 * grp + q;
        slab[go.w[id] + (oc * CR + ci) * 9 + tap] = STEM ? acc[j][q] * (1.f / 255.f) : acc[j][q];
      }
    }
  }
  if (grp == 0) slab[go.b[id] + 16 * nt + col] = bsum;
}

// fp32 on mfma_f32_16x16x4f32, one k value a lane: lane (col, grp) takes pixels 16 k + 4 e + grp of K-step
// k, so MFMA e's A operand g[pixel][16 nt + col] and B operand in[pixel + tap][16 half + col] are each four
// runs of 16 consecutive floats, one per pixel, read with ds_read_b32 -- no transpose, no staging copy.
// The stem's image is held as the forward holds it, the bytes converted on the read.
template <int CIN, int COUT, int H, int R, bool POOLED, bool RELU, bool STEM>
__global__ __launch_bounds__(RN_THREADS) void resnet_wgrad_kernel(const WgArgs<float> a, int id0) {
  constexpr int P = H + 2, NTL = COUT / 16, KSPL = RN_WAVES / NTL, NN = STEM ? 3 : 9 * CIN / 16, NK = R * H / 16;
  constexpr int IN_FLOATS = STEM ? 66 * 66 : P * P * CIN, GS_FLOATS = R * H * COUT;
  constexpr int RED_FLOATS = NTL * NN * 256 + NTL * 64;
  constexpr int LDS_FLOATS = IN_FLOATS + GS_FLOATS > RED_FLOATS ? IN_FLOATS + GS_FLOATS : RED_FLOATS;
  static_assert(LDS_FLOATS * 4 <= 160 * 1024 && IN_FLOATS % 4 == 0, "the CU's LDS");
  static_assert(NK % KSPL == 0 || NK > KSPL, "K-steps over the waves");
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* const in = lds;
  float* const gs = lds + IN_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, grp = lane >> 4, nt = wave % NTL, ks = wave / NTL;
  const int id = id0 + blockIdx.y, stage = id / 5;
  f32x4 acc[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  // the B operand's offset from a pixel's top-left tap, per column tile (the stem: per lane)
  int boff[NN];
  [[maybe_unused]] int bsh = 0;
  [[maybe_unused]] bool bok[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    if constexpr (STEM) {
      const int tap = (16 * j + col) >> 2;
      bok[j] = tap < 9;
      const int tc = min(tap, 8);
      boff[j] = (tc / 3) * 66 + tc % 3;
      bsh = 8 * (col & 3);
    } else {
      const int tap = j / (CIN / 16), half = j % (CIN / 16);
      boff[j] = ((tap / 3) * P + tap % 3) * CIN + 16 * half + col;
    }
  }
  for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
    __syncthreads();  // the previous frame's reads are done
    if constexpr (STEM) {
      lds_zero(reinterpret_cast<char*>(in), IN_FLOATS * 4);
      __syncthreads();
      load_image(a.obs, f, reinterpret_cast<uint32_t*>(in));
    } else {
      const float* src = a.sav + stage_at(a.B, id - 1, f);
      for (int i = tid; i < P * P * CIN / 4; i += RN_THREADS) {
        const int c0 = 4 * (i % (CIN / 4)), px = (i / (CIN / 4)) % P, py = i / (CIN / 4 * P);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (py >= 1 && py <= H && px >= 1 && px <= H) {
          v = *reinterpret_cast<const f32x4*>(src + ((py - 1) * H + px - 1) * CIN + c0);
          if (RELU) v = relu_v(v);
        }
        *reinterpret_cast<f32x4*>(in + (py * P + px) * CIN + c0) = v;
      }
    }
    const float* gsrc = a.gws + stage_at(a.B, id, f);
    for (int r0 = 0; r0 < H; r0 += R) {
      if (r0) __syncthreads();  // the previous strip's reads are done
      if constexpr (POOLED) {
        pool_gather<float, H, COUT, R, false>(gsrc, a.amax + (size_t)f * RN_AMAX_FRAME + amax_off(stage), gs, r0);
      } else {
        for (int i = tid; i < GS_FLOATS / 4; i += RN_THREADS)
          *reinterpret_cast<f32x4*>(gs + 4 * i) = *reinterpret_cast<const f32x4*>(gsrc + r0 * H * COUT + 4 * i);
      }
      __syncthreads();
      for (int k = ks; k < NK; k += KSPL) {
        f32x4 av;
        int po[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int pl = 16 * k + 4 * e + grp;
          av[e] = gs[pl * COUT + 16 * nt + col];
          po[e] = STEM ? (r0 + pl / H) * 66 + pl % H : ((r0 + pl / H) * P + pl % H) * CIN;
        }
        bsum += (av[0] + av[1]) + (av[2] + av[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float bv[NN];
#pragma unroll
          for (int j = 0; j < NN; ++j) {
            if constexpr (STEM) {
              const uint32_t d = reinterpret_cast<const uint32_t*>(in)[po[e] + boff[j]];
              bv[j] = bok[j] ? (float)((d >> bsh) & 255u) : 0.f;
            } else {
              bv[j] = in[po[e] + boff[j]];
            }
          }
#pragma unroll
          for (int j = 0; j < NN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j], acc[j], 0, 0, 0);
        }
      }
    }
  }
  wgrad_finish<NTL, NN, CIN, STEM>(acc, bsum, lds, a.slab + (size_t)blockIdx.x * RESNET_BODY_PARAMS, a.go, id);
}

// bf16 on mfma_f32_16x16x32_bf16, eight k values a lane -- eight pixels of one channel, which in a
// channels-last tensor lie C elements apart.  gfx950's transposing LDS read fetches them: in
// ds_read_b64_tr_b16 lane i of a 16-lane group gives the address of 4 consecutive channels (8 bytes) of
// row i / 4 and receives channel i of the group's four rows.  Rows are pixels at a pitch of C elements,
// so two reads make one fragment, for the gradient strip [R H][COUT] and, at a tap's offset, for the input
// halo tensor [P P][CIN] alike: no transposing copy, no staging tile.  The k slots of a K-step of 32
// pixels are dealt so that one read instruction covers 16 consecutive pixels: lane group grp takes pixels
// 4 grp .. 4 grp + 3 with its first read and 16 + 4 grp .. with its second (the order of k within a step is
// free, the two operands share it; H is a multiple of 8, so a run of 4 never leaves an image row, and a
// tap moves an address by whole pixels, so every lane address is 8-byte aligned).  At C = 16 the 32 lanes
// the LDS serves at once then read 256 consecutive bytes (tools/ldsbank.py: 1.0x; pixels 8 grp .. 8 grp + 7
// per group would be 2.0x); at C = 32 they read half of each of 8 pixels, 2.0x.
// The stem (columns tap * 4 + ci) holds the image as a bf16 halo tensor [66][66][4], 0..255 exact: the four
// 8-byte pieces of a 16-lane group are the pixels of four taps, so a read returns the (tap, ci) column
// tile with no gather of bytes.  Lanes of taps 9..11 read tap 8 again; their columns are not stored.
DEV bf16x8 lds_frag_tr(const __bf16* p, int step) {
  const bf16x4_t x = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
  const bf16x4_t y = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + step));
  bf16x8 v;
  v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
  v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
  return v;
}

// frame f's image into img [66][66][4] bf16 (zeroed): (c0, c1, c2, 0) inside the zero border
DEV void load_image_bf16(const uint8_t* __restrict__ obs, int f, __bf16* img) {
  const int tid = threadIdx.x;
  if (tid < 256) {
    const int yy = tid >> 2, x0 = (tid & 3) * 16;
    const uint8_t* src = obs + (size_t)f * 12288 + yy * 64 + x0;
    const i32x4 p0 = *reinterpret_cast<const i32x4*>(src), p1 = *reinterpret_cast<const i32x4*>(src + 4096),
                p2 = *reinterpret_cast<const i32x4*>(src + 8192);
    i32x2* dst = reinterpret_cast<i32x2*>(img) + (yy + 1) * 66 + x0 + 1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int sh = 8 * (j & 3);
      dst[j] = i32x2{pack_bf16x2((float)(((uint32_t)p0[j >> 2] >> sh) & 255u), (float)(((uint32_t)p1[j >> 2] >> sh) & 255u)),
                     pack_bf16x2((float)(((uint32_t)p2[j >> 2] >> sh) & 255u), 0.f)};
    }
  }
}

template <int CIN, int COUT, int H, int R, bool POOLED, bool RELU, bool STEM>
__global__ __launch_bounds__(RN_THREADS) void resnet_wgrad_bf16_kernel(const WgArgs<__bf16> a, int id0) {
  constexpr int P = H + 2, NTL = COUT / 16, KSPL = RN_WAVES / NTL, NN = STEM ? 3 : 9 * CIN / 16, NK = R * H / 32;
  constexpr int IN_ELTS = P * P * CIN, GS_ELTS = R * H * COUT;  // (the stem: CIN = 4, the pixel's pitch)
  constexpr int RED_BYTES = (NTL * NN * 256 + NTL * 64) * 4;
  constexpr int LDS_BYTES = (IN_ELTS + GS_ELTS) * 2 > RED_BYTES ? (IN_ELTS + GS_ELTS) * 2 : RED_BYTES;
  // the second read's 16 pixels on: in the same image row, or 16 / H rows down
  constexpr int STEP_B = H >= 32 ? 16 * CIN : (16 / H) * P * CIN;
  static_assert(LDS_BYTES <= 160 * 1024 && IN_ELTS % 8 == 0 && GS_ELTS % 8 == 0, "the CU's LDS");
  static_assert(H % 8 == 0 && (R * H) % 32 == 0 && (H >= 32 || 16 % H == 0), "whole K-steps; a run of 4 pixels in one row");
  __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
  __bf16* const in = reinterpret_cast<__bf16*>(lds);
  __bf16* const gs = in + IN_ELTS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, grp = lane >> 4, nt = wave % NTL, ks = wave / NTL;
  const int rq = col >> 2, pp = col & 3;  // the lane's address: row rq of its group's four, channels 4 pp ..
  const int id = id0 + blockIdx.y, stage = id / 5;
  f32x4 acc[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  // the B operand's element offset from a pixel's top-left tap, per column tile, for the lane's address
  int boff[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    if constexpr (STEM) {
      const int tap = min(4 * j + pp, 8);
      boff[j] = ((tap / 3) * P + tap % 3) * CIN;
    } else {
      const int tap = j / (CIN / 16), half = j % (CIN / 16);
      boff[j] = ((tap / 3) * P + tap % 3) * CIN + 16 * half + 4 * pp;
    }
  }
  for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
    __syncthreads();  // the previous frame's reads are done
    if constexpr (STEM) {
      lds_zero(lds, IN_ELTS * 2);
      __syncthreads();
      load_image_bf16(a.obs, f, in);
    } else {
      const __bf16* src = a.sav + stage_at(a.B, id - 1, f);
      for (int i = tid; i < IN_ELTS / 8; i += RN_THREADS) {
        const int c0 = 8 * (i % (CIN / 8)), px = (i / (CIN / 8)) % P, py = i / (CIN / 8 * P);
        bf16x8 v = Frag<__bf16>::zero();
        if (py >= 1 && py <= H && px >= 1 && px <= H) {
          v = *reinterpret_cast<const bf16x8*>(src + ((py - 1) * H + px - 1) * CIN + c0);
          if (RELU) v = relu_v(v);
        }
        *reinterpret_cast<bf16x8*>(in + (py * P + px) * CIN + c0) = v;
      }
    }
    const __bf16* gsrc = a.gws + stage_at(a.B, id, f);
    for (int r0 = 0; r0 < H; r0 += R) {
      if (r0) __syncthreads();  // the previous strip's reads are done
      if constexpr (POOLED) {
        pool_gather<__bf16, H, COUT, R, false>(gsrc, a.amax + (size_t)f * RN_AMAX_FRAME + amax_off(stage), gs, r0);
      } else {
        for (int i = tid; i < GS_ELTS / 8; i += RN_THREADS)
          *reinterpret_cast<bf16x8*>(gs + 8 * i) = *reinterpret_cast<const bf16x8*>(gsrc + r0 * H * COUT + 8 * i);
      }
      __syncthreads();
      for (int k = ks; k < NK; k += KSPL) {
        const int pl = 32 * k + 4 * grp + rq;  // the pixel whose row the lane addresses in its first read
        const bf16x8 av = lds_frag_tr(gs + pl * COUT + 16 * nt + 4 * pp, 16 * COUT);
        bsum += (((float)av[0] + (float)av[1]) + ((float)av[2] + (float)av[3])) +
                (((float)av[4] + (float)av[5]) + ((float)av[6] + (float)av[7]));
        const __bf16* bp = in + ((r0 + pl / H) * P + pl % H) * CIN;
        bf16x8 bv[NN];
#pragma unroll
        for (int j = 0; j < NN; ++j) bv[j] = lds_frag_tr(bp + boff[j], STEP_B);
#pragma unroll
        for (int j = 0; j < NN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[j], acc[j], 0, 0, 0);
      }
    }
  }
  wgrad_finish<NTL, NN, CIN, STEM>(acc, bsum, reinterpret_cast<float*>(lds), a.slab + (size_t)blockIdx.x * RESNET_BODY_PARAMS,
                                   a.go, id);
}

__global__ __launch_bounds__(256) void resnet_wreduce_kernel(const float* __restrict__ slab, int G, float* __restrict__ grad,
                                                             int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= RESNET_BODY_PARAMS) return;
  float s = slab[i];
  for (int g = 1; g < G; ++g) s += slab[(size_t)g * RESNET_BODY_PARAMS + i];
  grad_out(grad, i, s, accumulate);
}
