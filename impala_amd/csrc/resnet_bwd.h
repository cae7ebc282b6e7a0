// The backward pass of the IMPALA ResNet actor-critic in fp32, included by
// resnet.hip inside its unnamed namespace, after the forward's helpers.
//
// One resnet_backward of n frames, from what resnet_forward_train left in the handle:
//   resnet_head_bwd_kernel     one wave per frame: gz = GELU'(z) * (Wh^T dheads), z re-summed from the
//                              projection's K chunks in the forward's order
//   resnet_head_wgrad_kernel   d Wh, d bh, d bfc: one thread per element, the frames in order
//   resnet_fc_wgrad_kernel     d Wfc [256][2048] = gz^T y on the MFMAs, the contraction over frames
//   resnet_fc_dgrad_kernel     gy [n][2048] = gz Wfc on the MFMAs (Wfc packed transposed)
//   resnet_ln_affine_kernel    d gamma, d beta: one thread per feature, the frames in order
//   resnet_trunk_bwd_kernel    one frame per workgroup: LayerNorm and ReLU backward, then the data
//                              gradients of the 14 non-stem convolutions as pad-1 convolutions of
//                              the gradient with the flipped, Cin/Cout-swapped weights (the
//                              forward's conv_tiles), masks from the saved tensors in L2, the
//                              max-pools as gathers; the gradient at every convolution's output
//                              goes to HBM
//   resnet_wgrad_kernel        d W, d b of the 15 convolutions: workgroup (frame group, conv)
//                              holds the whole d W of its conv in accumulators over its frames;
//                              D[oc][tap, ci] = sum_pixel g[pixel][oc] relu(in)[pixel + tap][ci]
//   resnet_wreduce_kernel      the frame groups' partial d W, d b summed in order into the flat gradient
// No floating-point atomics: every sum over frames has one fixed order.
#pragma once

struct BwdArgs {
  int n, B;
  const float* wd[RN_CONVS];  // data-gradient weights of convs 1..14, fragment-major
  const float* vecs;
  const float* sav;      // the handle's stages, amax, lnstat as resnet_forward_train left them
  const uint8_t* amax;
  const float* lnstat;
  const float* gy;       // [n][2048], kernel order
  float* gws;            // the gradient at every conv's output (post-pool for 0, 5, 10), the stage tensors' layout
};

DEV const float* sav_at(const BwdArgs& a, int id, int f) { return a.sav + stage_at(a.B, id, f); }
DEV float* gws_at(const BwdArgs& a, int id, int f) { return a.gws + stage_at(a.B, id, f); }

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
__global__ __launch_bounds__(256) void resnet_head_wgrad_kernel(const float* __restrict__ h, const float* __restrict__ gz,
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
    s = fmaf(d, h[(size_t)f * RN_HID + j], s);
    sb += d;
  }
  grad_out(grad, (o < A ? go.wa + o * RN_HID : go.wc) + j, s, accumulate);
  if (j == 0) grad_out(grad, o < A ? go.ba + o : go.bc, sb, accumulate);
}

// d Wfc[o][k'] = sum_f gz[f][o] y[f][k']: workgroup (o tile, 256 features), a wave 16 x 64 of it.  Both
// operands are read along the frames from L2: lane (col, grp) takes frames f0 + 4 e + grp, so a wave
// instruction reads four 64-byte runs.  Frames past n contribute zero.
__global__ __launch_bounds__(256) void resnet_fc_wgrad_kernel(const float* __restrict__ gz, const float* __restrict__ y,
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
      for (int j = 0; j < 4; ++j) bv[j][e] = y[(size_t)fc * RN_FEAT + k0 + 16 * j + col];
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
__global__ __launch_bounds__(256) void resnet_pack_fct_kernel(const float* __restrict__ w, float* __restrict__ dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // < 2048 * 256
  const int j = e & 3, lane = (e >> 2) & 63, s = (e >> 8) & 15, kt = e >> 12;
  const int k = 16 * kt + (lane & 15), o = 16 * s + 4 * (lane >> 4) + j;
  dst[e] = w[(size_t)o * RN_FEAT + (k & 31) * 64 + (k >> 5)];
}
// data-gradient weights of a conv, canonical [COUT][CIN][3][3] -> fragment-major as the forward's with
// row ci and k = tap' * COUT + oc, tap' = 8 - tap: the gradient's convolution runs on conv_tiles
__global__ __launch_bounds__(256) void resnet_pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ dst,
                                                                int cin, int cout, int total) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int nks = 9 * cout / 16;
  const int j = e & 3, lane = (e >> 2) & 63, s = (e >> 8) % nks, nt = (e >> 8) / nks;
  const int ci = 16 * nt + (lane & 15), k = s * 16 + (lane >> 4) * 4 + j;
  const int tap = k / cout, oc = k % cout;
  dst[e] = w[((size_t)oc * cin + ci) * 9 + (8 - tap)];
}

// d gamma[k'] = sum_f gy xhat, d beta[k'] = sum_f gy, xhat from the saved x (stage tensor 14) and statistics
__global__ __launch_bounds__(256) void resnet_ln_affine_kernel(const float* __restrict__ gy, const float* __restrict__ x14,
                                                               const float* __restrict__ lnstat, float* __restrict__ grad,
                                                               int lng, int lnb, int n, int accumulate) {
  const int k = blockIdx.x * 256 + threadIdx.x, canon = (k & 31) * 64 + (k >> 5);
  float sg = 0.f, sb = 0.f;
  for (int f = 0; f < n; ++f) {
    const float g = gy[(size_t)f * RN_FEAT + k];
    const float xh = (fmaxf(x14[(size_t)f * RN_FEAT + k], 0.f) - lnstat[2 * f]) * lnstat[2 * f + 1];
    sg = fmaf(g, xh, sg);
    sb += g;
  }
  grad_out(grad, lng + canon, sg, accumulate);
  grad_out(grad, lnb + canon, sb, accumulate);
}

// ---- the max-pools' backward as a gather.  Rows of the gradient at a pooled conv's output (HC x HC x C)
// from the gradient g [HO][HO][C] at the pool's output and the winning taps: pixel (r, cx) collects from
// the windows (oy, ox) with |r - 2 oy| <= 1, |cx - 2 ox| <= 1 whose byte names it, in a fixed order.
// HALO: rows r0 - 1 .. r0 + R as a halo tensor [R + 2][HC + 2][C], zero outside the image; else rows
// r0 .. r0 + R - 1 as [R][HC][C].
template <int HC, int C, int R, bool HALO>
DEV void pool_gather(const float* __restrict__ g, const uint8_t* __restrict__ am, float* __restrict__ dst, int r0) {
  constexpr int HO = HC / 2, NR = HALO ? R + 2 : R, W = HALO ? HC + 2 : HC, CV = C / 4, ITEMS = NR * W * CV;
  for (int i = threadIdx.x; i < ITEMS; i += RN_THREADS) {
    const int c0 = 4 * (i % CV), px = (i / CV) % W, j = i / (CV * W);
    const int r = r0 + j - (HALO ? 1 : 0), cx = px - (HALO ? 1 : 0);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
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
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + at);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (((win >> (8 * q)) & 255u) == tap) s[q] += gv[q];
          }
        }
    }
    *reinterpret_cast<f32x4*>(dst + (j * W + px) * C + c0) = s;
  }
}

// ---- epilogues of the gradient's convolutions: the mask from the saved tensor in L2, the result into
// the interior of an LDS halo tensor and to gws
template <int H, int C> struct EpiMaskStore {  // gt = [t > 0] acc
  float* out;
  const float* sav;
  float* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const int at = (y * H + x) * C + c0;
    const f32x4 m = *reinterpret_cast<const f32x4*>(sav + at);
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = m[q] > 0.f ? acc[q] : 0.f;
    *reinterpret_cast<f32x4*>(out + ((y + 1) * (H + 2) + x + 1) * C + c0) = v;
    *reinterpret_cast<f32x4*>(gout + at) = v;
  }
};
template <int H, int C> struct EpiMaskAdd {  // g += [x > 0] acc, in place (the convolution reads gt only)
  float* g;
  const float* sav;
  float* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    const int at = (y * H + x) * C + c0;
    const f32x4 m = *reinterpret_cast<const f32x4*>(sav + at);
    float* p = g + ((y + 1) * (H + 2) + x + 1) * C + c0;
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += m[q] > 0.f ? acc[q] : 0.f;
    *reinterpret_cast<f32x4*>(p) = v;
    *reinterpret_cast<f32x4*>(gout + at) = v;
  }
};
template <int H, int C> struct EpiPlain {
  float* out;
  float* gout;
  DEV void operator()(int y, int x, int c0, f32x4 acc) const {
    *reinterpret_cast<f32x4*>(out + ((y + 1) * (H + 2) + x + 1) * C + c0) = acc;
    *reinterpret_cast<f32x4*>(gout + (y * H + x) * C + c0) = acc;
  }
};

// output rows r0 .. r0 + R - 1 of a pad-1 convolution whose operand is a halo strip [R + 2][H + 2][CIN]
// (row 0 = image row r0 - 1)
template <int CIN, int COUT, int H, int R, class Epi>
DEV void conv_strip(const float* __restrict__ strip, const float* __restrict__ wpk, int r0, Epi epi) {
  constexpr int NKS = conv_nks<float, CIN>(), P = H + 2;
  const int grp = (threadIdx.x & 63) >> 4;
  int off[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) off[s] = tap_off<float, CIN, P>(s, grp);
  conv_tiles<float, NKS, COUT, H, R>(
      wpk, r0, [&](int y, int x, int s) { return *reinterpret_cast<const f32x4*>(strip + ((y - r0) * P + x) * CIN + off[s]); },
      epi);
}

// the two residual blocks of a stage, backwards: g (the gradient at the stage's output, a halo tensor)
// becomes the gradient at the pool's output; gt is scratch with a zero halo.  P0: the stage's pooled conv.
template <int C, int H> DEV void res_blocks_bwd(float* g, float* gt, const BwdArgs& a, int P0, int f) {
#pragma unroll
  for (int blk = 1; blk >= 0; --blk) {
    const int xin = P0 + 2 * blk, i0 = xin + 1, i1 = xin + 2;
    conv_lds<float, C, C, H, H, false>(g, a.wd[i1], 0, EpiMaskStore<H, C>{gt, sav_at(a, i0, f), gws_at(a, i0, f)});
    __syncthreads();
    conv_lds<float, C, C, H, H, false>(gt, a.wd[i0], 0, EpiMaskAdd<H, C>{g, sav_at(a, xin, f), gws_at(a, xin, f)});
    __syncthreads();
  }
}

struct LdsBwd {
  static constexpr int S1 = Lds<float>::S1, S2 = Lds<float>::S2, S3 = Lds<float>::S3;
  static constexpr int G = 0, GT = S1, RED = 2 * S1, TOTAL = RED + 64 * 4;
  static_assert(10 * 34 * 32 * 4 <= S1 && 18 * 18 * 32 * 4 <= S1, "the pools' gradient strips live in gt's place");
  static_assert(TOTAL <= 160 * 1024, "the CU's LDS");
};

__global__ __launch_bounds__(RN_THREADS) void resnet_trunk_bwd_kernel(const BwdArgs a) {
  using L = LdsBwd;
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* const g = reinterpret_cast<float*>(lds + L::G);
  float* const gt = reinterpret_cast<float*>(lds + L::GT);
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
      const f32x4 x = *reinterpret_cast<const f32x4*>(sav_at(a, 14, f) + k);
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
      f32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = x[q] > 0.f ? rstd * (gg[q] - m1 - xh[q] * m2) : 0.f;
      *reinterpret_cast<f32x4*>(g + (((p >> 3) + 1) * 10 + (p & 7) + 1) * 32 + c0) = v;
      *reinterpret_cast<f32x4*>(gws_at(a, 14, f) + k) = v;
    }
    __syncthreads();
    res_blocks_bwd<32, 8>(g, gt, a, 10, f);
    // ---- stage 3's pool and conv 10 (32 -> 32 at 16 x 16): the gathered gradient whole in gt's place
    lds_zero(lds + L::G, L::S2);
    pool_gather<16, 32, 16, true>(gws_at(a, 10, f), am + amax_off(2), gt, 0);
    __syncthreads();
    conv_strip<32, 32, 16, 16>(gt, a.wd[10], 0, EpiPlain<16, 32>{g, gws_at(a, 9, f)});
    __syncthreads();
    lds_zero(lds + L::GT, L::S2);
    __syncthreads();
    res_blocks_bwd<32, 16>(g, gt, a, 5, f);
    // ---- stage 2's pool and conv 5 (16 -> 32 at 32 x 32): strips of 8 rows of the gathered gradient
    lds_zero(lds + L::G, L::S1);
    for (int r0 = 0; r0 < 32; r0 += 8) {
      pool_gather<32, 32, 8, true>(gws_at(a, 5, f), am + amax_off(1), gt, r0);
      __syncthreads();
      conv_strip<32, 16, 32, 8>(gt, a.wd[5], r0, EpiPlain<32, 16>{g, gws_at(a, 4, f)});
      __syncthreads();
    }
    lds_zero(lds + L::GT, L::S1);
    __syncthreads();
    res_blocks_bwd<16, 32>(g, gt, a, 0, f);  // ends on a barrier; the stem has no data gradient
  }
}

// ---- the convolutions' weight and bias gradients.  Workgroup (frame group fg, conv id0 + blockIdx.y)
// runs its frames fg, fg + G, ..; per frame the conv's input is a halo tensor in LDS (ReLU applied on
// the way in where the forward applies it; the stem's is the image as the forward holds it) and the
// gradient comes in strips of R rows [R][H][COUT] (a pooled conv's through pool_gather).  The
// contraction index is the pixel: lane (col, grp) takes pixels 16 k + 4 e + grp of K-step k, so MFMA
// e's A operand g[pixel][16 nt + col] and B operand in[pixel + tap][16 half + col] are each four runs
// of 16 consecutive floats, one per pixel, read with ds_read_b32 -- no transpose, no staging copy.
// Wave w: output channels 16 (w % NTL) .., K-steps w / NTL, + KSPL, ..; all 9 CIN / 16 column tiles, so
// an A fragment is read once for 9 or 18 tiles.  The KSPL waves' tiles are summed in wave order at the end.
struct WgArgs {
  const uint8_t* obs;
  int n, B;
  const float* sav;
  const float* gws;
  const uint8_t* amax;
  float* slab;  // [G][RESNET_BODY_PARAMS]
  GradOff go;
};

template <int CIN, int COUT, int H, int R, bool POOLED, bool RELU, bool STEM>
__global__ __launch_bounds__(RN_THREADS) void resnet_wgrad_kernel(const WgArgs a, int id0) {
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
        pool_gather<H, COUT, R, false>(gsrc, a.amax + (size_t)f * RN_AMAX_FRAME + amax_off(stage), gs, r0);
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
  // ---- the KSPL waves of an output-channel tile, summed in wave order through the (reused) LDS
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
  float* slab = a.slab + (size_t)blockIdx.x * RESNET_BODY_PARAMS;
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
        slab[a.go.w[id] + (oc * CR + ci) * 9 + tap] = STEM ? acc[j][q] * (1.f / 255.f) : acc[j][q];
      }
    }
  }
  if (grp == 0) slab[a.go.b[id] + 16 * nt + col] = bsum;
}

__global__ __launch_bounds__(256) void resnet_wreduce_kernel(const float* __restrict__ slab, int G, float* __restrict__ grad,
                                                             int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= RESNET_BODY_PARAMS) return;
  float s = slab[i];
  for (int g = 1; g < G; ++g) s += slab[(size_t)g * RESNET_BODY_PARAMS + i];
  grad_out(grad, i, s, accumulate);
}
