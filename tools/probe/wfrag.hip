// Probe: what sets the rate at which a CU pulls L2-resident fp32 weight fragments into
// registers, the bytes or the lines one wave instruction touches?  256 workgroups of 512 threads
// (one per CU: 96 KB of LDS each), every loading wave issues all its 16-byte loads back to back
// and then sums them, in the two shapes of each of the per-frame kernels' weight loads:
//   "rows"  lane l reads 16 B of row (l & 15) at column 4 (l >> 4): 16 lines per instruction,
//           64 B of each (the k-major / transposed matrices)
//   "frag"  lane l reads 16 B at byte 16 l of the instruction's own 1 KB (fragment-major)
// for
//   w3t   waves 4..7, 36 loads each: 147,456 B per workgroup (lnc3.h role 1, once per workgroup)
//   w2t   waves 0..3, 32 loads each: 131,072 B (conv1.h c12_load_w2, all four taps at once)
//   w2t/tap  the same, 8 loads per wave and repetition: one tap, 32,768 B (pre(k))
//   w2    all 8 waves, 32 loads each of the oc tile wave & 3: 131,072 B touched, 262,144 B
//         loaded per repetition (the forward's conv2 stream of two frames in flight)
// REPS repetitions per launch behind one barrier each; the first is timed apart (its lines
// come from wherever the previous launch left them), the figures are the later ones' mean.
// Prints, per case: us per repetition (s_memrealtime, 100 MHz, slowest wave of the median
// workgroup and of the slowest workgroup), clocks (s_memtime) and B/clk/CU.
// build: hipcc --offload-arch=gfx950 -O3 -o wfrag tools/probe/wfrag.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WGS = 256, REPS = 9, NFLOAT = 64 * 576;  // the larger matrix, W3

enum { W3_ROWS, W3_FRAG, W2T_ROWS, W2T_FRAG, W2TAP_ROWS, W2TAP_FRAG, W2F_ROWS, W2F_FRAG, NCASE };
struct Case {
  const char* name;
  int first_wave, nwave, nload;  // loading waves, loads per wave and repetition
};
__host__ __device__ constexpr Case kCase(int c) {
  return c == W3_ROWS ? Case{"w3t rows", 4, 4, 36} : c == W3_FRAG ? Case{"w3t frag", 4, 4, 36}
       : c == W2T_ROWS ? Case{"w2t rows", 0, 4, 32} : c == W2T_FRAG ? Case{"w2t frag", 0, 4, 32}
       : c == W2TAP_ROWS ? Case{"w2t/tap rows", 0, 4, 8} : c == W2TAP_FRAG ? Case{"w2t/tap frag", 0, 4, 8}
       : c == W2F_ROWS ? Case{"w2 fwd rows", 0, 8, 32} : Case{"w2 fwd frag", 0, 8, 32};
}

// element offset of load i of wave w (index among the loading waves), lane l; rep r picks the tap
// in the per-tap cases
template <int C> __device__ int elem(int w, int i, int l, int r) {
  const int row = l & 15, col = 4 * (l >> 4);
  if (C == W3_ROWS) return ((i >> 2) * 64 + 16 * w + row) * 64 + (i & 3) * 16 + col;  // i = tap * 4 + ko
  if (C == W3_FRAG) return (w * 36 + i) * 256 + 4 * l;
  if (C == W2T_ROWS || C == W2TAP_ROWS) {  // i = (t * 4 + ks) * 2 + ct, class w
    const int ii = C == W2TAP_ROWS ? (r & 3) * 8 + i : i;
    const int t = ii >> 3, ks = (ii >> 1) & 3, ct = ii & 1;
    const int kh = (w >> 1) + 2 * (t >> 1), kw = (w & 1) + 2 * (t & 1);
    return ((kh * 4 + kw) * 32 + 16 * ct + row) * 64 + ks * 16 + col;
  }
  if (C == W2T_FRAG) return (w * 32 + i) * 256 + 4 * l;
  if (C == W2TAP_FRAG) return (w * 32 + (r & 3) * 8 + i) * 256 + 4 * l;
  if (C == W2F_ROWS) return (16 * (w & 3) + row) * 512 + i * 16 + col;  // w2 [64][512], i = ks
  return ((w & 3) * 32 + i) * 256 + 4 * l;
}

template <int C>
__global__ __launch_bounds__(512) void pull(const float* __restrict__ w, float* __restrict__ out,
                                            unsigned long long* __restrict__ stamps) {
  constexpr Case cs = kCase(C);
  __shared__ float pad[96 * 1024 / 4];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  pad[t] = 0.f;
  const int lw = wave - cs.first_wave;
  const bool loads = lw >= 0 && lw < cs.nwave;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  unsigned long long c0 = 0, c1 = 0, r0 = 0, r1 = 0, cf = 0, rf = 0;
  for (int r = 0; r < REPS; ++r) {
    __syncthreads();
    if (!loads) continue;
    const float* p = w;
    int ln = lane;
    asm volatile("" : "+s"(p), "+v"(ln));  // nothing carried over from the last repetition
    if (r <= 1) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    f32x4 v[cs.nload];
#pragma unroll
    for (int i = 0; i < cs.nload; ++i) v[i] = *reinterpret_cast<const f32x4*>(p + elem<C>(lw, i, ln, r));
#pragma unroll
    for (int i = 0; i < cs.nload; ++i) asm volatile("" ::"v"(v[i]));  // all of them arrived
#pragma unroll
    for (int i = 0; i < cs.nload; ++i) acc += v[i];
    asm volatile("" : "+v"(acc));
    c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (r == 0) { cf = c1 - c0; rf = r1 - r0; }
  }
  out[blockIdx.x * 512 + t] = acc[0] + acc[1] + acc[2] + acc[3] + pad[t ^ 1];
  if (loads && lane == 0) {
    unsigned long long* s = stamps + (blockIdx.x * 8 + wave) * 4;
    s[0] = cf; s[1] = rf; s[2] = c1 - c0; s[3] = r1 - r0;  // first repetition; repetitions 1..REPS-1
  }
}

template <int C> void run(const float* w, float* out, unsigned long long* stamps) {
  constexpr Case cs = kCase(C);
  std::vector<unsigned long long> h(WGS * 8 * 4);
  std::vector<double> clk, us, first;
  for (int it = 0; it < 12; ++it) {
    (void)hipMemset(stamps, 0, h.size() * 8);
    pull<C><<<WGS, 512>>>(w, out, stamps);
    (void)hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost);
    if (it < 2) continue;
    for (int g = 0; g < WGS; ++g) {  // a workgroup's figure is its slowest wave's
      unsigned long long m[4] = {0, 0, 0, 0};
      for (int wv = 0; wv < 8; ++wv)
        for (int k = 0; k < 4; ++k) m[k] = std::max(m[k], h[(g * 8 + wv) * 4 + k]);
      first.push_back(m[1] / 100.0);
      clk.push_back(m[2] / double(REPS - 1));
      us.push_back(m[3] / 100.0 / (REPS - 1));
    }
  }
  std::sort(clk.begin(), clk.end());
  std::sort(us.begin(), us.end());
  std::sort(first.begin(), first.end());
  const double bytes = double(cs.nwave) * cs.nload * 1024, cm = clk[clk.size() / 2];
  printf("%-13s %7.0f B/rep: median workgroup %5.2f us %6.0f clk %5.1f B/clk/CU | slowest %5.2f us %6.0f clk"
         " %5.1f B/clk/CU | first rep %5.2f us\n",
         cs.name, bytes, us[us.size() / 2], cm, bytes / cm, us.back(), clk.back(), bytes / clk.back(),
         first[first.size() / 2]);
}

int main() {
  float *w, *out;
  unsigned long long* stamps;
  (void)hipMalloc(&w, NFLOAT * 4);
  (void)hipMalloc(&out, WGS * 512 * 4);
  (void)hipMalloc(&stamps, WGS * 8 * 4 * 8);
  (void)hipMemset(w, 0, NFLOAT * 4);
  run<W3_ROWS>(w, out, stamps);
  run<W3_FRAG>(w, out, stamps);
  run<W2T_ROWS>(w, out, stamps);
  run<W2T_FRAG>(w, out, stamps);
  run<W2TAP_ROWS>(w, out, stamps);
  run<W2TAP_FRAG>(w, out, stamps);
  run<W2F_ROWS>(w, out, stamps);
  run<W2F_FRAG>(w, out, stamps);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
