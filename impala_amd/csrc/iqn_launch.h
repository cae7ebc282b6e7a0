// Launchers of the IQN kernels (csrc/iqn.hip), called by the host side in csrc/iqn.h.  Each
// enqueues its kernels on `st` and returns hipGetLastError() of the first launch that failed.
// The kernels are compiled in a translation unit of their own so that impala.hip's code object
// stays what it is without them.  `bf16` picks the compute type T of the untyped pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iqn_dev {

// one net's kernel-layout weights past the conv trunk
struct HeadWeights {
  const void* wq;    // T [1024][64], rows p*64 + c
  const float* bq;   // [1024], p*64 + c
  const float* gam;  // [1024] LayerNorm weight, p*64 + c
  const float* bet;  // [1024]
  const void* wfc;   // T [512][1024]
  const float* bfc;  // [512]
  const void* wh;    // T [16][512]: advantage rows 0..A-1, value row 15
  const float* bh;   // [16]
};
// the R-row workspace the head runs in
struct HeadWork {
  void* y;       // T [R][YLD]
  float* zg;     // [R][512]
  void* h;       // T [R][512]
  float* heads;  // [R][16]
};

// canonical Wq (1024 x 64, rows c*16 + p) followed by bq (1024) -> wq (T), bq (fp32), permuted
hipError_t launch_pack(bool bf16, const float* wq_bq, void* wq, float* bq, hipStream_t st);
// taus[r] for r < R by the header's draw
hipError_t launch_taus(uint64_t seed, uint64_t counter, int which, int R, float* taus, hipStream_t st);
// act3 [n][1024] (T, post-ReLU) and taus [R] -> q [R][A]: embed + LayerNorm, FC, heads, dueling
hipError_t launch_head(bool bf16, const HeadWeights& w, const HeadWork& ws, const void* act3, const float* taus,
                       int R, int W, int A, int n_cu, float* q, hipStream_t st);
hipError_t launch_act(const float* q_on, const float* q_tg, int n, int W, int A, const float* eps, float eps_all,
                      uint64_t seed, uint64_t counter, int64_t* actions, float* q_pi, float* q_star,
                      int64_t* greedy, hipStream_t st);
hipError_t launch_nstep(const float* rew, const uint8_t* done, const float* q_pi, const float* q_star, long long K,
                        int W, int n_step, float gamma, float* targets, float* prio, hipStream_t st);
// part: [cdiv(N, 256)][4] scratch
hipError_t launch_loss_head(const float* adv, const float* v, const int64_t* act, const float* taus,
                            const float* tgt, const float* prob, int N, int Ws, int Wt, int A, float kappa,
                            float beta, float* dadv, float* dv, float* prio, float* part, float* metrics4,
                            hipStream_t st);

}  // namespace iqn_dev
