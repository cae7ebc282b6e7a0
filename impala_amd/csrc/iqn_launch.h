// Launchers of the IQN kernels (csrc/iqn.hip), called by the host side in csrc/iqn.h.  Each
// enqueues its kernels on `st` and returns hipGetLastError() of the first launch that failed.
// The kernels are compiled in a translation unit of their own so that impala.hip's code object
// stays what it is without them.  `bf16` picks the compute type T of the untyped pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adam_args.h"

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

// ---- the training step (DistributionalApex._train_step) ----
// iqn_head_step_kernel: dqn_head_step.h's DqnHeadArgs over R = N W quantile rows
struct HeadStepArgs {
  const void* h;       // T [R][512]
  const float* zg;     // [R][512] gelu'(pre-GELU), from the FC forward
  const void* wh;      // T [16][512]
  const void* wht;     // T [512][32]
  const float* bh;     // [16]
  const int64_t* act;  // [N]
  const float* taus;   // [R]
  const float* tgt;    // [N][W]
  const float* prob;   // [N] sampling probabilities, or null (w = 1)
  int N, W, R, A;
  float beta, kappa;
  void* dz;         // T [R][512]
  float* heads;     // [R][16]: the heads output the loss read
  float* partials;  // [gridDim.x][8]: sums of mean_i q, mean_j target, priorities, w L
  float* slab_h;    // [gridDim.x][16][512]
  float* slab_bh;   // [gridDim.x][16]
  float* prio;      // [N] out
};
struct LnModBwdArgs {
  const void* e;       // T [R][64] cosine tile
  const void* act3;    // T [N][1024]
  const void* wq;      // T [1024][64]
  const float* bq;     // [1024]
  const float* gam;    // [1024]
  const float* stats;  // [R][2] mean, rstd
  const float* dy;     // [R][1024]
  void* dpre;          // T [R][1024]
  float* dx;           // [N][1024]
  float* slab;         // [gridDim.x][2][1024]
  int N, W, fpw;       // fpw: frames per workgroup
};
struct RedInsArgs {
  const float* s_wq;  // [S][1024][64]
  const float* s_bq;  // [S][1024]
  int S;
  float* grads_ins;  // the flat gradient's inserted segment: Wq (canonical rows), then bq
  float* sumsq;      // [ins_wgs()] clip-norm partials
  const float* loss_part;
  int n_loss_part, N;
  float* metrics;
  int64_t* step;
  double lr, b1, b2;
  float* adam_sc;
};
// what the step past the trunk's forward reads and writes (device pointers; T by `bf16`)
struct StepWork {
  HeadWeights w;     // the online net
  const void* wht;   // T [512][32]
  HeadWork fw;       // y, zg, h, heads
  float* stats;      // [R][2]
  void* e;           // T [R][64]
  void* dz;          // T [R][512]
  float* dy;         // [R][1024]
  void* dpre;        // T [R][1024]
  float* dx;         // [N][1024]
  float *s_ln, *s_fc, *s_bfc, *s_h, *s_bh, *s_wq, *s_bq, *loss_part;
  int fc_S, fc_mps, wq_S, wq_mps;  // split plans of the two weight-gradient GEMMs over R rows
  int ln_fpw, ln_wgs;              // iqn_ln_mod_bwd_kernel: frames per workgroup, workgroups
};
// the trunk's per-frame backward from dx (lnc3_conv12_bwd_dx): the core handle's tensors
struct TrunkBwd {
  const void *act3, *w3, *w3t, *act2, *w2, *w2t;
  void *dact3, *dact2;
  const uint8_t* obs;
  const uint32_t* mask1;
  float *s_w1, *s_b1;
  int fpw, wgs;
  // the conv3 / conv2 weight gradients after it (wgrad23_kernel): act1, the slabs, the split plans
  const void* act1;
  float *s_w3, *s_b3, *s_w2, *s_b2;
  int S3, mps3, S2, mps2;
};
struct AdamIns {
  AdamArgs a;  // on the core's Canon, with the caller's IQN-order buffers
  FlatGap fm;  // where the Canon's indices lie in them
  void* wq;    // the online net's kernel-layout Wq (T), bq: re-emitted
  float* bq;
  int grid;    // adam_kernel's grid on the core's Canon
};
int head_step_wgs(int N, int W);  // workgroups (x) of iqn_head_step_kernel = its slabs / partials
int ins_wgs();                    // workgroups of iqn_reduce_ins_kernel = its clip-norm partials
// training forward past act3 (embed + LayerNorm keeping statistics and the cosine tile, FC), the
// head step, the FC backward, the LayerNorm / modulation backward, the Wq gradient, the trunk's
// per-frame backward and the conv3 / conv2 weight gradients, in this order on `st`
hipError_t launch_step(bool bf16, const StepWork& s, const TrunkBwd& tb, const float* taus, const int64_t* act,
                       const float* tgt, const float* prob, float* prio, int N, int W, int A, float beta,
                       float kappa, int n_cu, hipStream_t st);
hipError_t launch_reduce_ins(const RedInsArgs& a, int fin, hipStream_t st);
hipError_t launch_adam(bool bf16, const AdamIns& a, hipStream_t st);

}  // namespace iqn_dev
