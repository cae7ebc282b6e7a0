/* dqn_hip.h — C-ABI of the MI355X-native Ape-X DQN learner (in libimpala_hip.so).
 *
 * SURVEY.md §2, the reference's fourth agent (paths relative to the d3sm0/impala repository):
 *
 *   dqn_train_step   agents/dqn/learning.py:159-176  ApexLearner._train_step after the replay
 *                    sample: forward, importance-weighted squared TD error, backward,
 *                    clip_grad_norm_(max_grad_norm), Adam, and the new priorities |err|
 *   dqn_forward      models/models.py:79-87  DuellingAtariNetwork.forward (online or target net)
 *   dqn_act          models/distributed_models.py:84-101  AtariDQNModel.act
 *   dqn_sync_target  models/distributed_models.py:103-104  sync_target_net
 *   dqn_loss_head    the loss alone, on given advantage / value heads (test / reuse entry)
 *
 * Network: AtariBody -> LayerNorm(1024) -> Linear(1024, 512) -> GELU -> advantage head
 * Linear(512, A) and value head Linear(512, 1); q = v + adv - mean_A(adv).  The trunk up to the
 * LayerNorm is IMPALA's; the projection is 512 wide.
 *
 * Parameters are one flat fp32 buffer per net in torch `parameters()` order:
 *   body.body.{0,2,4}.{weight,bias}, q.body.0.{weight,bias} (LayerNorm), q.body.1.{weight,bias},
 *   q.q.{weight,bias}, q.v.{weight,bias}
 * (online_net.* and, with the same layout, target_net.*).
 *
 * Conventions as impala_hip.h: plain device pointers, `stream` = hipStream_t as void*,
 * 0 = success else a hipError_t or IMPALA_E_* code with dqn_last_error() (the library's one
 * last-error slot per thread) describing it.  A handle takes one device (no data-parallel DQN).
 */
#ifndef DQN_HIP_H_
#define DQN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "impala_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DQN_ABI_VERSION 1

/* metric slots (names as agents/dqn/learning.py:185-190); slots 4, 5 and 8 are written as 0 */
#define DQN_M_Q 0
#define DQN_M_TARGET 1
#define DQN_M_PRIORITIES 2
#define DQN_M_LOSS 3
#define DQN_M_GRAD_NORM 6
#define DQN_M_STEP 7
#define DQN_NUM_METRICS 9

#define DQN_HIDDEN 512
#define DQN_MAX_ACTIONS 15
#define DQN_MAX_BATCH 4096

typedef struct dqn_learner dqn_learner;

typedef struct dqn_config {
  int batch_size;   /* N transitions per step, 1..DQN_MAX_BATCH; also the most frames of one
                       dqn_forward / dqn_act call */
  int num_actions;  /* 1..15 (dqn_act needs >= 2) */
  int dtype;        /* IMPALA_DTYPE_F32 / IMPALA_DTYPE_BF16 */
  float lr, adam_beta1, adam_beta2, adam_eps; /* conf/agent/apex.yaml: 6.25e-5, 0.9, 0.999, 1e-4 */
  float max_grad_norm;                        /* 40 */
  float importance_sampling_exponent;         /* beta, 0.4 */
} dqn_config;

typedef struct dqn_batch {
  const uint8_t* obs;         /* [N][3][64][64], 16-byte aligned */
  const int64_t* actions;     /* [N] in [0, A) */
  const float* targets;       /* [N] n-step targets, computed by the actor */
  const float* probabilities; /* [N] sampling probabilities (any positive scale), or NULL: w = 1 */
  float* priorities;          /* [N] out: |target - q[a]| */
} dqn_batch;

int dqn_abi_version(void);
const char* dqn_last_error(void);
int dqn_config_default(dqn_config* cfg);
/* parameters of one net (the online net alone): 610,992 for A = 15 */
size_t dqn_param_count(int num_actions);

/* Invalid configurations are refused before any HIP call. */
int dqn_create(const dqn_config* cfg, int device, dqn_learner** out);
int dqn_destroy(dqn_learner* h);

/* Caller-owned state: flat fp32 [dqn_param_count] buffers and a DQN_NUM_METRICS-float metrics
 * vector.  grads / exp_avg / exp_avg_sq / metrics may be NULL for an inference-only handle.
 * Emits the online net's kernel-layout weights. */
int dqn_bind_state(dqn_learner* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                   float* metrics, void* stream);
/* The target net's flat parameters (caller-owned); emits its kernel-layout weights. */
int dqn_bind_target(dqn_learner* h, float* target_params, void* stream);
/* target <- online: the flat parameters and the kernel-layout weights (device copies). */
int dqn_sync_target(dqn_learner* h, void* stream);
/* Re-emit both nets' kernel-layout weights after the caller wrote the flat buffers. */
int dqn_refresh_weights(dqn_learner* h, void* stream);
int dqn_set_step(dqn_learner* h, int64_t step, void* stream);
int dqn_set_metrics(dqn_learner* h, float* metrics);
/* As impala_set_metrics_host: a 16-float page-locked host row the step's metrics also go to. */
int dqn_set_metrics_host(dqn_learner* h, float* host);

/* q [n][A] of n <= batch_size frames; which: 0 online net, 1 target net. */
int dqn_forward(dqn_learner* h, const uint8_t* obs, int n, int which, float* q, void* stream);
/* AtariDQNModel.act on n <= batch_size frames: eps [n] per frame, or NULL for eps_all.
 * actions [n] int64, q_pi [n] = q_online[action], q_star [n] = q_target[greedy]; greedy [n]
 * (int64, optional) = argmax q_online.  The draw is keyed by (seed, counter, frame). */
int dqn_act(dqn_learner* h, const uint8_t* obs, int n, const float* eps, float eps_all,
            uint64_t seed, uint64_t counter, int64_t* actions, float* q_pi, float* q_star,
            int64_t* greedy, void* stream);

int dqn_train_step(dqn_learner* h, const dqn_batch* batch, void* stream);

/* The loss alone on adv [N][A], v [N]: d loss / d adv [N][A], d loss / d v [N], the new
 * priorities [N] and metrics4 = {q, target, priorities, loss}.  probabilities may be NULL.
 * Handle-free, as impala_ppo_loss_head: it runs on the calling thread's current device and takes
 * its scratch from the stream's memory pool (hipMallocAsync). */
int dqn_loss_head(const float* adv, const float* v, const int64_t* actions, const float* targets,
                  const float* probabilities, int N, int A, float importance_sampling_exponent,
                  float* dadv, float* dv, float* priorities, float* metrics4, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DQN_HIP_H_ */
