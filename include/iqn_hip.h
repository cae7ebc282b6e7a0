/* iqn_hip.h — C-ABI of the MI355X-native distributional (IQN) Ape-X agent: the actor path and the
 * learner's training step (in libimpala_hip.so).
 *
 * The reference's distributional Ape-X variant (paths relative to the d3sm0/impala repository):
 *
 *   iqn_forward        models/models.py:90-101  DistributionalAtariNetwork.forward and
 *                      models/quantile_layers.py:7-54  ImplicitQuantileHead / QuantileLayer
 *                      (online or target net)
 *   iqn_act            models/distributed_models.py:47-66  DistributionalAtariDQN.act
 *   iqn_sync_target    models/distributed_models.py:68-69  sync_target_net
 *   iqn_nstep_targets  agents/dqn/learning.py:69-84  ApexDistributionalActor._make_replay: the
 *                      per-quantile n-step targets and the initial priorities of one rollout
 *   iqn_loss_head      agents/dqn/learning.py:203-216  DistributionalApex._train_step's loss on
 *                      given heads and models/quantile_layers.py:83-93  quantile_regression_loss
 *                      (test / reuse entry)
 *   iqn_train_step     agents/dqn/learning.py:197-237  DistributionalApex._train_step: forward of the
 *                      online net, the importance-weighted quantile-regression loss, the backward
 *                      through heads, projection, LayerNorm, modulation, quantile layer and conv
 *                      trunk, clip_grad_norm_ and Adam; iqn_compute_grads stops before the clip
 *   iqn_replay_*       the learner's replay (agents/dqn/builder.py:124-156 builds rlmeta's ReplayBuffer
 *                      with a PrioritizedSampler) as a ring in HBM whose target rows are W floats
 *                      wide: dqn_replay (dqn_hip.h) with targets [capacity][W], the same sampler
 *   iqn_replay_extend_rollout  agents/dqn/learning.py:69-84  the actor's whole rollout in one
 *                      pass: iqn_nstep_targets' numbers written at their ring rows
 *   iqn_train_step_replay  sample, gather, iqn_train_step and the priority update as one call
 *
 * Network, for n frames and W = n_tau quantiles per frame (R = n W rows, row r = f W + k):
 *   x_f = AtariBody(obs_f / 255); e_r[i] = cos(pi i tau_r), i = 1..64, the argument formed in fp32
 *   as (pi * i) * tau; phi_r = GELU(Wq e_r + bq); y_r = LayerNorm(x_f * phi_r);
 *   h_r = GELU(Wfc y_r + bfc); q = v + adv - mean_A(adv).
 *
 * Parameters are one flat fp32 buffer per net in torch `parameters()` order:
 *   body.body.{0,2,4}.{weight,bias}, q.quantile_layer.output_layer.0.{weight,bias},
 *   q.project.0.{weight,bias} (LayerNorm), q.project.1.{weight,bias}, q.q.{weight,bias},
 *   q.v.{weight,bias}
 * i.e. the dueling net's layout (dqn_hip.h) with 66,560 floats inserted before the LayerNorm.
 *
 * taus: every entry point that runs the net takes explicit taus (device, [n][W]) or NULL.  With
 * NULL the library draws u = (mix(mix(seed ^ mix(counter)) + ((1 + which) << 32) + r) >> 40) 2^-24
 * for row r, mix = splitmix64's finaliser, which = 0 online / 1 target: an index range disjoint
 * from the action draw's (frame < 2^32) under the same (seed, counter).
 *
 * Conventions as impala_hip.h / dqn_hip.h: plain device pointers, `stream` = hipStream_t as void*,
 * 0 = success else a hipError_t or IMPALA_E_* code with iqn_last_error() (the library's one
 * last-error slot per thread) describing it.
 */
#ifndef IQN_HIP_H_
#define IQN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "impala_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQN_ABI_VERSION 3

#define IQN_HIDDEN 512
#define IQN_COS 64 /* cosine features of a quantile */
#define IQN_MAX_ACTIONS 15
#define IQN_MAX_TAU 32
#define IQN_MAX_ROWS 16384 /* batch_size * n_tau */
#define IQN_MAX_NSTEP 16   /* = DQN_REPLAY_MAX_NSTEP */

typedef struct iqn_learner iqn_learner;

typedef struct iqn_config {
  int batch_size;  /* the most frames of one iqn_forward / iqn_act call */
  int num_actions; /* 1..15 (iqn_act needs >= 2) */
  int n_tau;       /* W quantiles per frame, 1..32 (conf/agent/apex.yaml n_tau_samples: 8) */
  int dtype;       /* IMPALA_DTYPE_F32 / IMPALA_DTYPE_BF16 */
} iqn_config;

/* Optimizer and loss settings of the training step (iqn_bind_state); iqn_config keeps the shapes. */
typedef struct iqn_optim {
  float lr;                           /* 6.25e-5 */
  float adam_beta1, adam_beta2;       /* 0.9, 0.999 */
  float adam_eps;                     /* 1e-4 */
  float max_grad_norm;                /* 40 */
  float importance_sampling_exponent; /* 0.4 */
  float huber_param;                  /* kappa of the quantile Huber loss: 1 (0: |delta|) */
} iqn_optim;

/* One training batch of exactly batch_size transitions (device pointers). */
typedef struct iqn_batch {
  const uint8_t* obs;         /* [N][3][64][64], 16-byte aligned */
  const int64_t* actions;     /* [N] */
  const float* targets;       /* [N][W] */
  const float* probabilities; /* [N] sampling probabilities, or NULL (weights 1) */
  const float* taus;          /* [N][W] the online net's quantiles, or NULL: drawn from seed / counter */
  float* priorities;          /* [N] out: |mean_j target - mean_i q| */
  float* taus_out;            /* [N][W] out, optional: the taus used */
  uint64_t seed, counter;     /* the draw's key when taus is NULL (which = 0, as iqn_forward) */
} iqn_batch;

/* Debug tensors of the training step beyond impala_hip.h's ids (iqn_debug_read). */
#define IQN_DBG_DPRE 100 /* [R][1024] compute type: d loss / d (Wq e + bq), kernel order p*64+c */
#define IQN_DBG_DX 101   /* [N][1024] fp32: d loss / d act3 (ReLU mask applied), kernel order */
#define IQN_DBG_COS 102  /* [R][64] compute type: the cosine tile e */

int iqn_abi_version(void);
const char* iqn_last_error(void);
int iqn_config_default(iqn_config* cfg);
/* parameters of one net (the online net alone): 677,552 for A = 15 */
size_t iqn_param_count(int num_actions);

/* Invalid configurations (n_tau outside [1, 32], num_actions outside [1, 15], batch_size < 1 or
 * batch_size * n_tau > IQN_MAX_ROWS, unknown dtype) are refused before any HIP call. */
int iqn_create(const iqn_config* cfg, int device, iqn_learner** out);
int iqn_destroy(iqn_learner* h);

/* The two nets' flat fp32 [iqn_param_count] buffers (caller-owned); emits their kernel-layout
 * weights. */
int iqn_bind_params(iqn_learner* h, float* online, float* target, void* stream);
/* target <- online: the flat parameters and the kernel-layout weights (device copies). */
int iqn_sync_target(iqn_learner* h, void* stream);
/* Re-emit both nets' kernel-layout weights after the caller wrote the flat buffers. */
int iqn_refresh_weights(iqn_learner* h, void* stream);

/* q [n][W][A] of n <= batch_size frames; which: 0 online net, 1 target net.  taus [n][W] or NULL
 * (drawn from seed / counter, above); taus_out [n][W], optional, receives the taus used. */
int iqn_forward(iqn_learner* h, const uint8_t* obs, int n, int which, const float* taus,
                uint64_t seed, uint64_t counter, float* q, float* taus_out, void* stream);
/* DistributionalAtariDQN.act on n <= batch_size frames: qbar = mean_k q_online[f][k][:] (summed
 * k = 0..W-1, then divided by W), greedy = first maximal index of qbar, the action drawn as dqn_act
 * draws it (1 - eps on greedy, eps / (A - 1) elsewhere, keyed by (seed, counter, frame)); eps [n] per
 * frame, or NULL for eps_all.  actions [n] int64, q_pi [n] = qbar[action], q_star [n][W] =
 * q_target[f][k][greedy] from a forward through the target net with its own taus; greedy [n]
 * (int64, optional). */
int iqn_act(iqn_learner* h, const uint8_t* obs, int n, const float* eps, float eps_all,
            uint64_t seed, uint64_t counter, const float* taus_online, const float* taus_target,
            int64_t* actions, float* q_pi, float* q_star, int64_t* greedy, void* stream);

/* One rollout of L >= 2 steps -> L - 1 transitions: targets [L-1][W], column k the n-step return
 * dqn_replay_extend_rollout defines (same fp32 nesting, one FMA per term) with v_t =
 * q_star[t+1][k]; priorities [L-1] = |mean_k target[t][k] - q_pi[t]|, the mean a k-ordered fp32 sum
 * divided by W.  rewards [L], done [L] (uint8), q_pi [L], q_star [L][W].  1 <= W <= IQN_MAX_TAU,
 * 1 <= n_step <= IQN_MAX_NSTEP. */
int iqn_nstep_targets(const float* rewards, const uint8_t* done, const float* q_pi,
                      const float* q_star, int64_t L, int W, int n_step, float gamma,
                      float* targets, float* priorities, void* stream);

/* The quantile-regression loss alone on adv [N][Ws][A], v [N][Ws], actions [N], taus [N][Ws],
 * targets [N][Wt], probabilities [N] or NULL (w = 1):
 *   q[n][i] = dueling q at actions[n]; delta = target[n][j] - q[n][i]; rho = |tau[n][i] - 1[delta < 0]|
 *   L_n = (1 / Wt) sum_j sum_i rho huber_kappa(delta)   (kappa = 0: |delta|)
 *   loss = mean_n(w_n L_n), w_n = p_n^-beta / max_batch
 * -> dadv [N][Ws][A], dv [N][Ws] (d loss / d heads; at an exact tie delta = 0 the kappa = 0
 * gradient is 0), priorities [N] = |mean_j target - mean_i q|, metrics4 = {mean q, mean target,
 * mean priorities, loss}.  1 <= Ws, Wt <= IQN_MAX_TAU.  No atomics: bitwise reproducible. */
int iqn_loss_head(const float* adv, const float* v, const int64_t* actions, const float* taus,
                  const float* targets, const float* probabilities, int N, int Ws, int Wt, int A,
                  float huber_param, float beta, float* dadv, float* dv, float* priorities,
                  float* metrics4, void* stream);

/* The defaults of dqn_config_default and huber_param = 1. */
int iqn_optim_default(iqn_optim* optim);
/* Training state of the online net, caller-owned flat fp32 [iqn_param_count] buffers in the IQN flat
 * order (`parameters()` order: Wq, bq between the conv trunk and the LayerNorm): params (it becomes
 * the online net of iqn_bind_params), grads, exp_avg, exp_avg_sq, and metrics [IMPALA_NUM_METRICS].
 * optim NULL: iqn_optim_default.  Allocates the step's workspace on the first call and emits the
 * online net's kernel-layout weights.  The target net is bound by iqn_bind_params. */
int iqn_bind_state(iqn_learner* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                   float* metrics, const iqn_optim* optim, void* stream);
/* Point the following steps' metrics at another [IMPALA_NUM_METRICS] device vector. */
int iqn_set_metrics(iqn_learner* h, float* metrics);
/* Set the Adam step counter (0 after iqn_create); synchronises `stream`. */
int iqn_set_step(iqn_learner* h, int64_t step, void* stream);
/* One learner step on `b`: loss L = mean_f w_f l_f with l_f iqn_loss_head's L_n on the online net's
 * own heads (Ws = Wt = n_tau) and w_f = p_f^-beta / max_batch; gradient of every parameter into
 * grads (pre-clip values scaled by the clip coefficient, as torch leaves them), clip to
 * max_grad_norm over all parameters, Adam, the kernel-layout weights re-emitted.  metrics: [0] mean
 * q, [1] mean target, [2] mean priorities, [3] loss, [6] gradient norm before the clip, [7] the
 * step count.  Every sum runs in a fixed order without atomics: equal inputs give equal bits. */
int iqn_train_step(iqn_learner* h, const iqn_batch* b, void* stream);
/* iqn_train_step without clip and Adam: the pre-clip gradient in grads, priorities, metrics 0..3;
 * the step counter advances.  iqn_apply_update then completes the step, bit for bit. */
int iqn_compute_grads(iqn_learner* h, const iqn_batch* b, void* stream);
int iqn_apply_update(iqn_learner* h, void* stream);

/* Test / inspection entry: the workspace tensor `which` (IMPALA_DBG_*, impala_hip.h) as the last
 * iqn_forward / iqn_act left it, copied to dst (device or host) on `stream`.  act1, act2, act3
 * and mask1 are the conv trunk's, per frame (impala_debug_read on the handle's core); y, zg, h
 * and heads are the quantile head's, per row r = f W + k ([R][1024] of the compute type,
 * [R][512] fp32, [R][512] of the compute type, [R][16] fp32), and `bytes` reads their leading
 * rows: in (0, batch_size * n_tau rows].  Both nets run through the one workspace: it holds the
 * net that ran last.  After a training step also: IMPALA_DBG_LNSTAT [R][2] (mean, rstd of the
 * modulated features), IQN_DBG_COS, IMPALA_DBG_DZ [R][512] compute type, IMPALA_DBG_DY [R][1024]
 * fp32, IQN_DBG_DPRE, IQN_DBG_DX, and the trunk's IMPALA_DBG_DACT3 / IMPALA_DBG_DACT2 per frame.
 * Every other id is refused. */
int iqn_debug_read(iqn_learner* h, int which, void* dst, size_t bytes, void* stream);

/* ---- the learner's replay, device-side: dqn_replay (dqn_hip.h) with W targets per transition ----
 *
 * A ring of `capacity` transitions (obs u8 [3][64][64], action i64, targets f32 [W], W = n_tau)
 * with a priority per transition, in caller-owned device arrays (iqn_replay_bind); the library
 * owns the float64 weights, their block sums, the running maximum priority, size and cursor.
 * Sampling, the priority update, the weights invariant and the running maximum are dqn_replay's
 * contract word for word, computed by the same kernels: weights[i] == (double)priorities[i] **
 * priority_exponent for every written row after every entry point below; draw j of a call is keyed
 * by (seed, counter, j) exactly as dqn_replay_sample's.  Refused before any HIP call, in this
 * order: bad scalars (n_tau outside [1, IQN_MAX_TAU], capacity outside [1, 2097152], a non-finite or
 * negative exponent, n < 1, L < 2, n_step outside [1, 16], gamma outside [0, 1]), then a null
 * pointer (named), obs / obs_out not 16-byte aligned and sample's three outputs not all or none,
 * then a null handle; n > capacity and L - 1 > capacity need the handle and follow it. */
typedef struct iqn_replay iqn_replay;

int iqn_replay_create(int64_t capacity, int n_tau, double priority_exponent, int device,
                      iqn_replay** out);
int iqn_replay_destroy(iqn_replay* r);
/* The ring's arrays: obs [capacity][3][64][64] (16-byte aligned), actions [capacity], targets
 * [capacity][W], priorities [capacity].  Empties the ring; the running maximum restarts at 1. */
int iqn_replay_bind(iqn_replay* r, uint8_t* obs, int64_t* actions, float* targets, float* priorities,
                    void* stream);
int iqn_replay_state(const iqn_replay* r, int64_t* size, int64_t* cursor);
/* n transitions appended at the cursor, across the wrap: targets [n][W]; priorities [n], or NULL:
 * every row takes the running maximum.  keys_out [n], optional: the ring rows written. */
int iqn_replay_extend(iqn_replay* r, const uint8_t* obs, const int64_t* actions, const float* targets,
                      const float* priorities, int64_t n, int64_t* keys_out, void* stream);
/* One rollout of L steps -> L - 1 transitions appended at the cursor.  Targets [L-1][W] and
 * priorities [L-1] are bit for bit what iqn_nstep_targets returns on the same inputs (q_pi [L],
 * q_star [L][W]), computed and written to the ring rows (cursor + t) % capacity, with actions and
 * weights, by one launch; the running maximum is raised afterwards. */
int iqn_replay_extend_rollout(iqn_replay* r, const uint8_t* obs, const int64_t* actions,
                              const float* rewards, const uint8_t* done, const float* q_pi,
                              const float* q_star, int64_t L, int n_step, float gamma,
                              int64_t* keys_out, void* stream);
/* n draws with replacement: keys [n], probabilities [n]; obs_out [n][3][64][64], actions_out [n],
 * targets_out [n][W]: the gathered rows, all three or none. */
int iqn_replay_sample(iqn_replay* r, uint64_t seed, uint64_t counter, int64_t n, int64_t* keys,
                      float* probabilities, uint8_t* obs_out, int64_t* actions_out, float* targets_out,
                      void* stream);
/* priorities[keys[j]] = priorities_in[j], n <= DQN_MAX_BATCH (4096) keys per call; duplicate keys
 * keep the invariant (dqn_replay_update). */
int iqn_replay_update(iqn_replay* r, const int64_t* keys, const float* priorities, int64_t n,
                      void* stream);
/* A copy of the float64 weights [capacity] and, optionally, of the running maximum priority. */
int iqn_replay_weights(iqn_replay* r, double* weights_out, float* max_priority_out, void* stream);
/* One learner step from the replay, enqueued on `stream` with no host synchronisation: batch_size
 * draws keyed by (seed, counter), their rows gathered into a library-owned batch buffer, exactly
 * iqn_train_step's work on that batch, then the priority update at the drawn keys -- bitwise
 * iqn_replay_sample + iqn_train_step + iqn_replay_update.  taus [N][W], or NULL: the online net's
 * quantiles drawn from (tau_seed, tau_counter) as iqn_batch.seed / counter do.  keys_out [N],
 * priorities_out [N], taus_out [N][W], each optional, take the results directly.  A batch of more
 * than DQN_MAX_BATCH keys (possible at small n_tau) is updated in chunks of DQN_MAX_BATCH, in
 * order.  Refused before any launch: null handles, iqn_bind_state not called, iqn_replay_bind not
 * called, a replay whose n_tau is not the learner's or on another device, an empty replay
 * (IMPALA_E_STATE). */
int iqn_train_step_replay(iqn_learner* h, iqn_replay* r, uint64_t seed, uint64_t counter,
                          const float* taus, uint64_t tau_seed, uint64_t tau_counter,
                          int64_t* keys_out, float* priorities_out, float* taus_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* IQN_HIP_H_ */
