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
 *   dqn_replay_*     agents/dqn/builder.py:82-89  the rlmeta ReplayBuffer + PrioritizedSampler the
 *                    builder makes: dqn_replay_extend = ReplayBuffer.extend
 *                    (agents/dqn/learning.py:65), dqn_replay_sample = ReplayBuffer.sample
 *                    (learning.py:141), dqn_replay_update = async_update_priorities
 *                    (learning.py:178-182)
 *   dqn_replay_extend_rollout  agents/dqn/learning.py:56-65  ApexActor._async_make_replay: the
 *                    n-step targets and initial priorities of one rollout, appended to the ring
 *   dqn_train_step_replay      agents/dqn/learning.py:139-147,159-182  sample, step and priority
 *                    update as one call
 *   dqn_train_step_replay_rows  the same, the step reading the sampled ring rows in place
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

#define DQN_ABI_VERSION 2

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
/* dqn_train_step without clip and Adam: the pre-clip gradient in the bound grads, the priorities
 * and metrics q / target / priorities / loss; the parameters, the Adam state and the metrics
 * grad_norm / step stay as they are.  (dqn_train_step leaves the CLIPPED gradient in grads: the
 * Adam kernel writes g * min(1, max_grad_norm / norm) back.) */
int dqn_compute_grads(dqn_learner* h, const dqn_batch* batch, void* stream);

/* Test / inspection entry: impala_debug_read on the DQN handle's workspace, as the last forward,
 * act or step left it -- the IMPALA_DBG_* ids and layouts, h / dz / zg DQN_HIDDEN wide.  The one
 * workspace serves both nets (it holds the net that ran last); net = 1 differs from net = 0 only
 * for IMPALA_DBG_HEADS, which then reads the target net's own heads buffer.  The step keeps its
 * heads in LDS: IMPALA_DBG_HEADS holds what the last dqn_forward / dqn_act wrote. */
int dqn_debug_read(dqn_learner* h, int net, int which, void* dst, size_t bytes, void* stream);

/* The loss alone on adv [N][A], v [N]: d loss / d adv [N][A], d loss / d v [N], the new
 * priorities [N] and metrics4 = {q, target, priorities, loss}.  probabilities may be NULL.
 * Handle-free, as impala_ppo_loss_head: it runs on the calling thread's current device and takes
 * its scratch from the stream's memory pool (hipMallocAsync). */
int dqn_loss_head(const float* adv, const float* v, const int64_t* actions, const float* targets,
                  const float* probabilities, int N, int A, float importance_sampling_exponent,
                  float* dadv, float* dv, float* priorities, float* metrics4, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prioritized replay on the device (rlmeta ReplayBuffer + PrioritizedSampler as
 * agents/dqn/builder.py:82-89 builds them).
 *
 * Ownership: the caller owns the ring arrays obs u8 [cap][3][64][64] (16-byte aligned), actions
 * i64 [cap], targets f32 [cap], priorities f32 [cap]; the library owns the sampling state:
 * weights f64 [cap], one f64 sum per block of DQN_REPLAY_BLOCK rows, the running maximum priority
 * (a device scalar, initially 1) and a gather buffer for one batch (allocated by the first
 * dqn_train_step_replay).  Cursor and size live on the host.  Invariant, for every row i written
 * since dqn_replay_bind (i < size):
 *   weights[i] == pow((double)priorities[i], priority_exponent)      (the exponent is a double)
 * (at priority_exponent == 1 the priority itself, exactly: the device pow(x, 1.0) is not always x)
 * kept where a priority is written (extend, extend_rollout, update); a sample calls no pow.
 * dqn_replay_bind zeroes the weights and leaves the caller's arrays as they are; a sample never
 * reads rows >= size.
 * Priorities are expected finite and >= 0.  A replay serves one host thread and one stream at a
 * time, as every handle of this library does.
 *
 * The sampling contract (tests/dqn_replay_oracle.py restates it in numpy):
 *   mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)      (mod 2^64)
 *   draw     u_j = (mix(mix(seed ^ mix(counter)) + j) >> 11) * 2^-53 -- keyed as dqn_act keys
 *            (seed, counter, frame)
 *   prefix   C_i = the inclusive float64 prefix sum of weights[0 .. size)
 *   key      keys[j] = the smallest i with C_i > u_j * C_{size-1}
 *   prob.    probabilities[j] = (float)(weights[keys[j]] / C_{size-1})
 *   zero total (every stored priority 0): keys[j] = floor(u_j * size), probabilities[j] = 1/size
 *   a row of weight 0 is never drawn while the total is positive: where rounding leaves no i with
 *   C_i > u_j * C_{size-1} the key is the last row of positive weight (the contract's clamp to
 *   size - 1, kept off zero-weight rows).
 * The kernels sum in a fixed order that is not numpy's (per block: 8 consecutive rows per lane,
 * then the lanes in order; the block sums in chunks, then the chunks in order), so C_i differs
 * from a sequential sum by float64 rounding: keys agree with the restatement whenever
 * u_j * C_{size-1} is not within rounding of a prefix boundary.  Results are bitwise reproducible
 * run to run (no atomics).
 *
 * N-step targets (dqn_replay_extend_rollout): rlax's n_step_bootstrapped_returns with lambda = 1
 * (rewards padded with 0 and discounts with 1 past the end).  rlego, which the reference calls, is
 * absent: parity with it is unpinned, as for V-trace.
 * ------------------------------------------------------------------------------------------ */
#define DQN_REPLAY_BLOCK 512
#define DQN_REPLAY_MAX_NSTEP 16

typedef struct dqn_replay dqn_replay;

/* rows per block sum: DQN_REPLAY_BLOCK */
int dqn_replay_block(void);
/* 1 <= capacity <= 4096 * DQN_REPLAY_BLOCK (2,097,152); priority_exponent (alpha) finite and >= 0 */
int dqn_replay_create(int64_t capacity, double priority_exponent, int device, dqn_replay** out);
int dqn_replay_destroy(dqn_replay* r);
/* Takes the caller's ring arrays and resets the replay: size 0, cursor 0, weights 0, maximum 1. */
int dqn_replay_bind(dqn_replay* r, uint8_t* obs, int64_t* actions, float* targets,
                    float* priorities, void* stream);
int dqn_replay_state(const dqn_replay* r, int64_t* size, int64_t* cursor);
/* ReplayBuffer.extend: n <= capacity rows of device data to rows (cursor + i) % capacity.
 * priorities NULL: every row gets the running maximum; given priorities raise it.
 * keys_out [n] i64 (optional): the rows written. */
int dqn_replay_extend(dqn_replay* r, const uint8_t* obs, const int64_t* actions,
                      const float* targets, const float* priorities, int64_t n, int64_t* keys_out,
                      void* stream);
/* ApexActor._async_make_replay on one rollout of L >= 2 steps (device arrays; done u8): appends
 * K = L - 1 transitions (obs[t], actions[t], target[t]) with priority |target[t] - q_pi[t]|.
 * With d_t = gamma * (1 - done[t]), v_t = q_star[t + 1], m = min(n_step, K - t):
 *   target[t] = r_t + d_t (r_{t+1} + d_{t+1} ( ... r_{t+m-1} + d_{t+m-1} v_{t+m-1}))
 * in fp32, innermost term first, each step one fused multiply-add (one rounding).
 * 1 <= n_step <= DQN_REPLAY_MAX_NSTEP, gamma in [0, 1]. */
int dqn_replay_extend_rollout(dqn_replay* r, const uint8_t* obs, const int64_t* actions,
                              const float* rewards, const uint8_t* done, const float* q_pi,
                              const float* q_star, int64_t L, int n_step, float gamma,
                              int64_t* keys_out, void* stream);
/* n draws with replacement by the contract above -> keys [n] i64, probabilities [n] f32 and, unless
 * all three are NULL, the gathered rows obs_out [n][3][64][64] (16-byte aligned), actions_out [n],
 * targets_out [n]. */
int dqn_replay_sample(dqn_replay* r, uint64_t seed, uint64_t counter, int64_t n, int64_t* keys,
                      float* probabilities, uint8_t* obs_out, int64_t* actions_out,
                      float* targets_out, void* stream);
/* priorities[keys[j]] = priorities_in[j] for n <= DQN_MAX_BATCH keys, the weights to match, and the
 * maximum raised.  With duplicate keys one of their values lands; the invariant holds either way. */
int dqn_replay_update(dqn_replay* r, const int64_t* keys, const float* priorities, int64_t n,
                      void* stream);
/* Sample batch_size rows into the replay's gather buffer, dqn_train_step on them, then
 * dqn_replay_update with the step's priorities: all enqueued on `stream`, no host synchronisation
 * (but the first call allocates the gather buffer).  keys_out / priorities_out [batch_size]
 * (optional, device) receive the sampled keys and the new priorities: the kernels write them
 * there directly. */
int dqn_train_step_replay(dqn_learner* h, dqn_replay* r, uint64_t seed, uint64_t counter,
                          int64_t* keys_out, float* priorities_out, void* stream);
/* dqn_train_step_replay without the gather: the same draws, then the step reads the sampled ring
 * rows in place -- the bound obs / actions / targets are its batch, transition f is ring row
 * keys[f] -- then dqn_replay_update.  Same arguments, checks and order of work, the same bits in
 * every output; no obs gather buffer is allocated (the first call allocates batch_size keys,
 * probabilities and priorities of scratch).  Everything is enqueued on `stream`, nothing waits on
 * the host.
 * Ownership: between this call and `stream` reaching its end the caller must not write the ring
 * rows (obs, actions, targets): the step's kernels read them after the call returns.  An extend
 * enqueued later on the same stream is ordered by the stream.
 * Only the default kernel path reads through the keys: a handle created under a switch that
 * leaves it (IMPALA_LC12=0, frames-per-workgroup overrides that differ or exceed 64) or a ring of
 * more than 2^31 - 1 rows gets IMPALA_E_UNSUPPORTED before any launch; dqn_train_step_replay
 * serves those. */
int dqn_train_step_replay_rows(dqn_learner* h, dqn_replay* r, uint64_t seed, uint64_t counter,
                               int64_t* keys_out, float* priorities_out, void* stream);
/* Test / inspection entry: copies weights [capacity] f64 and (optional) the running maximum f32
 * [1] into caller-owned device arrays. */
int dqn_replay_weights(dqn_replay* r, double* weights_out, float* max_priority_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DQN_HIP_H_ */
