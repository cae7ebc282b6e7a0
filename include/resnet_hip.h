/* resnet_hip.h — C-ABI of the MI355X-native IMPALA ResNet actor-critic: the actor path (forward and
 * act) and the backward pass of the reference's AtariActorCritic over ImpalaCNNLarge (in
 * libimpala_hip.so).
 *
 * The reference (paths relative to the d3sm0/impala repository):
 *   body        models/common.py:11-83   ResidualBlock, ImpalaCNNBlock, ImpalaCNNLarge
 *   projection  models/models.py:61-76   AtariActorCritic: LayerNorm, Linear + GELU, actor, critic
 *   act         models/distributed_models.py:21-32  AtariPPOModel.act
 *
 * Network, for n frames:
 *   x = obs_u8 / 255                                              [n][3][64][64]
 *   for (Cin, C, H) in (3,16,64), (16,32,32), (32,32,16):
 *     x = conv3x3_pad1(x; Cin->C) + b
 *     x = max_pool2d(x, kernel 3, stride 2, padding 1)            H -> H/2, padding -inf
 *     twice: t = conv3x3_pad1(relu(x)) + b; x = x + conv3x3_pad1(relu(t)) + b
 *   f = flatten_NCHW(relu(x))                                     [n][2048], index c*64 + y*8 + x
 *   y = LayerNorm(2048, eps 1e-5)(f); h = GELU_erf(Linear(2048, 256)(y))
 *   logits = Linear(256, A)(h); v = Linear(256, 1)(h)
 *
 * Parameters are one flat fp32 buffer in state_dict order:
 *   model.body.body.{0,1,2}.{conv,res_block0.conv0,res_block0.conv1,res_block1.conv0,
 *   res_block1.conv1}.{weight,bias}, model.projection.{0,1}.{weight,bias},
 *   model.actor.{weight,bias}, model.critic.{weight,bias}
 * 97,600 floats of body, 630,352 in all at A = 15.
 *
 * Conventions as iqn_hip.h: plain device pointers, `stream` = hipStream_t as void*, 0 = success
 * else a hipError_t or IMPALA_E_* code with resnet_last_error() (the library's one last-error slot
 * per thread) describing it.
 */
#ifndef RESNET_HIP_H_
#define RESNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "impala_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RESNET_ABI_VERSION 4

#define RESNET_FEATURES 2048
#define RESNET_HIDDEN 256
#define RESNET_MAX_ACTIONS 15
#define RESNET_BODY_PARAMS 97600

typedef struct resnet_actor resnet_actor;

typedef struct resnet_config {
  int batch_size;  /* the most frames of one resnet_forward / resnet_act call */
  int num_actions; /* 1..15 */
  int dtype;       /* IMPALA_DTYPE_F32 / IMPALA_DTYPE_BF16 */
  int debug;       /* 1: the trunk also stores its stage tensors (resnet_debug_read) */
  int train;       /* 1: the handle also holds, for batch_size frames, what resnet_forward_train saves and
                    *    the workspace of resnet_backward */
  int train_dtype; /* the type of resnet_forward_train / resnet_backward; train = 1 needs train_dtype == dtype
                    *    (resnet_forward_train is resnet_forward, the same bits).  Default fp32. */
} resnet_config;

/* Stage tensors of the last forward (resnet_debug_read), per frame.  The body's are channels-last
 * [H][H][C] of the compute type:
 *   0            x after the stem's pool                       [32][32][16]
 *   1..4         stage 1: t, x of res_block0, t, x of res_block1   [32][32][16]
 *   5, 6..9      stage 2: x after the pool, then t, x, t, x        [16][16][32]
 *   10, 11..14   stage 3: likewise                                 [8][8][32]
 * y [2048] of the compute type in the kernel order p*32 + c (p = y*8 + x; canonical c*64 + p),
 * h [256] of the compute type, heads [16] fp32 (logits 0..A-1, value at 15). */
#define RESNET_DBG_STAGES 15
#define RESNET_DBG_Y 15
#define RESNET_DBG_H 16
#define RESNET_DBG_HEADS 17
/* On a handle created with train = 1 (debug = 1 is not needed), after a resnet_backward, what the backward
 * computed and read; ids 0..17 are valid on such a handle too (as the last resnet_forward_train left them):
 *   32 + id      the gradient at convolution id's output (at its pool's output for 0, 5, 10): stage tensor
 *                id's layout, the compute type
 *   GY           the gradient at y [2048] fp32, kernel order;  GZ  at the pre-GELU z [256] fp32
 *   AMAX         the pools' winning taps, u8: [32][32][16], [16][16][32], [8][8][32] per frame
 *   LNSTAT       the LayerNorm's (mean, rstd) fp32 per frame
 *   PART         the projection's partial sums fp32, not per frame: the whole [8][batch_size][256] */
#define RESNET_DBG_GRAD0 32
#define RESNET_DBG_GY 47
#define RESNET_DBG_GZ 48
#define RESNET_DBG_AMAX 49
#define RESNET_DBG_LNSTAT 50
#define RESNET_DBG_PART 51
/* After a resnet_step_init, what resnet_loss_head left (rows of the step's B T frames, not batch_size):
 *   DLOGITS      d loss / d logits fp32 [B T][A];  DVALUES  d loss / d values fp32 [B T]
 *   TPART        per trajectory, 8 floats: the sums over its frames of log pi(a) adv and err^2 (the first
 *                T - 1), of the entropy, the KL term and rho (all T), then zeros: [B][8] */
#define RESNET_DBG_DLOGITS 52
#define RESNET_DBG_DVALUES 53
#define RESNET_DBG_TPART 54

int resnet_abi_version(void);
const char* resnet_last_error(void);
int resnet_config_default(resnet_config* cfg);
/* 630,352 for A = 15 */
size_t resnet_param_count(int num_actions);

/* Invalid configurations (batch_size < 1, num_actions outside [1, 15], unknown dtype, debug or train not
 * 0 / 1, train = 1 with train_dtype != dtype) are refused before any HIP call. */
int resnet_create(const resnet_config* cfg, int device, resnet_actor** out);
int resnet_destroy(resnet_actor* h);

/* The flat fp32 [resnet_param_count] buffer (caller-owned, device). */
int resnet_bind_params(resnet_actor* h, const float* flat);
/* Pack the flat parameters into the kernels' operand layouts (fragment-major weights of the
 * compute type, fp32 side vectors); call after bind and after every write to the flat buffer. */
int resnet_refresh_weights(resnet_actor* h, void* stream);

/* logits [n][A], values [n] of 1 <= n <= batch_size frames; obs [n][3][64][64] u8, 16-byte aligned. */
int resnet_forward(resnet_actor* h, const uint8_t* obs, int n, float* logits, float* values,
                   void* stream);
/* impala_act's semantics on this network: per frame argmax (first maximal index) where the
 * frame's deterministic flag is set (deterministic [n] u8, or NULL: deterministic_all), else a draw
 * from softmax(logits) on the uniform keyed by (seed, counter, frame).  actions [n] int64. */
int resnet_act(resnet_actor* h, const uint8_t* obs, int n, const uint8_t* deterministic,
               int deterministic_all, uint64_t seed, uint64_t counter, int64_t* actions,
               float* logits, float* values, void* stream);

/* Training (a handle created with train = 1), in fp32 or -- bf16 operands, saved tensors and gradients
 * between the layers, fp32 accumulation and fp32 grad_flat -- in bf16.  resnet_forward_train is resnet_forward -- the same bits --
 * and leaves in the handle what the backward reads: the 15 stage tensors, one byte per pooled element
 * naming the window's winning tap 0..8 (row-major; of equal values the first), the LayerNorm's mean and
 * rstd per frame, y, h and the projection's partial sums.
 * resnet_backward writes (accumulate = 0) or adds with one fp32 rounding per element (accumulate = 1) the
 * gradient of  sum dlogits * logits + sum dvalues * values  with respect to the flat parameters, in
 * their order, to grad_flat [resnet_param_count] fp32.  dlogits [n][A], dvalues [n] fp32; obs and n are
 * those of the handle's last resnet_forward_train, with no resnet_refresh_weights, resnet_forward or
 * resnet_act on the handle since: another n, no such call, or a train = 0 handle is IMPALA_E_INVALID
 * before any launch.  Sums over frames have one fixed order: equal inputs give equal bits. */
int resnet_forward_train(resnet_actor* h, const uint8_t* obs, int n, float* logits, float* values,
                         void* stream);
int resnet_backward(resnet_actor* h, const uint8_t* obs, int n, const float* dlogits,
                    const float* dvalues, float* grad_flat, int accumulate, void* stream);

/* The learner step (agents/impala/learning.py:140-177 on this network), on a handle created with
 * train = 1: the V-trace loss on the heads, the backward, clip_grad_norm_ and torch.optim.Adam (no weight
 * decay, no amsgrad) and the re-pack of the kernel-layout weights, all enqueued by one call.  The batch is
 * an impala_batch (impala_hip.h): obs u8 [B][T][3][64][64], actions i64 [B][T], rewards and discounts
 * fp32 [B][T], behaviour logits fp32 [B][T][A]; frame b T + t.  Metrics: the IMPALA_M_* vector
 * (IMPALA_M_TARGET zero).
 *
 *   resnet_step_init     B trajectories of T frames and the step's constants; allocates the step's
 *                        workspace (again on a second call) and zeroes the step count.  IMPALA_E_INVALID
 *                        before any HIP call unless 2 <= T <= 64, B >= 1, the gradient mode is an
 *                        IMPALA_VTRACE_SG_*, the handle has train = 1 and B T <= its batch_size.
 *   resnet_bind_state    caller-owned device buffers, 16-byte aligned: params, grads, exp_avg, exp_avg_sq
 *                        [resnet_param_count] and metrics [IMPALA_NUM_METRICS].  params also becomes the
 *                        buffer of resnet_bind_params (if it is another one, resnet_refresh_weights must
 *                        follow).  Host-side only, whatever `stream`: a learner may call it before every
 *                        step to hand the step a fresh metrics vector.
 *   resnet_set_step      Adam's step count (torch's state['step']), for a resumed run.
 *   resnet_set_debug_vtrace  as impala_set_debug_vtrace: while `out` is not NULL every resnet_loss_head also
 *                        writes adv, err, q [3][B][T-1] and rho [B][T] there (3 B (T-1) + B T floats).
 *   resnet_loss_head     on the heads of the last resnet_forward_train (of n = B T frames): d loss / d
 *                        logits and d loss / d values into the handle's cotangent buffers, and the metric
 *                        sums per trajectory.
 *   resnet_compute_grads resnet_forward_train on batch->obs, resnet_loss_head, resnet_backward into the
 *                        bound grads (written, not added): the gradient before the clip.
 *   resnet_apply_update  the clip and Adam on the bound buffers -- params, exp_avg, exp_avg_sq in place,
 *                        grads left clipped as p.grad is, the metrics vector written, the step count
 *                        advanced -- then resnet_refresh_weights' launches.
 *   resnet_train_step    resnet_compute_grads, then resnet_apply_update: the same launches in the same
 *                        order, the same bits.
 * Every sum has one fixed order: equal inputs give equal bits.  A call on a handle without train = 1 or
 * with a null pointer is IMPALA_E_INVALID, one before resnet_step_init or resnet_bind_state (or, for
 * resnet_loss_head, without a resnet_forward_train of B T frames) IMPALA_E_STATE, before any launch. */
typedef struct resnet_step_config {
  int batch_size;              /* B trajectories a step                                  */
  int rollout_length;          /* T, 2..64                                               */
  float lr, adam_beta1, adam_beta2, adam_eps; /* 1e-4, 0.9, 0.999, 1e-5 (builder.py:43-44) */
  float max_grad_norm;         /* learning.py:93: 0.5                                    */
  float entropy_coeff;         /* learning.py:94: 0.01                                   */
  float vtrace_lambda;         /* 1.0                                                    */
  float clip_rho_threshold;    /* 1.0                                                    */
  float clip_pg_rho_threshold; /* 1.0                                                    */
  int vtrace_grad_mode;        /* IMPALA_VTRACE_SG_*, default IMPALA_VTRACE_SG_ADVANTAGE */
} resnet_step_config;

int resnet_step_config_default(resnet_step_config* cfg);
int resnet_step_init(resnet_actor* h, const resnet_step_config* cfg);
int resnet_bind_state(resnet_actor* h, float* params, float* grads, float* exp_avg,
                      float* exp_avg_sq, float* metrics, void* stream);
int resnet_set_step(resnet_actor* h, int64_t step, void* stream);
int resnet_set_debug_vtrace(resnet_actor* h, float* out);
int resnet_loss_head(resnet_actor* h, const impala_batch* batch, void* stream);
int resnet_compute_grads(resnet_actor* h, const impala_batch* batch, void* stream);
int resnet_apply_update(resnet_actor* h, void* stream);
int resnet_train_step(resnet_actor* h, const impala_batch* batch, void* stream);

/* Test / inspection entry, valid on a handle created with debug = 1 or train = 1: the tensor `which`
 * (RESNET_DBG_*) as the last forward / act left it, its leading `bytes` copied to dst (device or
 * host) on `stream`; bytes in (0, batch_size frames]. */
int resnet_debug_read(resnet_actor* h, int which, void* dst, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESNET_HIP_H_ */
