/* openroborl_learner.h -- C-ABI of the hand-written pieces of the PPO update ("PPO learner in
 * PyTorch-ROCm"; host side: openroborl_amd/learner_hip.py).
 *
 * The reference builds the update as a TF1 graph (agents/ppo_imitation.py:156-258: clipped surrogate + value loss on the two
 * 160 -> 512 -> 256 -> {12, 1} ReLU networks of agents/imitation_policies.py:44-51) and applies it with MpiAdam
 * (stable_baselines/common/mpi_adam.py:40-62).  Here the dense contractions stay library GEMMs (hipBLASLt through torch); what the
 * autograd graph spends around them - ~70 elementwise / reduction launches per minibatch, more time than the GEMMs themselves - is
 * these launches:
 *   orr_ppo_head       loss terms, d loss / d mean, d loss / d value, bias gradients of the two output layers
 *   orr_ppo_head_logstd  that head for a learned per-dimension log-std read from the device: + its gradient, the entropy bonus, approx-KL, clip fraction
 *   orr_gauss_prepare  the sampler's half of a learned std: noise scaled by exp(log_std) and its log-probability, a whole rollout segment per launch
 *   orr_distill_head   the loss head of policy distillation instead: squared error of the actor's mean against a teacher's, its gradient
 *   orr_regress_head   the loss head of a history student's encoder: squared error of its 48 outputs against the privileged row, its gradient
 *   orr_history_student_head  that head with the action loss: forward through the frozen actor, both losses, backward to the latent, one launch
 *   orr_latent_backward  PPO on a history policy: the gradient from the actor's layer 0 into the encoder's output + the auxiliary estimation loss
 *   orr_head_backward  gradient through an output layer (fan-out 12 or 1) + ReLU mask + bias gradient of the layer below + the
 *                      output layer's weight gradient
 *   orr_colsum_finish  the column sums behind all bias gradients of a minibatch in one launch
 *   orr_relu_backward  ReLU mask in place + bias gradient
 *   orr_adam_step      Adam on the flat parameter vector, step counter on the device (the whole update replays as one hipGraph)
 *   orr_update_control the controls of a step from the flat gradient, on the device: clip coefficient of its norm, non-finite guard, KL gate
 *   orr_adam_step_ctl  orr_adam_step reading those controls and a learning-rate multiplier from device memory (no capture when they change)
 *   orr_running_stats_update  running mean / variance of the network inputs over a whole rollout segment, one pass, merged on the device
 *   orr_normalize_rows (x - mean) * rstd for the learner's batch (the rollout's forward pass has the normaliser folded into layer 0:
 *                      orr_policy_pack_norm, openroborl_policy.h)
 * All pointers are device pointers, float32, row-major and 16-byte aligned; calls are asynchronous on the caller's stream; every
 * reduction runs in a fixed order (no float atomics: the same inputs give the same bits).  Return 0 or a negative code with text in
 * orr_last_error() (openroborl_hip.h).
 */
#ifndef OPENROBORL_LEARNER_H
#define OPENROBORL_LEARNER_H

#include <stdint.h>

#include "openroborl_policy.h"   /* orr_policy_net, for orr_history_student_head */

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of scratch one call below needs for a minibatch of m rows and a layer of c columns.  Calls that finish their sums
 * themselves (gb given) can share one buffer: they run one after the other on the stream.  Deferred calls (gb = NULL) leave their
 * per-workgroup partial sums in the buffer for orr_colsum_finish and need one buffer each. */
int64_t orr_learner_workspace_floats(int32_t m, int32_t c);
/* Rows of partial sums a deferred call leaves for m samples. */
int32_t orr_learner_partial_rows(int32_t m);

#define ORR_PPO_BATCH_COLS 16
/* Loss head for a minibatch of m samples (agents/ppo_imitation.py:196-214: ratio = exp(logp - old logp), surrogate
 * -mean(min(ratio A, clip(ratio, 1 - c, 1 + c) A)), value loss mean((v - tdlamret)^2); fixed-std diagonal Gaussian,
 * agents/imitation_policies.py:96-107).
 *   mean  [m][12], value [m]    outputs of the two networks
 *   batch [m][16]               per sample: raw action (12), old log-probability, advantage, TD(lambda) return, unused
 *   g_mean [m][12], g_value [m] d loss / d mean, d loss / d value for loss = surrogate + vf_coef * value loss (the means over m included)
 *   gb_mean [12], gb_value [1]  column sums of g_mean / g_value = the output layers' bias gradients
 *   stats [2]                   surrogate, value loss (means over the minibatch) */
int32_t orr_ppo_head(const float* mean, const float* value, const float* batch, int32_t m, float std, float clip, float vf_coef,
                     float* g_mean, float* g_value, float* gb_mean, float* gb_value, float* stats, float* workspace, void* stream);

/* orr_ppo_head for a learned, state-independent std: the twelve log-stds (model/pi/logstd:0; the reference declares pi/logstd and freezes it,
 * agents/imitation_policies.py:48) are read from the device at run time, so a captured launch follows them as Adam moves them.
 *   z_k = (a_k - mean_k) exp(-log_std_k),  logp = -1/2 sum_k z_k^2 - sum_k log_std_k - 6 log(2 pi);  ratio, clip and surrogate as orr_ppo_head
 *   loss = surrogate + vf_coef * value loss - ent_coef * H,  H = sum_k log_std_k + 6 log(2 pi e)    (pol_entpen, agents/ppo_imitation.py:196-210)
 *   mean, value, batch, m, g_mean, g_value, gb_mean, gb_value, the alignment: orr_ppo_head's
 *   log_std [12]     device memory, 4-byte aligned (e.g. the parameter's slot in a flat buffer)
 *   g_logstd [12]    d loss / d log_std: the sum over the samples of (d loss / d logp) (z_k^2 - 1), and - ent_coef once
 *   stats [5]        surrogate, value loss, H, approx_kl = mean((ratio - 1) - log ratio), clip_fraction = mean(ratio < 1 - c or ratio > 1 + c)
 *   workspace        orr_learner_workspace_floats(m, 32) floats suffice (32 partial sums per workgroup, added in a fixed order)
 * A refused call launches and writes nothing. */
int32_t orr_ppo_head_logstd(const float* mean, const float* value, const float* batch, const float* log_std, int32_t m, float clip, float vf_coef,
                            float ent_coef, float* g_mean, float* g_value, float* g_logstd, float* gb_mean, float* gb_value, float* stats,
                            float* workspace, void* stream);

/* The sampler's half of a learned std, for n rows in one launch (a whole rollout segment: n = T N):
 *   scaled[i][j] = exp(log_std[j]) * noise[i][j]
 *   logp[i]      = -1/2 sum_j noise[i][j]^2 - sum_j log_std[j] - 6 log(2 pi)      the log-probability of mean + scaled[i] under the sampling policy
 * The forward passes of openroborl_policy.h are then called with noise = scaled and std = 1: mean + 1 * x is mean + x, bit for bit.
 *   noise [n][12], scaled [n][12]   16-byte aligned; scaled may be noise itself (in place) and must not overlap it otherwise
 *   log_std [12]                    device memory, 4-byte aligned, read at run time
 *   logp [n] | NULL                 NULL: only scaled is written
 * A refused call launches and writes nothing. */
int32_t orr_gauss_prepare(const float* noise, const float* log_std, float* scaled, float* logp, int32_t n, void* stream);

/* Loss head of policy distillation for a minibatch of m samples: the student's means against a teacher's (DAgger labels; host side:
 * learner_hip.FusedDistill).  loss = (1 / m) sum_i sum_j (mean[i][j] - target[i][j])^2, j over the 12 actions.
 *   mean [m][12], target [m][12]   the student's and the teacher's actor outputs
 *   g_mean [m][12]                 d loss / d mean = 2 (mean - target) / m
 *   gb_mean [12]                   column sums of g_mean = the student's output-layer bias gradient
 *   stats [1]                      the loss
 * m, the alignment and the workspace are orr_ppo_head's (orr_learner_workspace_floats(m, 16) floats suffice); the sums run in a fixed
 * order.  The rest of the student's backward pass is orr_head_backward, orr_relu_backward, orr_colsum_finish and orr_adam_step. */
int32_t orr_distill_head(const float* mean, const float* target, int32_t m, float* g_mean, float* gb_mean, float* stats, float* workspace,
                         void* stream);

/* Regression loss head for a minibatch of m samples of c columns (host side: learner_hip.FusedDistillHistory, where pred is the history
 * encoder's output and target the recorded privileged rows, c = 48).  loss = (1 / m) sum_i sum_j (pred[i][j] - target[i][j])^2, j < c.
 *   pred [m][c], target [m][c]
 *   g [m][c]       d loss / d pred = 2 (pred - target) / m
 *   gb [c]         column sums of g = the bias gradient of the layer that produced pred
 *   stats [1]      the loss
 * c: a multiple of 4, at most 64.  pred, target, g and workspace 16-byte aligned; workspace: orr_learner_workspace_floats(m, 64) floats.
 * The sums run in a fixed order.  The layers below are torch GEMMs, orr_relu_backward, orr_colsum_finish and orr_adam_step. */
int32_t orr_regress_head(const float* pred, const float* target, int32_t m, int32_t c, float* g, float* gb, float* stats, float* workspace,
                         void* stream);

/* Loss head of a history student's encoder WITH the action loss, for a minibatch of m samples: the encoder's output z goes through the frozen
 * teacher's actor, and the actor's mean is regressed on the teacher's next to the latent regression of orr_regress_head (host side:
 * learner_hip.FusedDistillHistory(action_coef > 0)).  One launch: forward, both losses, backward to the latent; a workgroup owns 16 samples,
 * no activation leaves LDS and no weight gradient is formed (csrc/orr_policy.hip).
 *   in_i   = obs_i | z_i                                      (160 + 48)
 *   mean_i = W2^T relu(W1^T relu(W0^T in_i + b0) + b1) + b2   the actor as orr_policy_forward_teacher computes it, bit for bit (priv = z)
 *   L_act  = (1 / m) sum_i sum_j (mean_ij - target_mean_ij)^2, j < 12;   L_lat = (1 / m) sum_i sum_c (z_ic - target_priv_ic)^2, c < 48
 *   g_z    = d (action_coef L_act + latent_coef L_lat) / d z  [m][48]
 *   net                  only the *_pi members are read (w0_pi packed at k = 208); the vf members may be NULL
 *   w2t, w1t, w0zt       orr_policy_pack of W2^T zero-padded to [16][256], of W1^T [256][512] and of the transpose of W0's rows 160..207, [512][48]
 *   obs [m][160], z [m][48], target_mean [m][12], target_priv [m][48]
 *   g_z [m][48]
 *   mean [m][12] | NULL  the actor's output; NULL: not written, and no other output bit changes
 *   partials             ORR_STUDENT_HEAD_PARTIAL_FLOATS(m) floats, rows = ORR_STUDENT_HEAD_ROWS(m) = one per workgroup:
 *                        [rows][48] the workgroup's column sums of g_z (their sum is the bias gradient of the layer that produced z), followed by
 *                        [rows][2] its shares of L_act and L_lat (the 1 / m included).  orr_colsum_finish folds them in its fixed order, as two
 *                        jobs: {partials, gb [48], rows, 48} and {partials + 48 rows, stats [2], rows, 2}
 * Packed matrices 16-byte aligned, every other buffer 4-byte aligned; m >= 1.  Rows beyond m read as zero and write nothing.  No float atomics:
 * the same inputs give the same bits.  A refused call launches and writes nothing. */
#define ORR_STUDENT_HEAD_ROWS(m) (((m) + 15) / 16)
#define ORR_STUDENT_HEAD_PARTIAL_FLOATS(m) (50 * (int64_t)ORR_STUDENT_HEAD_ROWS(m))
int32_t orr_history_student_head(const orr_policy_net* net, const float* w2t, const float* w1t, const float* w0zt, const float* obs, const float* z,
                                 const float* target_mean, const float* target_priv, int32_t m, float action_coef, float latent_coef, float* g_z,
                                 float* mean, float* partials, void* stream);

/* The PPO gradient of a history policy from the actor's layer 0 into the encoder's output, for a minibatch of m samples (host side:
 * learner_hip.FusedPPOHistory).  The actor's layer 0 reads obs | z; g0 is the gradient at its pre-activation (what orr_relu_backward leaves),
 * and the latent's share of it is an N = 48 GEMM with a reduction and the auxiliary estimation loss fused behind it.  One launch, 16 samples
 * per workgroup, on the f32 matrix cores (csrc/orr_policy.hip):
 *   g_z[i][c] = sum_k g0[i][k] W0_pi[160 + c][k]  +  latent_coef * 2 (z[i][c] - target_priv[i][c]) / m          [m][48]
 *   L_lat     = (1 / m) sum_i sum_c (z_ic - target_priv_ic)^2
 *   g0 [m][512]
 *   w0zt                 orr_policy_pack of the transpose of W0_pi's rows 160..207, [512][48] (orr_history_student_head's w0zt)
 *   z [m][48], target_priv [m][48]    with latent_coef == 0 they may be NULL and are not read; the loss shares are then 0
 *   partials             ORR_LATENT_BACKWARD_PARTIAL_FLOATS(m) floats, rows = ORR_LATENT_BACKWARD_ROWS(m) = one per workgroup:
 *                        [rows][48] the workgroup's column sums of g_z (their sum is the bias gradient of the layer that produced z), followed by
 *                        [rows][1] its share of L_lat (the 1 / m included).  orr_colsum_finish folds them as two jobs:
 *                        {partials, gb [48], rows, 48} and {partials + 48 rows, loss [1], rows, 1}
 * Packed matrix 16-byte aligned, every other buffer 4-byte aligned; m >= 1.  Rows beyond m read as zero and write nothing.  No float atomics
 * and a fixed summation order: the same inputs give the same bits, and with latent_coef == 0 a row of g_z does not depend on m.  A refused
 * call launches and writes nothing. */
#define ORR_LATENT_BACKWARD_ROWS(m) (((m) + 15) / 16)
#define ORR_LATENT_BACKWARD_PARTIAL_FLOATS(m) (49 * (int64_t)ORR_LATENT_BACKWARD_ROWS(m))
int32_t orr_latent_backward(const float* g0, const float* w0zt, const float* z, const float* target_priv, int32_t m, float latent_coef,
                            float* g_z, float* partials, void* stream);

/* g [m][c] (gradient w.r.t. a ReLU layer's output h [m][c]) becomes the gradient w.r.t. its pre-activation, in place: g *= (h > 0);
 * gb [c] = its column sums (the layer's bias gradient).  c: a multiple of 4 with 1024 % c == 0.
 * gb = NULL defers the sum: workspace then holds [orr_learner_partial_rows(m)][c] partial sums for orr_colsum_finish. */
int32_t orr_relu_backward(float* g, const float* h, int32_t m, int32_t c, float* gb, float* workspace, void* stream);

/* The layer below an OUTPUT layer of fan-out k = 12 or 1 (w [c][k] as stored, gy [m][k] = d loss / d output): no GEMM with N = k.
 *   gz [m][c] = (gy . w^T) * (h > 0)    gradient w.r.t. the pre-activation of the hidden layer h [m][c]
 *   gb [c]    = column sums of gz       that layer's bias gradient
 *   gw [c][k] = h^T . gy                the output layer's weight gradient
 * gb = gw = NULL defers both sums: workspace holds [rows][c] partials of gb followed by [rows][c * k] partials of gw. */
int32_t orr_head_backward(const float* gy, int32_t k, const float* w, const float* h, int32_t m, int32_t c, float* gz, float* gb, float* gw,
                          float* workspace, void* stream);

/* out [cols] = sum over `rows` rows of partials [rows][cols], for up to 12 jobs in one launch, in a fixed order (e.g. the six bias
 * gradients, the two output-layer weight gradients and the four split weight gradients of a minibatch). */
#define ORR_COLSUM_MAX_JOBS 12
typedef struct orr_colsum_job {
  const float* partials;
  float* out;
  int32_t rows;
  int32_t cols;
} orr_colsum_job;
int32_t orr_colsum_finish(const orr_colsum_job* jobs, int32_t n_jobs, void* stream);

/* One Adam step on n parameters; t = state[0] + 1, the gradient is multiplied by grad_scale first (1 / world size after an
 * all-reduce sum: mpi_adam.py:51-53).
 *   flags = 0: torch.optim.Adam's arithmetic,  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *   flags = ORR_ADAM_MPI_EPSILON: the reference's MpiAdam (stable_baselines/common/mpi_adam.py:55-62),
 *                                 p -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)      (eps not scaled by sqrt(1 - b2^t))
 * state [2] int32, zero-initialised by the caller once: state[0] counts the steps taken (incremented by the launch itself, so that a
 * captured launch can be replayed), state[1] is internal. */
#define ORR_ADAM_MPI_EPSILON 1
int32_t orr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float grad_scale, int32_t flags, int32_t* state, void* stream);

/* The controls of an optimiser step, in caller-owned DEVICE memory: twelve 32-bit words, 16-byte aligned.  orr_adam_step_ctl reads them at run
 * time, so a captured step follows a learning-rate schedule, a gradient clip, a non-finite guard and a KL gate without being captured again.
 * The caller initialises the record once: lr_mult = kl_lr_mult = grad_scale = 1, every other word 0. */
typedef struct orr_update_ctl {
  /* written by the host */
  float lr_mult;          /* the schedule's multiplier of lr */
  /* written by orr_update_control */
  float kl_lr_mult;       /* the KL-adaptive multiplier of lr, within [kl_lr_lo, kl_lr_hi]; starts at 1 */
  float grad_scale;       /* the clip coefficient of the last call: 1, max_norm / (norm + 1e-6) when that is smaller, 0 for a non-finite norm */
  int32_t skip;           /* != 0: orr_adam_step_ctl changes nothing.  bit 0: the last call saw a non-finite norm or KL (rewritten by every
                           * call); bit 1: KL stop, set by a call and kept until the host clears it */
  /* diagnostics */
  float grad_norm;        /* the last call's norm (may be Inf or NaN) */
  float grad_norm_max;    /* the largest finite norm since the host last cleared the counters */
  float grad_norm_sum;    /* the sum of the finite norms, and */
  int32_t n_calls;        /* how many there were: calls with a finite norm and KL */
  int32_t n_clipped;      /* calls with grad_scale < 1 and a finite norm */
  int32_t n_nonfinite;    /* calls that set bit 0 */
  int32_t n_kl_skipped;   /* calls that left bit 1 set, i.e. steps skipped by the KL stop (the one that tripped it included) */
  int32_t reserved;
} __attribute__((aligned(16))) orr_update_ctl;
int32_t orr_sizeof_update_ctl(void);

/* Floats of `partials` orr_update_control needs for a gradient of n floats (one per workgroup of ORR_UPDATE_CONTROL_BLOCK_FLOATS); -1 for n <= 0. */
#define ORR_UPDATE_CONTROL_BLOCK_FLOATS 1024
int64_t orr_update_control_partials(int64_t n);

/* Produces the controls of the next orr_adam_step_ctl from the flat gradient, in two launches (a streaming pass that leaves one partial sum of
 * squares per workgroup, and one wave that adds them in index order and writes the record).
 *   norm = pre_scale * ||g||_2     g [n] 16-byte aligned, n need not be a multiple of 4 and nothing at or beyond n is read; pre_scale is
 *                                  orr_adam_step's grad_scale (1 / world size).  float32 accumulation in an order fixed by n alone: no float
 *                                  atomics, the same inputs give the same bits; the sum of squares is within (17 + ceil(P / 64)) * 2^-24
 *                                  relative of the exact one, P = orr_update_control_partials(n)
 *   max_norm > 0                   grad_scale = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s formula; n_clipped counts
 *                                  grad_scale < 1.  max_norm <= 0: grad_scale = 1
 *   a non-finite norm              (a NaN or Inf element; or a square or the sum above float32's range, i.e. |g_i| > 1.8e19 or a norm above that:
 *                                  this overflow is reported as non-finite, not computed in a wider format) sets bit 0 of skip, counts in
 *                                  n_nonfinite and gives grad_scale = 0.  A non-finite *kl counts the same.  A finite call clears bit 0
 *   kl | NULL                      device pointer to this minibatch's approx_kl (stats[3] of orr_ppo_head_logstd), 4-byte aligned, read at run time
 *   kl_stop > 0                    *kl > kl_stop sets bit 1 of skip, which stays set until the host clears it.  Every call that leaves it set
 *                                  counts in n_kl_skipped
 *   kl_target > 0                  on a call that leaves skip == 0 (a step that is taken), once:  *kl > 2 kl_target: kl_lr_mult =
 *                                  max(kl_lr_lo, kl_lr_mult / 1.5);  otherwise 0 < *kl < kl_target / 2: kl_lr_mult = min(kl_lr_hi, kl_lr_mult * 1.5)
 * Refused (nothing is launched or written): a NULL g, partials or ctl, g or ctl not 16-byte aligned, n <= 0, kl_lr_lo > kl_lr_hi (or a NaN
 * bound), kl_stop > 0 or kl_target > 0 with kl == NULL. */
int32_t orr_update_control(const float* g, int64_t n, float pre_scale, float max_norm, const float* kl, float kl_stop, float kl_target,
                           float kl_lr_lo, float kl_lr_hi, float* partials, orr_update_ctl* ctl, void* stream);

/* orr_adam_step under a control record written earlier on the same stream: lr * ctl->lr_mult * ctl->kl_lr_mult and
 * grad_scale * ctl->grad_scale take the places of lr and grad_scale.  With ctl->skip != 0 the launch changes nothing - not p, m, v nor state:
 * a skipped step is no Adam step and the bias correction does not advance.  With the record's three factors 1 and skip 0 it gives
 * orr_adam_step's bits (one kernel body; times 1.0f is exact).  ctl 16-byte aligned; everything else as orr_adam_step. */
int32_t orr_adam_step_ctl(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                          float grad_scale, int32_t flags, int32_t* state, const orr_update_ctl* ctl, void* stream);

/* ---- running observation normalisation (host side: ppo.RunningNorm) ------------------------------------------------------------------
 * The statistics record of d columns, in caller-owned DEVICE memory, 16-byte aligned, ORR_RUNNING_STATS_FLOATS(d) 32-bit words:
 *   word 0..1      int64 count (rows seen so far); words 2..3 pad
 *   word 4         float mean[d]
 *   word 4 + d     float var[d]     population variance
 *   word 4 + 2 d   float rstd[d]    1 / (sqrt(var) + eps), formed from the float32 var as stored (a record rebuilt from count, mean, var has the same bits)
 * d is a multiple of 4, so every array starts on 16 bytes.  The host initialises the record once: count 0, mean 0, var 1, rstd 1 - the
 * identity. */
#define ORR_RUNNING_STATS_FLOATS(d) (4 + 3 * (int64_t)(d))
#define ORR_RUNNING_STATS_MEAN(d) 4
#define ORR_RUNNING_STATS_VAR(d) (4 + (d))
#define ORR_RUNNING_STATS_RSTD(d) (4 + 2 * (d))
/* Bytes of the record of d columns; -1 for a d the kernels refuse. */
int64_t orr_sizeof_running_stats(int32_t d);

/* The streaming pass of the update: workgroups of ORR_RUNNING_STATS_THREADS threads, a thread owns four adjacent columns (one 16-byte load per
 * row), a pass covers ORR_RUNNING_STATS_PASS_ROWS(d) whole rows = one contiguous range of x, a workgroup makes ORR_RUNNING_STATS_PASSES of them. */
#define ORR_RUNNING_STATS_THREADS 320
#define ORR_RUNNING_STATS_PASSES 32
#define ORR_RUNNING_STATS_PASS_ROWS(d) (ORR_RUNNING_STATS_THREADS / ((d) / 4))
#define ORR_RUNNING_STATS_BLOCK_ROWS(d) (ORR_RUNNING_STATS_PASSES * ORR_RUNNING_STATS_PASS_ROWS(d))
/* Floats of `partials` for a batch of n rows of d columns: [workgroups][2][d], workgroups = ceil(n / ORR_RUNNING_STATS_BLOCK_ROWS(d)); -1 for
 * arguments the update refuses. */
int64_t orr_running_stats_partials(int64_t n, int32_t d);

/* Merges the moments of a batch x [n][d] into the record, in two launches (like orr_update_control):
 *   1. one pass over x, every element read exactly once by a 16-byte load.  A thread keeps the float32 sums of (x - s) and (x - s)^2 of its
 *      four columns, s = the batch's FIRST row (a shift: the sums never see the column's offset, and sum(x^2) - sum(x)^2 / n is never formed in
 *      float32); a workgroup adds its threads' sums row group by row group and leaves [2][d] floats in partials.  The grid is a function of n
 *      and d alone;
 *   2. one workgroup: the partials are added in float64, consecutive index ranges one after the other, each in index order; then one thread
 *      per column forms the batch's mean = s + S1 / n and M2 = S2 - S1^2 / n (float64) and merges them with the record by the parallel formula
 *      (Chan et al.), n_a, mean_a, M2_a = n_a var_a the record's:
 *          n = n_a + n_b,  delta = mean_b - mean_a,  mean = mean_a + delta n_b / n,  M2 = M2_a + M2_b + delta^2 n_a n_b / n,  var = M2 / n
 *      count 0: the batch replaces the record.  rstd = 1 / (sqrt(var) + eps), rsl_rl's form: at most 1 / eps.  The count is an integer sum.
 * No float atomics and a fixed order of every addition: the same inputs give the same bits.
 * Conditioning: the shift is one sample, not the mean.  With the first row D standard deviations from the column's mean, S2 - S1^2 / n
 * cancels about 1 + D^2 of the partials' float32 digits: the batch's M2 carries a relative error of about (1 + D^2) x a few 2^-24 (D = 4:
 * 1e-5 at most; a first row that is an outlier by 100 sigma: 1e-2).  The mean is not affected beyond the float32 sums' own rounding.
 *   x [n][d] float32, 16-byte aligned; d a multiple of 4, 4 <= d <= 256; n >= 1; eps > 0 and finite
 *   rec        the record, 16-byte aligned
 *   partials   orr_running_stats_partials(n, d) floats, 16-byte aligned
 * A refused call launches and writes nothing. */
int32_t orr_running_stats_update(const float* x, int64_t n, int32_t d, float eps, float* rec, float* partials, void* stream);

/* out[i][c] = (x[i][c] - mean[c]) * rstd[c] in float32: two roundings, no clip (a normaliser folded into a layer cannot clip either, and the
 * learner must see the function the rollout ran).
 *   x, out [n][d] 16-byte aligned; out may be x itself (in place) and must not overlap it otherwise
 *   mean, rstd [d] 16-byte aligned (e.g. the record's arrays); d and n as above
 * A refused call launches and writes nothing. */
int32_t orr_normalize_rows(const float* x, int64_t n, int32_t d, const float* mean, const float* rstd, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
