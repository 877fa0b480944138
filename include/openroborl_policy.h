/* openroborl_policy.h -- C-ABI of the fused policy / value forward pass ("policy inference
 * in the loop on device").
 *
 * Replaces, for all N robots of a shard in ONE launch, what the reference does robot by robot with batch 1:
 *   PPOImitation runner: `policy.step(ob.reshape(-1, *ob.shape))` per robot   (agents/imitation_runners.py:88-92)
 *   ImitationPolicy: actor 160 -> 512 -> 256 -> 12 and critic 160 -> 512 -> 256 -> 1, ReLU (run.py:101-105;
 *   agents/imitation_policies.py:44-51), fixed-std diagonal Gaussian, action = mean + std * N(0, 1)
 *   (agents/imitation_policies.py:96-107), clipped to the action bounds by the runner (imitation_runners.py:140-143).
 *
 * Arithmetic: f32 inputs, f32 accumulation on the matrix cores (v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fmaf
 * chain), i.e. the precision of the reference's float32 TensorFlow graph.  All pointers are device pointers; calls are
 * asynchronous on the caller's stream; return 0 or a negative code with text in orr_last_error() (openroborl_hip.h).
 */
#ifndef OPENROBORL_POLICY_H
#define OPENROBORL_POLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORR_POLICY_OBS_DIM 160
#define ORR_POLICY_H0 512
#define ORR_POLICY_H1 256
#define ORR_POLICY_ACT_DIM 12

/* Number of floats of the packed ("fragment-major") image of a K x N weight matrix: N is padded to a multiple of 16,
 * K must be a multiple of 16. */
int64_t orr_policy_packed_size(int32_t k, int32_t n);

/* Repack a row-major [K][N] float32 weight matrix (the stable-baselines `model/<net>_fc<i>/w:0` layout, fan_in x fan_out)
 * into the layout the forward kernel streams: for output-column tile nt (16 columns), k-group kg (16 rows), lane l, j < 4:
 *   out[((nt * K/16 + kg) * 64 + l) * 4 + j] = W[16 kg + 4 j + (l >> 4)][16 nt + (l & 15)]      (0 beyond column N)
 * so that one 16-byte load per lane yields its B operands of four consecutive MFMA k-steps. */
int32_t orr_policy_pack(const float* w_dev, int32_t k, int32_t n, float* out_dev, void* stream);

/* orr_policy_pack of a layer that has an input normaliser (x - mean) * rstd in front of it, folded into the layer: the forward kernels then
 * run on RAW inputs, unchanged.  ((x - mean) * rstd) W + b = x (diag(rstd) W) + (b - (mean * rstd) W):
 *   out_w     orr_policy_pack's image of diag(rstd) W: every element W[i][j] * rstd[i], one float32 multiplication
 *   out_b[j]  = b[j] - sum_i (mean[i] * rstd[i]) * W[i][j]: the product mean * rstd rounded to float32, then a float32 fused multiply-add per
 *             row, i = 0 .. k - 1 in that order from +0, then one subtraction
 *   w [k][n] row-major, b [n], mean [k], rstd [k] (for a 208-row matrix the caller concatenates the tables: the observation's statistics,
 *   then the privileged row's, or mean 0 and rstd 1 for rows that are not normalised); out_b [n], which may be b itself
 * With mean 0 and rstd 1 the image and the bias equal orr_policy_pack's and b, bit for bit.  One launch, no atomics: the same inputs give the
 * same bits.  Refused, nothing launched or written: what orr_policy_pack refuses, a null b, out_b, mean or rstd, an out_dev, mean or rstd that
 * is not 16-byte aligned, a w, b or out_b that is not 4-byte aligned. */
int32_t orr_policy_pack_norm(const float* w_dev, int32_t k, int32_t n, const float* mean, const float* rstd, const float* b, float* out_dev,
                             float* out_b, void* stream);

typedef struct orr_policy_net {
  /* packed weights (orr_policy_pack) and plain biases of the actor ("pi") and the critic ("vf") */
  const float* w0_pi; const float* b0_pi;   /* 160 x 512 */
  const float* w1_pi; const float* b1_pi;   /* 512 x 256 */
  const float* w2_pi; const float* b2_pi;   /* 256 x 12  (bias: 12 floats) */
  const float* w0_vf; const float* b0_vf;   /* 160 x 512 */
  const float* w1_vf; const float* b1_vf;   /* 512 x 256 */
  const float* w2_vf; const float* b2_vf;   /* 256 x 1   (bias: 1 float) */
} orr_policy_net;

/* One forward pass for n robots.
 *   obs      [n][160]  observation (the env's obs tensor)
 *   noise    [n][12]   standard normal samples, or NULL for the deterministic action (mean)
 *   action   [n][12]   clip(mean + std * noise, -clip, +clip)    -> what env.step() takes
 *   raw      [n][12]   mean + std * noise (unclipped; what the learner's log-probability uses), may be NULL
 *   value    [n]       critic output, may be NULL
 *   mean     [n][12]   actor output, may be NULL */
int32_t orr_policy_forward(const orr_policy_net* net, const float* obs, int32_t n, const float* noise, float std, float clip,
                           float* action, float* raw, float* value, float* mean, void* stream);

/* The same with a privileged critic (the asymmetric actor-critic): the critic's layer 0 reads obs | priv, the actor is untouched.
 *   net->w0_vf  the packed image of a (160 + 48) x 512 matrix (orr_policy_pack with k = 208): rows 0..159 multiply obs[.][0..159],
 *               rows 160..207 multiply priv[.][0..47]; every other member as above
 *   priv        [n][48] the privileged observation (orr_privileged_obs, openroborl_hip.h: ORR_PRIV_DIM has the same value)
 * The actor path runs the same code on the same inputs: action, raw and mean equal orr_policy_forward's bit for bit. */
#define ORR_POLICY_PRIV_DIM 48
int32_t orr_policy_forward_priv(const orr_policy_net* net, const float* obs, const float* priv, int32_t n, const float* noise,
                                float std, float clip, float* action, float* raw, float* value, float* mean, void* stream);

/* The same with a privileged ACTOR as well (a teacher policy, to be distilled into a plain one: openroborl_learner.h, orr_distill_head):
 * both layer 0s read obs | priv.
 *   net->w0_pi, net->w0_vf  packed images of (160 + 48) x 512 matrices (orr_policy_pack with k = 208), rows as above; every other
 *                           member, and every other argument, as in orr_policy_forward_priv
 *   value == NULL           also skips the critic's three layers (about half of the pass; a labelling call needs the mean only).
 *                           action, raw and mean are the same bits with and without a value buffer
 * With rows 160..207 of the actor's matrix zero, action, raw and mean equal orr_policy_forward's; with the same critic, value equals
 * orr_policy_forward_priv's, bit for bit.
 * Refused with a negative code, nothing launched or written: a null net, obs, priv or action, a null member of net, n <= 0, a packed
 * weight matrix that is not 16-byte aligned, any other buffer that is not 4-byte aligned. */
int32_t orr_policy_forward_teacher(const orr_policy_net* net, const float* obs, const float* priv, int32_t n, const float* noise,
                                   float std, float clip, float* action, float* raw, float* value, float* mean, void* stream);

/* The sensor history a history student reads (orr_policy_forward_history): hist [n][16][32] float32, newest first.  A frame is the newest
 * reading of each sensor history inside the 160-word observation followed by four zeros:
 *   obs[0:4] (IMU roll, pitch, roll rate, pitch rate) | obs[12:24] (last action) | obs[48:60] (motor angles) | 0 0 0 0
 * (the histories in obs are slot-major, newest first: sensors_push, csrc/orr_task.h).  16 x 32 = 512 words = 0.53 s at the 30.3 Hz control
 * rate = 32 whole k-groups of the matrix-core operand.
 *   next[i][0] = frame(obs[i]);   next[i][s] = done[i] ? frame(obs[i]) : prev[i][s - 1]     for s = 1..15
 *   obs   [n][160]  the observation the new frame is taken from
 *   done  [n] uint8 the flags of the step that produced obs (after an auto-reset obs is the new episode's first observation: that frame
 *                   fills all 16 slots, as HistoricSensorWrapper.on_reset fills the 3-deep histories); NULL: everybody starts an episode
 *   prev  [n][512]  the history before the step; may be NULL when done is NULL
 *   next  [n][512]  the history after it.  prev == next (in place) is allowed: a thread stores only to words of a column it alone has
 *                   loaded.  Ranges that overlap without being equal are refused
 * Refused with a negative code, nothing launched or written: a null obs or next, a null prev with a done, n <= 0, prev / next not 16-byte
 * aligned, obs not 4-byte aligned, partly overlapping prev and next. */
#define ORR_HISTORY_STEPS 16
#define ORR_HISTORY_FRAME 32
#define ORR_HISTORY_DIM 512
int32_t orr_history_push(const float* obs, const uint8_t* done, const float* prev, float* next, int32_t n, void* stream);

/* A history student (RMA's adaptation module): an encoder estimates the privileged row from the sensor history and the TEACHER's net
 * reads the estimate in the row's place, all in one launch.
 *   z = relu(hist W0 + b0) W1 + b1        [n][48]
 *   action, raw, value, mean = orr_policy_forward_teacher(net, obs, priv = z, ...)        bit for bit
 *   net     a teacher's net: both layer 0s packed at k = 208
 *   enc     the encoder: w0 the packed image of a 512 x 256 matrix, b0 [256], w1 of a 256 x 48 matrix, b1 [48]
 *   hist    [n][512] the history (orr_history_push), 16-byte aligned
 *   latent  [n][48] receives z; may be NULL
 *   value == NULL skips the critic as in orr_policy_forward_teacher; neither it nor latent == NULL changes another output bit
 * Refused like orr_policy_forward_teacher, and: a null enc, a null member of it, a null hist, packed encoder weights or a hist that are
 * not 16-byte aligned, encoder biases or a latent that are not 4-byte aligned. */
typedef struct orr_history_encoder {
  const float* w0; const float* b0;   /* 512 x 256, packed by orr_policy_pack; bias 256 */
  const float* w1; const float* b1;   /* 256 x 48,  packed;                    bias 48  */
} orr_history_encoder;
int32_t orr_policy_forward_history(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs, const float* hist, int32_t n,
                                   const float* noise, float std, float clip, float* action, float* raw, float* value, float* mean,
                                   float* latent, void* stream);

/* A history policy with an ASYMMETRIC critic, for reinforcement learning on the deployable policy itself (RMA's third phase; host side:
 * learner_hip.FusedPPOHistory): the actor reads obs | z as above, the critic reads obs | priv - the true privileged row, which the simulator
 * has at training time and deployment does not need.  One launch.
 *   action, raw, mean, latent = orr_policy_forward_history(net, enc, obs, hist, ...)     bit for bit
 *   value                     = orr_policy_forward_teacher(net, obs, priv, ...)          bit for bit
 *   priv    [n][48] the privileged observation (orr_privileged_obs); may be NULL with value == NULL, which skips the critic as above
 *   every other argument as in orr_policy_forward_history; neither value == NULL nor latent == NULL changes another output bit
 * Refused like orr_policy_forward_history, and: a null priv with a value, a priv that is not 4-byte aligned. */
int32_t orr_policy_forward_history_priv(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs, const float* hist,
                                        const float* priv, int32_t n, const float* noise, float std, float clip, float* action, float* raw,
                                        float* value, float* mean, float* latent, void* stream);

/* Per-robot GAE(lambda) over a [T][N] rollout segment + per-robot advantage standardisation, one launch
 * (reference: add_vtarg_and_adv, agents/ppo_imitation.py:68-93, and the per-robot normalisation :329-338; device
 * layout and the deliberate use of each robot's own done flags: openroborl_amd/rollout.py).
 *   rewards, vpred [T][N] float32; dones [T][N] uint8 (1 = the episode ended at that step);
 *   bootstrap [N] value after the last step (NULL = 0, the reference's choice)
 *   adv [T][N]: advantages, standardised per robot ((a - mean) / (population std + eps)) when normalize != 0
 *   ret [T][N]: TD(lambda) targets = raw advantage + vpred */
int32_t orr_gae(const float* rewards, const float* vpred, const uint8_t* dones, const float* bootstrap, int32_t t, int32_t n,
                float gamma, float lam, int32_t normalize, float eps, float* adv, float* ret, void* stream);

/* The same with flags.  ORR_GAE_LEGACY_INDEX reproduces the reference's recursion for num_robot > 1 bit for bit in its INDEXING:
 * add_vtarg_and_adv reads `episode_starts[(step*num_robot+i) + (1+i)]` (agents/ppo_imitation.py:88), i.e. the episode-start flag of
 * robot (2i+1) mod N at step t + (2i+1)/N instead of robot i's own at t+1 (identical only for N = 1).  For users who compare learning
 * curves with the reference at its default num_robot: 2.  first_starts [N] uint8 = episode_starts of the segment's first step
 * (NULL = all 1: a segment that begins with fresh episodes). */
#define ORR_GAE_NORMALIZE 1
#define ORR_GAE_LEGACY_INDEX 2
int32_t orr_gae_flags(const float* rewards, const float* vpred, const uint8_t* dones, const uint8_t* first_starts, const float* bootstrap,
                      int32_t t, int32_t n, float gamma, float lam, int32_t flags, float eps, float* adv, float* ret, void* stream);

#ifdef __cplusplus
}
#endif
#endif
