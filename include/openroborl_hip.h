/*
 * openroborl_hip.h -- C-ABI of the MI355X-native vectorised quadruped imitation environment.
 *
 * Drop-in boundary.  The reference has no FFI: its boundary is the
 * duck-typed Gym env consumed by PPOImitation / traj_segment_generator
 *   (OpenRoboRL/envs/quadruped_robot/wrapper_env.py:58-107  WrapperEnv.step / reset,
 *    OpenRoboRL/envs/quadruped_robot/quadruped_gym_env.py:63-104,213-239  reset / _step).
 * Every entry point below names the reference call(s) it replaces.  The Python host side
 * (openroborl_amd/env.py) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C, no torch types; all device buffers are CALLER-OWNED (torch tensors' data_ptr()),
 *     the library allocates only its small model/clip tables inside orr_create();
 *   - every launch is asynchronous on the hipStream_t passed as void* (NULL = default stream);
 *   - return value 0 = OK, negative = error (text via orr_last_error()); nothing throws;
 *   - quaternions are [x, y, z, w] (reference: envs/utilities/pose3d.py:31,132-136);
 *   - arithmetic type on device: float32.
 */
#ifndef OPENROBORL_HIP_H_
#define OPENROBORL_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORR_ABI_VERSION 5

#define ORR_NUM_MOTORS 12 /* laikago.py:29, mini_cheetah.py:29 */
#define ORR_NUM_LEGS 4
#define ORR_POSE_DIM 19     /* root pos 3 + root quat 4 + 12 joints  (motion_data.py:46-49)   */
#define ORR_VEL_DIM 18      /* root vel 3 + root ang vel 3 + 12 joint rates                   */
#define ORR_PROPRIO_DIM 84  /* IMU 12 | LastAction 36 | MotorAngle 36 (quadruped_gym_env.py:289-320) */
#define ORR_NUM_TAR_FRAMES 4
#define ORR_TARGET_DIM (ORR_NUM_TAR_FRAMES * ORR_POSE_DIM) /* imitation_task.py:254-301 */
#define ORR_OBS_DIM (ORR_PROPRIO_DIM + ORR_TARGET_DIM)     /* 160, wrapper_env.py:109-125 */
#define ORR_MAX_ROBOT_TYPES 32 /* slots of the device model table (a batch may mix that many tables: heterogeneous batches, table sweeps) */
#define ORR_MAX_CLIPS 16
#define ORR_MAX_FALL_PROXIES 16
#define ORR_RING_DEPTH 44   /* latency <= 0.04 s -> int(0.04/0.001)+1 = 41 entries needed      */
#define ORR_RING_ENTRY 20   /* 12 motor angles + 4 rel. quat + 3 rpy rate (+1 pad)             */

/* ---------------------------------------------------------------------------------------
 * Per-robot state record: ORR_STATE_STRIDE 32-bit words, one record per robot, records
 * contiguous ([N, ORR_STATE_STRIDE] tensor).  A 16-lane group (a quarter of a wavefront: four
 * robots per wave) owns one record: lane k moves words k, k+16, ... in 16-byte pieces
 * (coalesced).  X(name, words, kind) with kind F = float32, I = int32.
 * Reference provenance of every group: SURVEY.md Appendix A.1.
 * ------------------------------------------------------------------------------------- */
#define ORR_STATE_FIELDS(X)                                                                   \
  /* rigid state, Bullet conventions: base COM frame, world-frame velocities */               \
  X(POS, 3, F) X(QUAT, 4, F) X(LINVEL, 3, F) X(ANGVEL, 3, F)                                  \
  X(Q, 12, F)  /* URDF joint coordinates, URDF joint order */                                 \
  X(QD, 12, F)                                                                                \
  /* actuator (minitaur.py:160-164,280-293; action_filter.py:99-127), motor order */          \
  X(ACTION, 12, F) X(FILTER_ACTION, 12, F) X(LAST_ACTION, 12, F)                              \
  X(XHIST, 24, F) /* x[n-1] (12), x[n-2] (12) */                                              \
  X(YHIST, 24, F)                                                                             \
  /* 3-deep sensor histories, newest first (sensor_wrappers.py:122-142) */                    \
  X(IMU_HIST, 12, F) X(LASTACT_HIST, 36, F) X(MOTORANG_HIST, 36, F)                           \
  /* task (imitation_task.py:105-139) */                                                      \
  X(TIME_OFFSET, 1, F) X(ORIGIN_POS, 3, F) X(ORIGIN_ROT, 4, F) X(PREV_PHASE, 1, F)            \
  X(REF_POSE, 19, F) X(REF_VEL, 18, F)                                                        \
  /* per-episode randomised parameters (controllable_env_randomizer_from_config.py) */        \
  X(STRENGTH, 12, F) X(LATENCY, 1, F) X(FOOT_MU, 1, F) X(KNEE_FRICTION, 4, F)                 \
  X(MASS_RATIO, 2, F) X(INERTIA_RATIO, 2, F) X(BASE_DAMPING, 2, F)                            \
  /* contact warm start: per leg (normal, t1, t2) impulses */                                 \
  X(LAMBDA, 12, F)                                                                            \
  X(EP_RETURN, 1, F) X(LAST_EP_RETURN, 1, F) X(GRID_OFFSET, 2, F)                             \
  /* integers */                                                                              \
  X(STATE_ACTION_COUNTER, 1, I) /* minitaur.py:186-189 */                                     \
  X(STEP_COUNTER, 1, I)                                                                       \
  X(FILTER_VALID, 1, I)  /* _filter_action is not None (minitaur.py:450-453) */               \
  X(RING_LEN, 1, I) X(RING_HEAD, 1, I)                                                        \
  X(EPISODE_IDX, 1, I)   /* RNG stream selector */                                            \
  X(EP_STEP, 1, I)       /* env_step_counter, per robot (quadruped_gym_env.py:88,237) */      \
  X(WARMUP, 1, I)        /* _curr_episode_warmup */                                           \
  X(MAX_EP_STEPS, 1, I)  /* wrapper_env.py:151-159 */                                         \
  X(ROBOT_TYPE, 1, I) X(CLIP_ID, 1, I)                                                        \
  X(ROBOT_INDEX, 1, I)   /* global robot index (RNG key, grid slot) */                        \
  X(LAST_EP_LEN, 1, I)                                                                        \
  X(DONE_REASON, 1, I)   /* of the last step; survives the (auto-)reset that follows it */    \
  X(RESERVED_I, 2, I)                                                                         \
  /* latency ring (minitaur.py:127,313-357): ORR_RING_DEPTH entries of ORR_RING_ENTRY */      \
  X(RING, ORR_RING_DEPTH * ORR_RING_ENTRY, F)                                                 \
  /* ABI v5, behind the ring (never staged with the head): Bullet's friction anchors, one cached contact point per toe             \
   * (btPersistentManifold::replaceContactPoint): the point on the toe in the lower-leg link frame (3) and on the plane in world (3) */ \
  X(ANCHOR, 4 * 6, F)                                                                         \
  X(ANCHOR_VALID, 4, I)  /* per leg: 1 = that toe holds a cached point */                    \
  /* behind the anchors (never staged with the head): motion time at which the next clip is drawn (orr_set_clip_switch); written by   \
   * the multi-clip variants only, +inf = never (state.default_state's initial value) */                                        \
  X(CLIP_CHANGE_TIME, 1, F)

enum orr_state_offset_e {
#define ORR_X_OFF(name, words, kind) ORR_OFF_##name, ORR_OFFEND_##name = ORR_OFF_##name + (words)-1,
  ORR_STATE_FIELDS(ORR_X_OFF)
#undef ORR_X_OFF
      ORR_STATE_WORDS
};
#define ORR_STATE_STRIDE 1216 /* ORR_STATE_WORDS rounded up to a multiple of 64 (19 x 64) */
typedef char orr_state_words_fit_the_stride[(ORR_STATE_WORDS <= ORR_STATE_STRIDE) ? 1 : -1]; /* C99 static assertion */

/* done reasons (bit mask) */
#define ORR_DONE_CONTACT_FALL 1 /* imitation_task.py:536-546 */
#define ORR_DONE_ROOT_POS 2     /* imitation_task.py:553-556 */
#define ORR_DONE_ROOT_ROT 4     /* imitation_task.py:558-565 */
#define ORR_DONE_TIME_LIMIT 8   /* wrapper_env.py:79 */
#define ORR_DONE_NAN 16         /* new: non-finite state guard */
#define ORR_DONE_MOTION_OVER 32 /* imitation_task.py:532,567 + motion_data.py:265-276: a non-looping clip played to its end */

/* orr_config.flags */
#define ORR_FLAG_AUTO_RESET 1        /* per-robot masked auto-reset inside orr_step (native mode) */
#define ORR_FLAG_RANDOMIZER 2        /* run.py:205-206: enabled when mode == "train" */
#define ORR_FLAG_CYCLE_SYNC 4        /* run.py:61 enable_cycle_sync=True */
#define ORR_FLAG_LEGACY_GRID 8       /* minitaur.py:246-248: 2 m grid slots (float32 loses precision at N>>100) */
#define ORR_FLAG_CURRICULUM 16       /* wrapper_env.py:147-159 */

/* clip flags (motion_data.py:83-97) */
#define ORR_CLIP_WRAP 1
#define ORR_CLIP_CYCLE_POS 2
#define ORR_CLIP_CYCLE_ROT 4

typedef struct orr_config {
  int32_t abi_version;     /* ORR_ABI_VERSION */
  int32_t num_robots;      /* robots on THIS device (shard size) */
  int32_t action_repeat;   /* 33: laikago.py:26 */
  int32_t solver_iters;    /* int(300/33) = 9: quadruped_gym_env.py:177-178 */
  float sim_dt;            /* 0.001: pybullet_sim_param.yaml:3 */
  float gravity_z;         /* -10: quadruped_gym_env.py:200 */
  float reward_w[5];       /* pose, velocity, end-effector, root pose, root velocity: imitation_task.py:45-49 */
  float reward_scale[6];   /* pose, vel, end-eff, end-eff height, root pose, root vel: imitation_task.py:50-55 */
  int32_t tar_frame_steps[ORR_NUM_TAR_FRAMES]; /* run.py:62 [1,2,10,30] */
  float ref_state_init_prob; /* run.py:63 0.9 */
  float warmup_time;         /* run.py:64 0.25 */
  int32_t ep_len_start;      /* run.py:54 20 */
  int32_t ep_len_end;        /* run.py:55 600 */
  int64_t curriculum_steps;  /* ceil(3e7 / num_procs): wrapper_env.py:45-46 */
  uint64_t seed;
  int32_t flags;
  /* physics-engine constants (parity-unpinned).  First value: what the Python host passes since round 6 = what PyBullet's
     createEmptyDynamicsWorld is remembered to set; in brackets the Bullet library's default (rounds 1-5).  DESIGN.md section 4. */
  float contact_erp;         /* 0.08 [0.2] */
  float contact_margin;      /* 0.004 [0.02] contact breaking threshold: a normal row exists / a termination proxy counts inside it */
  float warmstart_factor;    /* 0.1 [0.85] */
  float max_coord_velocity;  /* 100; orr_create refuses sqrt(3) * max_coord_velocity * sim_dt / 2 >= 0.2 (the base may turn at most 0.4 rad per sub-step) */
  float plane_friction;      /* 1.0 plane_implicit.urdf */
  float limit_activation;    /* 0.1 rad: a joint-limit row exists iff the joint is this close */
  float max_angle_change;    /* 0.2: laikago.py:71 MAX_MOTOR_ANGLE_CHANGE_PER_STEP */
  float dist_fail_threshold; /* 1.0: imitation_task.py:518 */
  float rot_fail_threshold;  /* pi/2 */
  float friction_erp;        /* ABI v5: 0.2 = Bullet's m_frictionERP: share of a friction anchor's tangential drift removed per sub-step
                                (friction rows get -drift * friction_erp / dt; only toes with orr_model::friction_anchor) */
} orr_config;

/* Robot model table (data, swappable without touching kernels).  All geometry is given in the
 * "kinematic" body frame (x forward, y left, z up) at zero motor angles, where every link frame
 * is parallel to the base frame.  Base orientation used by the dynamics is
 * QUAT (x) INIT_QUAT^-1 (the reference's "relative orientation", minitaur.py:325-331), so the
 * stored QUAT stays in the URDF convention of the motion clips.
 * Bodies: 0 = base; 1 + 3*leg + k, k = 0 hip(abduction) link, 1 upper leg, 2 lower leg (+ fixed toe
 * merged for the dynamics).  Joint j = 3*leg + k (URDF joint order) connects body j+1 to its parent. */
typedef struct orr_model {
  float init_pos[3];                    /* laikago.py:48 / mini_cheetah.py:49 */
  float init_quat[4];                   /* laikago.py:49 / mini_cheetah.py:50 */
  float init_motor_angles[ORR_NUM_MOTORS]; /* motor order; laikago.py:62 */
  float motor_dir[ORR_NUM_MOTORS];      /* JOINT_DIRECTIONS, motor order; +1 or -1 (orr_set_model refuses anything else) */
  float motor_offset[ORR_NUM_MOTORS];   /* JOINT_OFFSETS, motor order */
  int32_t joint_of_motor[ORR_NUM_MOTORS]; /* URDF joint index driven by motor m (MOTOR_NAMES order) */
  float kp[ORR_NUM_MOTORS];             /* motor order; laikago.py:65 */
  float kd[ORR_NUM_MOTORS];
  float base_mass;
  float base_inertia[6];                /* xx yy zz xy xz yz about the base COM */
  float link_mass[12];
  float link_com[12][3];                /* in link frame (origin = joint origin) */
  float link_inertia[12][6];            /* about link COM; scales with the inertia ratio */
  float link_inertia_pa[12][6];         /* parallel-axis part of a merged (lower leg + toe) link; scales with the mass ratio */
  int32_t link_group[12];               /* 0 = "base" randomisation group (hip links), 1 = "leg" group (minitaur.py:812-851) */
  float joint_pos[12][3];               /* joint origin in the parent link frame */
  float joint_axis[12][3];              /* unit axis; kinematic angle = dir * (q_urdf - offset) */
  float joint_lo[12];                   /* limits in kinematic (motor-convention) angle */
  float joint_hi[12];
  float toe_pos[4][3];                  /* toe sphere centre in the lower-leg link frame (= toe link COM) */
  float lower_com[4][3];                /* lower leg's own COM (end-effector reward, imitation_task.py:441-446) */
  float toe_radius;
  float shank_pos[4][3];                /* second contact sphere of the lower leg ("shank"; lower legs are feet: minitaur.py:842-844), */
  float shank_radius;                   /* in the lower-leg link frame; radius 0 = none.  A leg touches the ground with whichever of its
                                           two spheres (toe, shank) is lower: one contact point per leg and sub-step */
  float foot_friction;                  /* default lateral friction of toe / lower leg */
  float contact_stiffness;              /* URDF <contact><stiffness/><damping/> of the TOE link (Bullet's BT_CONTACT_FLAG_CONTACT_STIFFNESS_DAMPING): */
  float contact_damping;                /* the toe's normal row gets cfm = 1 / (dt k + d), erp = dt k / (dt k + d) instead of the global
                                           contact_erp and cfm 0 (btMultiBodyConstraintSolver::setupMultiBodyContactConstraint).
                                           stiffness <= 0 = rigid contact (the global pair); ABI v4.  These are the values of the PAIR: Bullet combines
                                           the two bodies' entries (btManifoldResult: k = 1 / (1 / k_toe + 1 / k_plane), d = d_toe + d_plane; the
                                           plane's defaults - a huge stiffness and a damping of 0.1 - change (30000, 1000) by 0.01 %), the caller folds
                                           them in if it has them.  The configuration's sim_dt and contact_erp must be final before the model is set: the
                                           row's cfm / erp are folded when the model is set */
  int32_t friction_anchor;              /* URDF <contact><friction_anchor/> of the TOE link (ABI v5): the toe's contact point is CACHED while its
                                           friction impulse stays inside the cone (btPersistentManifold::replaceContactPoint), and the friction
                                           rows pull the cached pair of points together (orr_config::friction_erp).  0 = off */
  int32_t num_fall_proxies;             /* termination-only collision spheres on non-foot links */
  int32_t fall_body[ORR_MAX_FALL_PROXIES];
  float fall_pos[ORR_MAX_FALL_PROXIES][3];
  float fall_radius[ORR_MAX_FALL_PROXIES];
} orr_model;

/* device-side global counters, caller-owned int64[ORR_NUM_COUNTERS], zero-initialised */
enum orr_counter_e {
  ORR_CNT_TOTAL_STEP_COUNT = 0, /* wrapper_env.py:47,82-83 curriculum counter */
  ORR_CNT_DONE_ACCUM = 1,       /* per-launch scratch (unused; zero) */
  ORR_CNT_TICKET = 2,           /* per-launch scratch: the launch tally, done count << 32 | robots counted; zero between launches */
  ORR_CNT_TOTAL_TIMESTEPS = 3,  /* robot-steps executed (ppo_imitation.py:421) */
  ORR_CNT_EPISODES = 4,         /* finished episodes appended to the episode log */
  ORR_CNT_EPLOG_DROPPED = 5,
  ORR_NUM_COUNTERS = 8
};

typedef struct orr_handle orr_handle;

const char* orr_last_error(void);
int32_t orr_abi_version(void);
const char* orr_source_hash(void);              /* hash of the sources this library was built from (host loader: stale-build check) */
int32_t orr_state_stride(void);                 /* ORR_STATE_STRIDE */
int32_t orr_layout_count(void);                 /* number of fields in ORR_STATE_FIELDS */
const char* orr_layout_name(int32_t i);
int32_t orr_layout_offset(int32_t i);
int32_t orr_layout_size(int32_t i);
int32_t orr_layout_is_int(int32_t i);
int32_t orr_sizeof_config(void);
int32_t orr_sizeof_model(void);

/* replaces LocomotionGymEnv._init world setup (quadruped_gym_env.py:158-211) */
int32_t orr_create(const orr_config* cfg, orr_handle** out);
int32_t orr_destroy(orr_handle* h);

/* replaces LocomotionGymEnv.seed (quadruped_gym_env.py:59-61): new key of the counter-based RNG, used from the next reset on */
int32_t orr_set_seed(orr_handle* h, uint64_t seed);

/* replaces loadURDF + _build_urdf_ids + _record_*_from_urdf (minitaur.py:201-230,812-851,897-903) */
int32_t orr_set_model(orr_handle* h, int32_t robot_type, const orr_model* model_host);

/* replaces MotionData.load results (motion_data.py:72-112): frames [F,19] and frame velocities
 * [F,18] are DEVICE pointers to post-processed data; cycle_delta = {dx, dy, dz(=0), dheading}.
 * frame_dt = the clip's "FrameDuration" as a DOUBLE (ABI v3): the sampler keeps the motion time in float64 like the reference
 * (shipped clips use 1/24 s and 0.03 s; 20 s into an episode a float32 frame time misplaces the blend factor by 1e-5, which
 * the O(100) jumps of the finite-difference frame velocities turn into 1e-3). */
int32_t orr_set_motion(orr_handle* h, int32_t clip_id, const float* frames_dev, const float* frame_vels_dev,
                       int32_t num_frames, double frame_dt, int32_t clip_flags, const float cycle_delta[4]);

/* bind caller-owned device buffers: state [N, ORR_STATE_STRIDE] words (16-byte aligned), counters int64[8],
 * episode log float[ep_log_capacity][2] = (return, length) (may be NULL / 0). */
int32_t orr_bind(orr_handle* h, void* state_dev, int64_t* counters_dev, float* ep_log_dev, int32_t ep_log_capacity);

/* clip set of a robot type (ImitationTask with several ref_motion_filenames: _sample_ref_motion, imitation_task.py:694-701,1077-1085):
 * n = 1 .. ORR_MAX_CLIPS ids, each loaded with orr_set_motion (repeats allowed).  At every reset of a robot of that type (orr_reset and
 * the auto-reset inside orr_step) its CLIP_ID becomes clip_ids[(m * n) >> 24], m = the 24-bit integer of draw 28 of the episode's
 * (seed, robot index, episode) stream (Philox block 7, word 0; draws 0..27 keep their meaning), before anything reads the clip.
 * That is the uniform draw, which this call (re)installs for the type; orr_set_clip_weights and orr_clip_curriculum_update below
 * replace it by a weighted one on the same m.
 * While some type's set has more than one clip, orr_step and orr_reset launch the multi-clip variants of the kernels (one wave per SIMD
 * at any batch size; refused together with friction anchors).  A type without a set keeps the record's CLIP_ID.  A rejected call
 * changes nothing. */
int32_t orr_set_clip_set(orr_handle* h, int32_t robot_type, const int32_t* clip_ids_host, int32_t n);

/* clip log int32[ep_log_capacity] (device; NULL unbinds): while the multi-clip variants run, episode-log row `slot` also gets the
 * clip the ending episode played in clip_log[slot].  The capacity is orr_bind's. */
int32_t orr_bind_clip_log(orr_handle* h, int32_t* clip_log_dev);

/* mid-episode clip switching of a robot type (ImitationTask's clip_time_min / clip_time_max: _reset_clip_change_time, _check_change_clip,
 * _update_ref_motion, imitation_task.py:734-761,1057-1069,1096-1101).  tmin = tmax = +inf (the default) = never; otherwise
 * 0 <= tmin <= tmax < inf.  Turning switching off on a running handle stops it from the next step on (a record keeps its finite
 * CLIP_CHANGE_TIME until its next reset writes +inf, but no step switches it).  Refused: NaN, a negative value, tmin > tmax, exactly one infinite bound, friction anchors on the handle;
 * a rejected call changes nothing.  A type whose clip set has one clip (or none) never switches.  Draw rule, on the episode's
 * (seed, robot index, episode) stream u_d (d = 4 * Philox block + word):
 *   reset: CLIP_CHANGE_TIME = t0 + tmin + u_29 (tmax - tmin), t0 = the motion time after the reset (warm-up shift included);
 *   step whose env-step counter before the step is s, when the motion time t (old offset) >= CLIP_CHANGE_TIME and the set has n > 1
 *   clips: with d = 32 + 4 s (Philox block 8 + s), CLIP_ID = set[(m_d n) >> 24] (as at a reset), CLIP_CHANGE_TIME = t + tmin +
 *   u_(d+1) (tmax - tmin), TIME_OFFSET = u_(d+2) * the new clip's duration, PREV_PHASE = the new clip's phase at t, and the
 *   reference origin is synchronised in heading (relative to the robot's init orientation) and horizontal position at the new time.
 * Pose, velocity, target frames and termination of that step use the new clip at the new time.  The multi-clip kernel variants do
 * this (orr_set_clip_set); the parity replays (orr_debug_replay_step / _reset) run them while some type has a switch range. */
int32_t orr_set_clip_switch(orr_handle* h, int32_t robot_type, float tmin, float tmax);

/* weighted clip draws.  The draw of a clip (at a reset and at a mid-episode switch) goes by a table of 24-bit-scale thresholds per robot
 * type in DEVICE memory, cum[0 .. n]: cum[0] = 0, cum[n] = 2^24, non-decreasing, and entry k of the set is drawn iff cum[k] <= m <
 * cum[k + 1], m = the 24-bit integer of the same draw as before (draw 28 at a reset, 32 + 4 s at a switch; no draw moves).  The kernels
 * read the table in memory, so new thresholds hold from the next launch on, in a replayed hipGraph as well, and select no kernel variant.
 * orr_set_clip_set writes the UNIFORM thresholds cum[k] = (k * 2^24 + n - 1) / n (integer ceil), which pick exactly (m * n) >> 24.
 * orr_set_clip_weights: n float32 weights in entry order (n = the set's size); cum[k] = ceil(2^24 * W_k / W) in double, W_k = the
 * running sum of the weights, W their total.  A zero weight = the entry is never drawn; equal weights give the uniform thresholds
 * exactly.  NULL restores the uniform thresholds.  Refused, changing nothing: a bad type, a type without a set, n != the set's size, a
 * negative, NaN or infinite weight, all weights zero. */
int32_t orr_set_clip_weights(orr_handle* h, int32_t robot_type, const float* weights_host, int32_t n);
/* the thresholds of a type as the DEVICE holds them (the curriculum's kernel below writes them there) and the set's size; synchronises */
int32_t orr_get_clip_thresholds(orr_handle* h, int32_t robot_type, uint32_t out_host[ORR_MAX_CLIPS + 1], int32_t* n);

/* failure-adaptive clip sampling: one kernel turns the episode log into per-clip scores, a running score per clip id and new thresholds,
 * without a host round trip.  The episode score of a logged episode of clip c is q = floor(65536 * clamp(x / ref[c], 0, 1) + 0.5), x
 * the float32 metric of its log row (LENGTH: its length, RETURN: its return, STEP_REWARD: return / max(length, 1) in float32), the
 * quotient in double. */
#define ORR_CLIP_METRIC_LENGTH 0
#define ORR_CLIP_METRIC_RETURN 1
#define ORR_CLIP_METRIC_STEP_REWARD 2
typedef struct orr_clip_curriculum {
  float alpha;                 /* weight of an update's mean score in the running score, in (0, 1] */
  float eps;                   /* share of the uniform distribution in the new probabilities, in [0, 1] */
  int32_t metric;              /* ORR_CLIP_METRIC_* */
  float ref[ORR_MAX_CLIPS];    /* per clip id: the metric's value that counts as mastered (score 1) */
} orr_clip_curriculum;
int32_t orr_sizeof_clip_curriculum(void);
/* uploads the settings and zeroes the running scores.  Refused, changing nothing: alpha outside (0, 1], eps outside [0, 1], an unknown
 * metric, a ref that is not finite and > 0 for a clip id that occurs in some type's set. */
int32_t orr_set_clip_curriculum(orr_handle* h, const orr_clip_curriculum* cur_host);
/* ONE launch on `stream`, asynchronous and capturable into a hipGraph.  Needs a bound episode log (orr_bind), a bound clip log
 * (orr_bind_clip_log) and settings (orr_set_clip_curriculum): otherwise a negative code, and nothing is launched.  Reads the rows [0,
 * min(counters[ORR_CNT_EPISODES], ep_log_capacity)) of both logs and clears NOTHING: call it once between two clears of the log
 * (orr_episode_stats, or the owner of the counters, clears it).  Per clip id c (rows whose clip id lies outside [0, ORR_MAX_CLIPS) are
 * ignored): n_c = its rows, S_c = the sum of their q as INTEGERS (the rows land in the log in no fixed order; integer sums make the
 * result independent of it); if n_c > 0, ema_c = (1 - alpha) ema_c + alpha S_c / (65536 n_c) in double, else ema_c stays.  Then for
 * every type whose set has n > 1 entries, entry k with clip id c_k: f_k = 1 - ema_{c_k}, F = their sum in entry order; F < 1e-12 gives the
 * uniform thresholds, else p_k = (1 - eps) f_k / F + eps / n and the thresholds follow from p by orr_set_clip_weights' rule, in double.
 * stats_dev: double [ORR_MAX_CLIPS][4] on the device = (n_c, S_c, S_c / (65536 n_c) or 0, ema_c after the update) per clip id, or NULL. */
int32_t orr_clip_curriculum_update(orr_handle* h, double* stats_dev, void* stream);

/* task noise of the handle (ImitationTask's perturb_init_state_prob with _apply_state_perturb, and tar_obs_noise[0]: imitation_task.py:
 * 192-197, 273-275, 778-793, 1195-1243).  A task option, not a robot-type one: one setting per handle, read from the next launch on. */
typedef struct orr_task_noise {
  float perturb_init_state_prob;   /* 0 = off */
  float root_pos_std, root_rot_std, joint_pose_std, root_vel_std, root_ang_vel_std, joint_vel_std;  /* the reference's six:
                                      0.025, 0.025 pi, 0.05 pi, 0.1, 0.05 pi, 0.05 pi (imitation_task.py:1201-1206) */
  float tar_heading_std;           /* tar_obs_noise[0]; 0 = off */
} orr_task_noise;
/* noise_host NULL = all off.  Refused: NaN, a probability outside [0, 1], a negative or infinite standard deviation (the message names
 * the field), friction anchors on the handle; a rejected call changes nothing.  While perturb_init_state_prob and tar_heading_std are
 * both 0 the handle runs exactly the kernels it runs without this call; otherwise orr_step, orr_reset and the parity replays launch the
 * noise variants (the clip-set variants + noise: one wave per SIMD at any batch size, refused together with friction anchors; a type
 * without a clip set keeps its CLIP_ID).  Draw rule, on the episode's (seed, robot index, episode) stream u_d (d = 4 * Philox block +
 * word; draws 0..29 and the clip-switch blocks 8 + s keep their meaning; in the parity replays these blocks always come from Philox):
 *   normal pair of two uniforms (ua, ub):  r = sqrt(-2 ln(1 - ua)),  z0 = r cos(2 pi ub),  z1 = r sin(2 pi ub);
 *   reset: U(k) = word k of blocks 0x20000000 .. 0x20000008 (k = 0..35).  The robot is perturbed iff U(0) < perturb_init_state_prob.
 *     Axis a_i = -1 + 2 U(i), i = 1..3, normalised (squared norm below 1e-30: no rotation).  Pair j = 0..15 of (U(4 + 2j), U(5 + 2j))
 *     gives z_2j, z_2j+1, assigned in the reference's call order: z0 z1 root position x y, z2 rotation angle, z3..z14 joint angles,
 *     z15 z16 root velocity x y, z17..z19 root angular velocity, z20..z31 joint rates.  What the reset writes into POS / QUAT / LINVEL /
 *     ANGVEL / Q / QD is the reference state + std * z, the orientation quaternion_about_axis(root_rot_std z2, a) (x) reference rotation
 *     (not renormalised); REF_POSE, REF_VEL, the origin and PREV_PHASE stay the unperturbed ones;
 *   target observation: block 0x30000000 + i, i = 0 for the observation of a reset of that episode (the auto-reset inside a step
 *     included), i = 1 + s for the step whose env-step counter before the step is s: heading += tar_heading_std * z0 of the pair
 *     (word 0, word 1) before the target frames are expressed in it.  Nothing but the observation depends on it. */
int32_t orr_set_task_noise(orr_handle* h, const orr_task_noise* noise_host);
int32_t orr_sizeof_task_noise(void);

/* sensor noise of the handle (Minitaur._observation_noise_stdev, minitaur.py:67,126,370-375: zero-mean Gaussian noise on every reading
 * of the "noisy" getters get_motor_angles, get_base_rpy and get_base_rpy_rate).  One setting per handle, read from the next launch on. */
typedef struct orr_sensor_noise {   /* Minitaur._observation_noise_stdev, in its order */
  float motor_angle_std, motor_velocity_std, motor_torque_std, base_rpy_std, base_rpy_rate_std;
} orr_sensor_noise;
/* noise_host NULL = all off.  Refused: a NaN, a negative or an infinite value (the message names the field), friction anchors on the
 * handle (a launch refuses the combination too, and launches nothing, when such a model is set afterwards); a rejected call changes
 * nothing.  motor_velocity_std and motor_torque_std are stored for schema fidelity and have NO consumer on this path: in the reference
 * only get_energy_consumption_per_step reads the getters they belong to.  While motor_angle_std, base_rpy_std and base_rpy_rate_std are
 * all 0 the handle launches exactly the kernels it launches without this call; otherwise orr_step, orr_reset and the parity replays
 * launch the sensor variants (supersets of the actuator, contact, reward-terms and task-noise variants: one wave per SIMD at any batch
 * size).  With sa, sr, sd = the angle, rpy and rate deviations, co = the control (latency-delayed) observation and map_pi =
 * MapToMinusPiToPi, every reading has a normal z of its own:
 *   sub-step k of a step, motor m: cur = map_pi(co[m] + sa z) is what the +-max_angle_change clip of the motor command is centred on
 *     (_clip_motor_commands, :706-723); while the episode has no filtered action yet (its first step) the interpolation starts from
 *     map_pi(co[m] + sa z') with a separate draw, redrawn every sub-step (process_action, :449-456).  The PD law's own angle and rate
 *     stay the true ones;
 *   the Butterworth history of an episode's first step is initialised with map_pi(co[m] + sa z) (_filter, :1169-1178);
 *   the sensor histories (robot_sensors.py:74-83,153-190): the motor-angle columns get map_pi(co[m] + sa z), roll and pitch rpy + sr z,
 *     the two rates rate + sd z.  At a reset the three history entries are three separate readings (sensor_wrappers.py:122-129), the
 *     first of which ends up as the oldest entry;
 *   the target observation: pitch and yaw of the delayed rpy each get sr z before the heading is formed (get_base_orientation,
 *     :630-638); orr_task_noise::tar_heading_std's term, if on, is added after.
 * Draw rule, on the episode's (seed, robot index, episode) stream; every older block keeps its meaning, and in the parity replays
 * these blocks always come from Philox, like the task-noise blocks:
 *   block = 0x10000000 + (i << 9) + (slot << 4) + lane   (below 0x20000000 for i < 2^19)
 *   i = 0 for a reset of that episode (the auto-reset inside a step included), 1 + s for the step whose env-step counter before it is s;
 *   normal pairs as in orr_set_task_noise: (z0, z1) of the uniforms (word 0, word 1) and of (word 2, word 3);
 *   slot 0..16 (steps), lane = motor m: sub-step 2 slot uses the pair (0, 1), sub-step 2 slot + 1 the pair (2, 3); z0 = the clip's
 *     reading, z1 = the interpolation start's;
 *   slot 17, lane = history column (0..11 motor angle, 12 roll, 13 pitch, 14 roll rate, 15 pitch rate): a step takes z0 of the pair
 *     (0, 1); a reset z0, z1 of the pair (0, 1), then z0 of the pair (2, 3), in reading order;
 *   slot 18, lane = motor m: z0 of the pair (0, 1), the filter history's initial value;
 *   slot 19, lane 0: the pair (0, 1) -> roll (unused), pitch; z0 of the pair (2, 3) -> yaw: the target observation's rpy. */
int32_t orr_set_sensor_noise(orr_handle* h, const orr_sensor_noise* noise_host);
int32_t orr_sizeof_sensor_noise(void);

/* domain randomisation of the handle (ControllableEnvRandomizerFromConfig, controllable_env_randomizer_from_config.py:92-172; the
 * parameter dictionary of minitaur_env_randomizer_config.py: name -> [lower, upper]).  Ten of the reference's sixteen names, in its
 * application order (sorted by name); "battery" and "motor friction" are no-ops in the reference, "control step", "individual mass",
 * "individual inertia" and "restitution" have nothing to act on in this engine. */
enum { ORR_RAND_BASE_MASS, ORR_RAND_GLOBAL_MOTOR_STRENGTH, ORR_RAND_INERTIA, ORR_RAND_JOINT_FRICTION, ORR_RAND_LATENCY,
       ORR_RAND_LATERAL_FRICTION, ORR_RAND_LEG_WEAKEN, ORR_RAND_MASS, ORR_RAND_MOTOR_STRENGTH, ORR_RAND_SINGLE_LEG_WEAKEN,
       ORR_RAND_NUM_PARAMS };                       /* the reference's application order: sorted by name */
typedef struct orr_randomizer { int32_t enabled[ORR_RAND_NUM_PARAMS]; float lo[ORR_RAND_NUM_PARAMS], hi[ORR_RAND_NUM_PARAMS]; } orr_randomizer;
/* Everything below holds while ORR_FLAG_RANDOMIZER is set; without the flag no reset randomises anything and no row is written.
 * host NULL = the built-in six ranges (inertia 0.5-1.5, joint friction 0-0.05, latency 0-0.04, lateral friction 0.5-1.25, mass 0.8-1.2,
 *   motor strength 0.8-1.2; the other four disabled) and the kernels the handle launched before.  A non-NULL host - whatever its
 *   ranges - or a bound params buffer selects the randomiser variants of orr_step, orr_reset and the parity replays (supersets of the
 *   sensor variants: one wave per SIMD at any batch size, unbound outputs skipped, zero noise passes the reading).
 * Value of an enabled parameter: fmaf(u, hi - lo, lo) in float32, u in [0, 1) its draw, hi - lo one float32 subtraction on the device.
 *   A disabled parameter leaves its record words as they are.  Parameters apply in enum order, a later one overwrites an earlier one's
 *   words: base mass -> MASS_RATIO[0]; global motor strength -> all 12 STRENGTH words; inertia, mass -> their two ratios (mass over
 *   base mass in MASS_RATIO[0]); joint friction -> the four KNEE_FRICTION words, from the even ones of its eight draws; latency ->
 *   LATENCY; lateral friction -> FOOT_MU; leg weaken -> 1.0 on all 12 STRENGTH words, then the value on the three motors 3 leg ..
 *   3 leg + 2 of the drawn leg; motor strength -> the 12 STRENGTH words, a draw each; single leg weaken -> as leg weaken, on leg 0.
 * Draws, on the episode's (seed, robot index, episode) stream; every older block keeps its meaning: draws 0..25 as ever (inertia 0..1,
 *   joint friction 2..9, latency 10, lateral friction 11, mass 12..13, motor strength 14..25); block 0x40000000: word 0 base mass, word 1
 *   global motor strength, word 2 the weakened leg = (m * 4) >> 24 with m the draw's 24-bit integer, word 3 leg weaken's ratio; block
 *   0x40000001: word 0 single leg weaken.  In the parity replays these two blocks always come from Philox; draws 0..27 from uniforms_dev.
 * Refused, nothing changed (the message names the parameter): a null handle; for an enabled entry (a disabled one's bounds are not read) a NaN or infinite
 *   bound, lo > hi, lo <= 0 for base mass, mass or inertia, lo < 0 for the rest; a latency hi above (ORR_RING_DEPTH - 2) * sim_dt - the
 *   ring reader blends entries int(latency / sim_dt) and int(latency / sim_dt) + 1 back from the newest, and a ring of ORR_RING_DEPTH
 *   entries holds those for int(latency / sim_dt) + 1 <= ORR_RING_DEPTH - 1 (0.042 s at sim_dt 0.001); friction anchors on the handle
 *   (a launch refuses that combination too). */
int32_t orr_set_randomizer(orr_handle* h, const orr_randomizer* host);
int32_t orr_sizeof_randomizer(void);
/* The episode's normalised samples per robot (get_randomization_parameters / set_env_from_randomization_parameters).  Row of a robot:
 *   [0..25] draws 0..25, [26] base mass, [27] global motor strength, [28] the weakened leg as a float 0..3, [29] leg weaken's ratio
 *   draw, [30] single leg weaken, [31] 0.
 * suspend == 0: every reset (orr_reset, the auto-reset inside orr_step, orr_debug_replay_reset) writes the new episode's row - the
 *   draws, those of disabled parameters included.  suspend != 0 (suspend_randomization): a reset draws none of these; it reads the
 *   robot's row, applies it by the same rule and order and leaves the row alone.  The caller owns the row's contents.
 * params_dev NULL unbinds.  Refused, nothing changed: a null handle, a buffer that is not 16-byte aligned, friction anchors. */
#define ORR_RAND_ROW 32
int32_t orr_bind_randomizer_params(orr_handle* h, float* params_dev /* [N][ORR_RAND_ROW] */, int32_t suspend);

/* external pushes of the handle (the push randomiser of legged-robot training recipes; the reference ships none).  A push is a
 * velocity kick of the whole robot at the start of an env step: the record's LINVEL gets + dv and ANGVEL + dw, both world frame, after
 * the record is loaded and before anything reads the rigid state for the first sub-step.  Not a force: independent of mass, so one
 * setting serves a mixed batch; the joint rates are relative, so the legs move with the base; the sensors see the kick from the first
 * sub-step's ring entry on. */
typedef struct orr_push {
  float   prob;         /* probability of a kick per robot and env step, [0, 1] */
  float   lin_lo;       /* horizontal speed of the kick, m/s, 0 <= lin_lo <= lin_hi */
  float   lin_hi;
  float   lin_z;        /* vertical component in U(-lin_z, lin_z), >= 0 */
  float   ang;          /* each component of dw in U(-ang, ang), rad/s, >= 0 */
  int32_t grace_steps;  /* no kick while the episode's env-step counter is below it, >= 0 */
} orr_push;
/* host NULL = off.  While prob is 0 and no outputs are bound (orr_bind_push_outputs) the handle launches exactly the kernels it
 *   launched before; otherwise orr_step launches the push variant (a superset of the randomiser variant: one wave per SIMD at any batch
 *   size, unbound outputs skipped, zero noise passes the reading; its auto-reset is the table-driven one only while the handle has a
 *   randomiser table or params buffer, otherwise the one the handle ran before).  There is no reset and no replay kernel with pushes:
 *   orr_reset, orr_debug_replay_reset and orr_debug_replay_step of such a handle launch exactly what they launch without this call.
 *   The parity replay and orr_debug_physics IGNORE pushes: the replay replaces the physics by recorded states, the debug physics has no
 *   env step.  The variant's first launch in a process loads its code object: it must not happen inside a stream capture.
 * Draw rule, on the episode's (seed, robot index, episode) stream, ROBOT_INDEX and EPISODE_IDX as they are before the step; every older
 *   block keeps its meaning (sensor noise below 0x20000000, task noise 0x2... and 0x3..., the randomiser 0x40000000 and 0x40000001):
 *   s = EP_STEP before the step; block A = 0x50000000 + 2 s, block B = A + 1 (below 0x60000000 for s < 2^27); words are the stream's
 *   24-bit uniforms m / 2^24.
 *   The robot is kicked iff s >= grace_steps and A.word0 < prob (a float32 comparison of an exact fraction: the host can decide it).
 *   theta = 2 pi A.word1, formed as the normal pairs form their angle: k = rint(4 u) quarter turns, f = u - k / 4 exactly, a =
 *     fmaf(f, 2pi_hi, f 2pi_lo) with the two-part 2 pi, sine and cosine of a by the joint polynomial, the quarter turns applied after;
 *   m = fmaf(A.word2, lin_hi - lin_lo, lin_lo), lin_hi - lin_lo one float32 subtraction on the device;
 *   dv = (m cos theta, m sin theta, fmaf(A.word3, 2 lin_z, -lin_z));   dw_k = fmaf(B.word_k, 2 ang, -ang), k = 0..2.
 *   Block B is computed only while ang > 0 (dw = 0 otherwise).  A robot that is not kicked has dv = dw = 0 and its velocities pass
 *   as they are (selects, not + 0: a velocity of -0.0 keeps its sign), so "no kick" is bit for bit "no push variant".
 * Refused, nothing changed (the message names the field): a null handle; a NaN or infinite value; prob outside [0, 1]; a negative
 *   lin_lo, lin_hi, lin_z, ang or grace_steps; lin_lo > lin_hi; lin_hi, lin_z or ang above orr_config::max_coord_velocity (the physics
 *   clamps every coordinate velocity there anyway); friction anchors on the handle while prob > 0 (a launch refuses that combination
 *   too, and launches nothing, when such a model is set afterwards). */
int32_t orr_set_push(orr_handle* h, const orr_push* push_host);
int32_t orr_sizeof_push(void);
/* What the step did to each robot.  push_dev float[N][ORR_PUSH_ROW] (device, 16-byte aligned); NULL unbinds.  Every orr_step writes the
 *   row of every robot of the shard: words 0..5 {dv x y z, dw x y z} of this step, word 6 = 1.0 if the robot was kicked in this step else
 *   0.0, word 7 = the number of kicks in the robot's current episode including this step.  Word 7 restarts in the step whose EP_STEP
 *   before it is 0; no reset touches the buffer, so the caller zeroes it once.  With auto-reset the row is that of the step that ended
 *   the episode.  A step that ends with ORR_DONE_NAN still reports what was applied.  Padding lanes store nothing.  A bound buffer
 *   selects the push variant whatever prob is.
 * Refused, nothing changed: a null handle, a buffer that is not 16-byte aligned, friction anchors. */
#define ORR_PUSH_ROW 8
int32_t orr_bind_push_outputs(orr_handle* h, float* push_dev /* [N][ORR_PUSH_ROW] */);

/* Privileged observation: what the simulator knows about each robot and no sensor reports, for an asymmetric critic
 * (orr_policy_forward_priv, openroborl_policy.h).  priv_dev float[N][ORR_PRIV_DIM] (device, 16-byte aligned); done_dev uint8[N] = the
 * done flags of the step just taken, or NULL (after a reset).  One launch (csrc/orr_kernels_priv.hip); it reads, and changes nothing.
 * The row of robot i is built from its state record as it stands when the launch runs - the state the current observation belongs
 * to: after an auto-reset the new episode's - and from the output buffers the handle has bound at that moment:
 *   words 0..2    R^T LINVEL: the base's linear velocity in the base frame.  R = the rotation matrix of rel = QUAT (x) INIT_QUAT^-1 of
 *                 the robot's type (the orientation relative to the initial one that the observation's IMU reading starts from), by
 *                 the standard quaternion-to-matrix formula, rel not renormalised
 *         3..5    R^T ANGVEL
 *         6..8    R^T (0, 0, -1): the direction of gravity in the base frame
 *         9       POS[2]
 *         10..21  STRENGTH[12]
 *         22      LATENCY / ((ORR_RING_DEPTH - 2) * sim_dt)
 *         23      FOOT_MU
 *         24..27  KNEE_FRICTION[4] * 20
 *         28..31  MASS_RATIO[2], INERTIA_RATIO[2]
 *         32..35  per leg 1.0 if the contact row's normal sum (contact_dev[i][leg][0], orr_bind_contact_outputs) is > 0, else 0.0
 *         36..39  per leg that normal sum / (action_repeat * sim_dt) / 100: the step's mean normal force in units of 100 N
 *         40..45  push_dev[i][0..5] (orr_bind_push_outputs): dv, dw of the step
 *         46      EP_STEP / max(MAX_EP_STEPS, 1), both as floats
 *         47      0
 *   Words 32..39 are 0 while no contact outputs are bound and words 40..45 while no push outputs are bound.  Words 32..45 are also 0
 *   for a robot whose done_dev byte is non-zero (those buffers still describe the episode that ended, the record is the new one), and
 *   for every robot with done_dev == NULL (after a reset the buffers hold no step of the current episode).
 *   The divisors (ORR_RING_DEPTH - 2) * sim_dt and action_repeat * sim_dt are formed once on the host, in float32; the device
 *   multiplies and divides in float32 in the order written.
 * Refused, nothing written: a null handle or buffer, a priv_dev that is not 16-byte aligned, no state bound (orr_bind).  Friction
 * anchors are not refused: nothing here depends on them. */
#define ORR_PRIV_DIM 48
int32_t orr_privileged_obs(orr_handle* h, const uint8_t* done_dev, float* priv_dev, void* stream);

/* Reward shaping: effort, smoothness, impact and failure penalties taken off the imitation reward on the device.  This project's own:
 * the reference's reward is its five imitation terms and nothing else.  A post-step kernel (csrc/orr_kernels_shaping.hip), no variant of
 * the step: orr_step, orr_reset and the replays launch what they launch without it, and EP_RETURN, the episode log and the clip
 * curriculum's scores stay on the imitation reward.
 * orr_shaped_reward is ONE launch, called after the orr_step whose actions_dev [N][12], reward (reward_in_dev [N]) and done_dev [N] it is
 * given; reward_out_dev [N] may be reward_in_dev.  It reads the state record as it stands and the actuator / contact buffers the handle
 * has bound when the launch RUNS (orr_bind_actuator_outputs, orr_bind_contact_outputs), as orr_privileged_obs does.  For robot i, with
 *   a = its action row, A[m] = its act_dev row of motor m, C[leg] = its contact_dev row, r = reward_in[i], d = done[i] != 0,
 *   reason = DONE_REASON, n_step = d ? LAST_EP_LEN : EP_STEP (the number of the step just taken within its episode; both survive the
 *   auto-reset), a1 = prev[i][0..11], a2 = prev[i][12..23] (the actions of the two steps before),
 * the terms p_k, unweighted, in ORR_SHAPING_* order:
 *   0 torque        (sum_m A[m][2]) * inv_nsub: the mean square torque summed over the 12 motors, (N m)^2; inv_nsub = 1 / action_repeat
 *   1 work          sum_m |A[m][3]|, J
 *   2 action_rate   sum_j (a_j - a1_j)^2 if n_step >= 2, else 0
 *   3 action_accel  sum_j (a_j - 2 a1_j + a2_j)^2 if n_step >= 3, else 0
 *   4 impact        (sum_leg C[leg][3]) * inv_dt: the sum of the legs' peak normal forces, N; inv_dt = 1 / sim_dt
 *   5 failure       1.0 if d and reason & (CONTACT_FALL | ROOT_POS | ROOT_ROT | NAN), else 0.0: a time limit or a clip played to its
 *                   end is no failure
 *   inv_nsub and inv_dt are formed once on the host in float32; the 12- and 4-element sums are float32 adds in a fixed tree.  A step
 *   with reason & ORR_DONE_NAN writes terms 0..4 as 0 (the step has zeroed the buffers; the actions may be non-finite).  Terms 0 and 1
 *   are 0 while no actuator outputs are bound, term 4 while no contact outputs are bound.
 *   pen = sum_k w[k] p_k: float32, k ascending, a chain of fused multiply-adds from +0.  shaped = fmaxf(r - pen, floor), built from the
 *   very term values stored.
 * Stores (every row two 16-byte pieces; padding lanes store nothing; no atomics: the same inputs give the same bits):
 *   shape_dev[i]     = {p0..p5, shaped, 1.0f}
 *   shape_ep_dev[i]  is OVERWRITTEN with that row when n_step <= 1, otherwise it gets one float32 add per column (the rule of
 *                    term_sums_dev; no reset touches the buffer)
 *   shape_tot_dev[i] += shape_ep_dev[i] (its new value) when d; the kernel never restarts it, so column 7 counts the steps of the
 *                    robot's finished episodes
 *   prev_dev[i]      = {a, a1}
 *   reward_out[i]    = shaped
 * The weights and the floor live in the handle's device table, where the kernel reads them: a replayed graph follows
 * orr_set_reward_shaping without a re-capture.  The setter writes them in stream order on `stream` and synchronises nothing.
 * host NULL = off.  floor = -inf: none.  shape_dev NULL unbinds all four buffers.
 * Refused with a negative code, nothing launched or written (the message starts with the entry point's name): a null handle or
 *   pointer; no state bound (orr_bind); orr_shaped_reward while shaping is not set or the buffers are not bound; shape_dev without any
 *   of the other three; a row buffer, prev_dev or actions_dev that is not 16-byte aligned; reward_in / reward_out not 4-byte aligned; a
 *   weight that is negative, NaN or infinite; a floor that is NaN or +inf; at launch w[0] or w[1] != 0 without bound actuator outputs,
 *   or w[4] != 0 without bound contact outputs. */
#define ORR_SHAPING_TERMS 6
#define ORR_SHAPING_ROW 8
#define ORR_SHAPING_PREV 24 /* floats per robot of prev_dev */
enum orr_shaping_term_e { ORR_SHAPING_TORQUE, ORR_SHAPING_WORK, ORR_SHAPING_ACTION_RATE, ORR_SHAPING_ACTION_ACCEL, ORR_SHAPING_IMPACT, ORR_SHAPING_FAILURE };
typedef struct orr_reward_shaping {
  float w[ORR_SHAPING_TERMS];
  float floor;
} orr_reward_shaping;
int32_t orr_sizeof_reward_shaping(void);
int32_t orr_set_reward_shaping(orr_handle* h, const orr_reward_shaping* host /* NULL = off */, void* stream);
int32_t orr_bind_reward_shaping(orr_handle* h, float* shape_dev /* [N][8] */, float* shape_ep_dev /* [N][8] */, float* shape_tot_dev /* [N][8] */,
                                float* prev_dev /* [N][24] */);
int32_t orr_shaped_reward(orr_handle* h, const float* actions_dev, const float* reward_in_dev, const uint8_t* done_dev, float* reward_out_dev,
                          void* stream);

/* reward terms (ImitationTask._calc_reward_pose / _velocity / _end_effector / _root_pose / _root_velocity, imitation_task.py:358-516).
 * terms_dev float[N][5] (device): every orr_step and orr_debug_replay_step writes, for every robot of the shard, the five UNWEIGHTED
 *   terms r_k = exp(-scale_k err_k) of the reward it wrote to reward_dev, in orr_config::reward_w's order: pose, velocity, end effector,
 *   root pose, root velocity.  reward == sum_k reward_w[k] r_k, built from the very values stored.  A step that sets ORR_DONE_NAN
 *   writes five zeros (its reward is 0).
 * term_sums_dev float[N][5] (device): the running sums of the terms over the robot's current episode.  A step whose EP_STEP before
 *   the step is 0 OVERWRITES the row with that step's terms, every other step adds to it: after the step that ends an episode the row
 *   holds that episode's totals - with auto-reset too - until the robot's next step overwrites it.  No reset touches it.
 * term_log_dev float[ep_log_capacity][5] (device), or NULL: episode-log row `slot` also gets the ending episode's five sums, as
 *   orr_bind_clip_log adds the clip.  The capacity is orr_bind's; a dropped row (slot >= capacity) writes nothing.
 * terms_dev == NULL unbinds everything: the handle then launches exactly the kernels it launched before.  Otherwise term_sums_dev must
 * be non-NULL too.  While bound, orr_step and orr_debug_replay_step launch the terms variants of the step kernel (the task-noise variant
 * + these stores: one wave per SIMD at any batch size; with no clip set and all noise zero they compute what the default kernels
 * compute) and the resets the task-noise variant.  Refused, nothing changed: a null handle, terms_dev without term_sums_dev, a robot
 * type with friction anchors (a launch refuses the combination too when such a model is set afterwards). */
int32_t orr_bind_reward_terms(orr_handle* h, float* terms_dev, float* term_sums_dev, float* term_log_dev);

/* foot contact outputs: what the step kernel's ground-contact solver found, per robot and leg.  Legs in the order of the record's
 * LAMBDA field (slot 3 leg + d: normal, friction along world x, friction along world y).  Impulses in N s.
 * contact_dev float[N][16] (device), row = [leg 0..3][4]: every orr_step (orr_time_steps) and every orr_debug_physics writes, for every
 *   robot of the shard, per leg: [0] the sum over the launch's sub-steps (action_repeat of them; orr_debug_physics: its nsub) of the
 *   leg's normal contact impulse, [1] [2] the sums of its two friction impulses, [3] the largest normal impulse of any one sub-step.
 *   sum / (action_repeat * sim_dt) = the mean force over the step, in N.  The sums are plain float32 adds in sub-step order from 0, the
 *   maximum starts from 0 too; a leg without a contact row in a sub-step contributes the zeros that LAMBDA holds for it.  A step that
 *   sets ORR_DONE_NAN writes sixteen zeros.  With auto-reset the row is the step's that ended the episode; no reset touches the buffer.
 * contact_ep_dev float[N][8] (device), row = [leg 0..3][2], updated by orr_step only: [0] the number of env steps of the robot's
 *   current episode whose normal sum was > 0 (a float), [1] the sum of those normal sums.  A step whose EP_STEP before the step is 0
 *   OVERWRITES the row, every other step adds to it: after the step that ends an episode the row holds that episode's totals - with
 *   auto-reset too - until the robot's next step.  No reset touches it.
 * contact_log_dev float[ep_log_capacity][8] (device), or NULL: episode-log row `slot` also gets the ending episode's contact_ep row, as
 *   orr_bind_reward_terms adds the term sums.  The capacity is orr_bind's; a dropped row (slot >= capacity) writes nothing.
 * contact_dev == NULL unbinds everything: the handle then launches exactly the kernels it launched before.  Otherwise contact_ep_dev
 * must be non-NULL too, and every buffer given 16-byte aligned.  While bound, orr_step and orr_debug_physics launch the contact variants
 * of the step kernel (orr_step: the task-noise variant + the sums, also together with orr_bind_reward_terms; one wave per SIMD at any
 * batch size; with no clip set and all noise zero they compute what the default kernels compute) and the resets the task-noise
 * variant.  The parity replays (orr_debug_replay_step / _reset) replace the physics by recorded states: they run what they run
 * without the binding and leave the buffers alone.  Refused, nothing changed: a null handle, contact_dev without contact_ep_dev, a
 * misaligned buffer, a robot type with friction anchors (a launch refuses the combination too, and launches nothing, when such a
 * model is set afterwards). */
int32_t orr_bind_contact_outputs(orr_handle* h, float* contact_dev, float* contact_ep_dev, float* contact_log_dev);

/* motor torque limits and per-motor torque / work outputs: what the actuator chain did, per robot and motor (motor order).
 * MotorModel torque_limits (minitaur_motor.py:166-171): limits_host[12] in motor order, N m, applied to the
 * strength-scaled PD torque of every sub-step; +inf = no limit for that motor; NULL = none for the type.
 * 0 is legal (the motor is off).  The limits are the caller's data: a handle starts with none, and no shipped robot table carries any.
 * Refused, nothing changed: a null handle, a robot type out of range, a NaN or negative limit (the message names limits_host[i]), a
 * finite limit on a handle that has a robot type with friction anchors. */
int32_t orr_set_torque_limits(orr_handle* h, int32_t robot_type, const float* limits_host);

/* act_dev float[N][12][4], row [motor] = {sum tau, max |tau|, sum tau^2, W} over the launch's sub-steps (orr_step,
 *   orr_time_steps, orr_debug_replay_step); a step that sets ORR_DONE_NAN writes zeros; with auto-reset the row
 *   is that of the step that ended the episode; no reset touches it.
 *   tau = the motor-convention torque that went into the physics, after strength and limit (what orr_debug_replay_step's tau_out
 *   reports), N m.  W = sim_dt * sum tau_s * qd_s, qd_s = the motor-convention joint rate after sub-step s: with the semi-implicit
 *   integrator sim_dt * qd_s is the sub-step's change of the angle, so W is the discrete mechanical work in J.  All from 0, float32, in
 *   sub-step order; sum tau^2 and W by fused multiply-adds.
 * act_ep_dev float[N][4] = {sum over the episode's steps and the 12 motors of W,  the same of sum tau^2,
 *   the largest |tau| of the episode,  the number of env steps in which some motor's peak equalled its limit};
 *   overwritten by the step whose EP_STEP before it is 0, added to otherwise (orr_step only).
 * act_log_dev float[ep_log_capacity][4] or NULL: the ending episode's act_ep row, next to term_log / contact_log.
 * act_dev == NULL unbinds everything.  16-byte alignment required (one 16-byte store per motor lane).
 * While a robot type has a finite limit or the outputs are bound, orr_step and orr_debug_replay_step launch the actuator variants of the
 * step kernel (one wave per SIMD at any batch size; supersets of the task-noise, reward-terms and - orr_step - contact variants, which
 * serve orr_bind_reward_terms and orr_bind_contact_outputs where those are bound as well) and the resets the task-noise variant.  With
 * neither the handle launches exactly the kernels it launched before.  orr_debug_physics takes its torques as given: it applies no limit
 * and leaves these buffers alone.  Refused, nothing changed: a null handle, act_dev without act_ep_dev, a misaligned buffer, a robot
 * type with friction anchors (a launch refuses the combination too, and launches nothing, when such a model is set afterwards). */
int32_t orr_bind_actuator_outputs(orr_handle* h, float* act_dev, float* act_ep_dev, float* act_log_dev);

/* replaces WrapperEnv.reset (wrapper_env.py:87-107): mask_dev NULL = all robots; obs_dev [N,160]
 * (rows of robots that are not reset are left untouched). */
int32_t orr_reset(orr_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* replaces WrapperEnv.step (wrapper_env.py:58-85): actions [N,12] policy outputs (already clipped to
 * +-2pi by the caller, imitation_runners.py:140-143; NOT modified, unlike minitaur.py:281);
 * obs [N,160] (16-byte aligned), reward [N], done [N] (uint8).
 * One launch.  The library holds two builds of the same kernel source and picks by batch size: up to 4 robots x #SIMDs of the device
 * (4096 on an MI355X) one wave per SIMD, above that two waves per SIMD (identical results; the environment variable
 * ORR_STEP_WAVES_PER_EU = 1 | 2, read by orr_create, forces one of them - measurements and tests only). */
int32_t orr_step(orr_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                 void* stream);

/* replaces the rank-local side of MPI allgather((ep_lens, ep_rets)) + allreduce(total_timestep) at a rollout boundary
 * (agents/ppo_imitation.py:405-423): packs the episode log into the fixed-size float64 payload of ONE all-gather,
 *   out_dev[6 + 2 * capacity] = [n_listed, total_timesteps, n_dropped, n_episodes, sum_ret, sum_len, ret[capacity], len[capacity]],
 * and clears the log (one launch, no host sync; n_episodes / sums cover every logged episode, the lists the first `capacity`). */
int32_t orr_episode_stats(orr_handle* h, double total_timesteps, int32_t capacity, double* out_dev, void* stream);

/* parity / debug entry (not part of the drop-in surface): nsub physics sub-steps with fixed motor torques
 * [N,12] applied as tau_urdf = tau * JOINT_DIRECTIONS; fall_dev [N] receives the fall-proxy flag (may be NULL). */
int32_t orr_debug_physics(orr_handle* h, const float* torques_dev, uint8_t* fall_dev, int32_t nsub, void* stream);

/* parity / debug entries (not part of the drop-in surface): WrapperEnv.step / reset with the physics engine REPLAYED.
 * traj [N][action_repeat][37] = rigid state (POS QUAT LINVEL ANGVEL Q QD) after each sub-step, eff [N][2][8][3] = link positions
 * for the end-effector reward ([0] robot, [1] reference model; lower leg, toe per leg), fall [N] = non-foot ground contact,
 * tau_out [N][action_repeat][12] receives the motor torques; uniforms [N][28] = the draws of the reset in [0, 1).  They exist so
 * that the HIP path can be compared with fixtures recorded from the reference's own Python (tests/golden/make_golden_task.py). */
int32_t orr_debug_replay_step(orr_handle* h, const float* actions_dev, const float* traj_dev, const float* eff_dev,
                              const uint8_t* fall_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                              float* tau_out_dev, void* stream);
int32_t orr_debug_replay_reset(orr_handle* h, const float* uniforms_dev, float* obs_dev, void* stream);

/* last launch durations in ms measured with hipEvents on the launch stream (bench only; syncs) */
int32_t orr_time_steps(orr_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                       void* stream, int32_t num_steps, float* total_ms_out);

/* measurement input (bench only; no reference counterpart): the policy-free stress actions of SURVEY.md section 8d (i) in ONE launch for
 * any mix of robot types: actions[i][m] = clip((obs[i][84 + 7 + joint_of_motor[m]] - motor_offset[m]) * motor_dir[m]
 * - init_motor_angles[m] + noise[i][m], +-2 pi) with the table of robot i's type (obs [N,160], noise and actions [N,12], device). */
int32_t orr_stress_actions(orr_handle* h, const float* obs_dev, const float* noise_dev, float* actions_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENROBORL_HIP_H_ */
