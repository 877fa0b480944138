"""ctypes mirror of include/openroborl_hip.h (struct layouts and constants only)."""
import ctypes as C

ABI_VERSION = 5
NUM_MOTORS = 12
POSE_DIM = 19
VEL_DIM = 18
PROPRIO_DIM = 84
TARGET_DIM = 76
OBS_DIM = 160
MAX_ROBOT_TYPES = 32
MAX_CLIPS = 16
MAX_FALL_PROXIES = 16
RING_DEPTH = 44
RING_ENTRY = 20
STATE_STRIDE = 1216

DONE_CONTACT_FALL, DONE_ROOT_POS, DONE_ROOT_ROT, DONE_TIME_LIMIT, DONE_NAN, DONE_MOTION_OVER = 1, 2, 4, 8, 16, 32

FLAG_AUTO_RESET = 1
FLAG_RANDOMIZER = 2
FLAG_CYCLE_SYNC = 4
FLAG_LEGACY_GRID = 8
FLAG_CURRICULUM = 16

CLIP_WRAP, CLIP_CYCLE_POS, CLIP_CYCLE_ROT = 1, 2, 4

CNT_TOTAL_STEP_COUNT = 0
CNT_DONE_ACCUM = 1
CNT_TICKET = 2
CNT_TOTAL_TIMESTEPS = 3
CNT_EPISODES = 4
CNT_EPLOG_DROPPED = 5
NUM_COUNTERS = 8
# orr_bind_reward_terms: int32_t (orr_handle*, float* terms_dev [N][5], float* term_sums_dev [N][5], float* term_log_dev [ep_log_capacity][5] | NULL);
# the columns, in orr_config::reward_w's order
NUM_REWARD_TERMS = 5
REWARD_TERM_NAMES = ("pose", "velocity", "end_effector", "root_pose", "root_velocity")
# orr_bind_contact_outputs: int32_t (orr_handle*, float* contact_dev [N][16], float* contact_ep_dev [N][8], float* contact_log_dev [ep_log_capacity][8] | NULL);
# contact_dev row = [leg][normal sum, friction x sum, friction y sum, largest normal], contact_ep_dev row = [leg][stance steps, normal sum]
CONTACT_OUT_DIM = 16
CONTACT_EP_DIM = 8
CONTACT_COLUMNS = ("normal", "friction_x", "friction_y", "normal_max")
# orr_set_torque_limits: int32_t (orr_handle*, int32_t robot_type, const float* limits_host [12] | NULL); +inf = no limit
# orr_bind_actuator_outputs: int32_t (orr_handle*, float* act_dev [N][12][4], float* act_ep_dev [N][4], float* act_log_dev [ep_log_capacity][4] | NULL);
# act_dev row [motor] = ACTUATOR_COLUMNS, act_ep_dev row = ACTUATOR_EP_COLUMNS
ACTUATOR_OUT_DIM = 4
ACTUATOR_EP_DIM = 4
ACTUATOR_COLUMNS = ("torque_sum", "torque_peak", "torque_sq_sum", "work")
ACTUATOR_EP_COLUMNS = ("work", "torque_sq_sum", "torque_peak", "saturated_steps")


class OrrConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_robots", C.c_int32),
        ("action_repeat", C.c_int32),
        ("solver_iters", C.c_int32),
        ("sim_dt", C.c_float),
        ("gravity_z", C.c_float),
        ("reward_w", C.c_float * 5),
        ("reward_scale", C.c_float * 6),
        ("tar_frame_steps", C.c_int32 * 4),
        ("ref_state_init_prob", C.c_float),
        ("warmup_time", C.c_float),
        ("ep_len_start", C.c_int32),
        ("ep_len_end", C.c_int32),
        ("curriculum_steps", C.c_int64),
        ("seed", C.c_uint64),
        ("flags", C.c_int32),
        ("contact_erp", C.c_float),
        ("contact_margin", C.c_float),
        ("warmstart_factor", C.c_float),
        ("max_coord_velocity", C.c_float),
        ("plane_friction", C.c_float),
        ("limit_activation", C.c_float),
        ("max_angle_change", C.c_float),
        ("dist_fail_threshold", C.c_float),
        ("rot_fail_threshold", C.c_float),
        ("friction_erp", C.c_float),
    ]


class OrrModel(C.Structure):
    _fields_ = [
        ("init_pos", C.c_float * 3),
        ("init_quat", C.c_float * 4),
        ("init_motor_angles", C.c_float * 12),
        ("motor_dir", C.c_float * 12),
        ("motor_offset", C.c_float * 12),
        ("joint_of_motor", C.c_int32 * 12),
        ("kp", C.c_float * 12),
        ("kd", C.c_float * 12),
        ("base_mass", C.c_float),
        ("base_inertia", C.c_float * 6),
        ("link_mass", C.c_float * 12),
        ("link_com", (C.c_float * 3) * 12),
        ("link_inertia", (C.c_float * 6) * 12),
        ("link_inertia_pa", (C.c_float * 6) * 12),
        ("link_group", C.c_int32 * 12),
        ("joint_pos", (C.c_float * 3) * 12),
        ("joint_axis", (C.c_float * 3) * 12),
        ("joint_lo", C.c_float * 12),
        ("joint_hi", C.c_float * 12),
        ("toe_pos", (C.c_float * 3) * 4),
        ("lower_com", (C.c_float * 3) * 4),
        ("toe_radius", C.c_float),
        ("shank_pos", (C.c_float * 3) * 4),
        ("shank_radius", C.c_float),
        ("foot_friction", C.c_float),
        ("contact_stiffness", C.c_float),
        ("contact_damping", C.c_float),
        ("friction_anchor", C.c_int32),
        ("num_fall_proxies", C.c_int32),
        ("fall_body", C.c_int32 * MAX_FALL_PROXIES),
        ("fall_pos", (C.c_float * 3) * MAX_FALL_PROXIES),
        ("fall_radius", C.c_float * MAX_FALL_PROXIES),
    ]


class OrrTaskNoise(C.Structure):
    """include/openroborl_hip.h: orr_task_noise (orr_set_task_noise)."""
    _fields_ = [(n, C.c_float) for n in ("perturb_init_state_prob", "root_pos_std", "root_rot_std", "joint_pose_std", "root_vel_std",
                                         "root_ang_vel_std", "joint_vel_std", "tar_heading_std")]


SENSOR_NOISE_FIELDS = ("motor_angle_std", "motor_velocity_std", "motor_torque_std", "base_rpy_std", "base_rpy_rate_std")


class OrrSensorNoise(C.Structure):
    """include/openroborl_hip.h: orr_sensor_noise (orr_set_sensor_noise), Minitaur._observation_noise_stdev in its order."""
    _fields_ = [(n, C.c_float) for n in SENSOR_NOISE_FIELDS]


# include/openroborl_hip.h: ORR_RAND_*, the reference's parameter names in its application order (sorted by name)
RAND_PARAM_NAMES = ("base mass", "global motor strength", "inertia", "joint friction", "latency", "lateral friction", "leg weaken", "mass",
                    "motor strength", "single leg weaken")
RAND_NUM_PARAMS = len(RAND_PARAM_NAMES)
RAND_ROW = 32                       # ORR_RAND_ROW: floats per robot in the params buffer (orr_bind_randomizer_params)
RAND_BLOCK = 0x40000000             # Philox block of base mass, global motor strength, weakened leg, leg weaken's ratio; + 1: single leg weaken


class OrrRandomizer(C.Structure):
    """include/openroborl_hip.h: orr_randomizer (orr_set_randomizer)."""
    _fields_ = [("enabled", C.c_int32 * RAND_NUM_PARAMS), ("lo", C.c_float * RAND_NUM_PARAMS), ("hi", C.c_float * RAND_NUM_PARAMS)]


# include/openroborl_hip.h: orr_push (orr_set_push), ORR_PUSH_ROW (orr_bind_push_outputs)
PUSH_FIELDS = ("prob", "lin_lo", "lin_hi", "lin_z", "ang")
PUSH_ROW = 8                        # floats per robot in the outputs buffer: dv x y z, dw x y z, kicked, kicks of the episode
PUSH_BLOCK = 0x50000000             # Philox blocks of the step whose env-step counter before it is s: PUSH_BLOCK + 2 s (A) and + 2 s + 1 (B)


# include/openroborl_hip.h: ORR_PRIV_DIM (orr_privileged_obs) = include/openroborl_policy.h: ORR_POLICY_PRIV_DIM (orr_policy_forward_priv)
PRIV_DIM = 48
POLICY_PRIV_DIM = 48


# include/openroborl_hip.h: ORR_SHAPING_* and orr_reward_shaping (orr_set_reward_shaping, orr_bind_reward_shaping, orr_shaped_reward).  A row
# of the three sum buffers = the six unweighted terms in SHAPING_NAMES' order, the shaped reward, 1.0 (a step count once summed)
SHAPING_TERMS = 6
SHAPING_ROW = 8
SHAPING_PREV = 24                   # floats per robot of the prev buffer: the last two actions, the newer first
SHAPING_NAMES = ("torque", "work", "action_rate", "action_accel", "impact", "failure")
SHAPING_COLUMNS = SHAPING_NAMES + ("shaped_reward", "steps")


class OrrRewardShaping(C.Structure):
    """include/openroborl_hip.h: orr_reward_shaping (orr_set_reward_shaping)."""
    _fields_ = [("w", C.c_float * SHAPING_TERMS), ("floor", C.c_float)]


class OrrPush(C.Structure):
    """include/openroborl_hip.h: orr_push (orr_set_push)."""
    _fields_ = [(n, C.c_float) for n in PUSH_FIELDS] + [("grace_steps", C.c_int32)]


# include/openroborl_hip.h: ORR_CLIP_METRIC_* and orr_clip_curriculum (orr_set_clip_curriculum); a stats row of orr_clip_curriculum_update
CLIP_METRICS = ("length", "return", "step_reward")       # the index is the ORR_CLIP_METRIC_* value
CLIP_SCORE_ONE = 65536                                   # an episode's score is an integer in [0, CLIP_SCORE_ONE]
CLIP_STATS_COLS = 4                                      # n_c, S_c, S_c / (65536 n_c) or 0, ema_c


class OrrClipCurriculum(C.Structure):
    """include/openroborl_hip.h: orr_clip_curriculum (orr_set_clip_curriculum)."""
    _fields_ = [("alpha", C.c_float), ("eps", C.c_float), ("metric", C.c_int32), ("ref", C.c_float * MAX_CLIPS)]


def fill(struct, name, values):
    """Assign a (nested) python sequence / scalar to a ctypes struct field."""
    import numpy as np
    field = getattr(struct, name)
    if isinstance(field, C.Array):
        arr = np.ctypeslib.as_array(field)
        arr[...] = np.asarray(values, dtype=arr.dtype).reshape(arr.shape)
    else:
        setattr(struct, name, values)


class OrrPolicyNet(C.Structure):
    """include/openroborl_policy.h: orr_policy_net (packed weights + biases of the actor and the critic)."""
    _fields_ = [(n, C.c_void_p) for n in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi",
                                            "w0_vf", "b0_vf", "w1_vf", "b1_vf", "w2_vf", "b2_vf")]


class OrrHistoryEncoder(C.Structure):
    """include/openroborl_policy.h: orr_history_encoder (packed weights + biases of a history student's encoder, 512 -> 256 -> 48)."""
    _fields_ = [(n, C.c_void_p) for n in ("w0", "b0", "w1", "b1")]


# include/openroborl_policy.h: ORR_HISTORY_STEPS, ORR_HISTORY_FRAME, ORR_HISTORY_DIM (orr_history_push, orr_policy_forward_history)
HISTORY_STEPS = 16
HISTORY_FRAME = 32
HISTORY_DIM = 512


class OrrColsumJob(C.Structure):
    """include/openroborl_learner.h: orr_colsum_job."""
    _fields_ = [("partials", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32)]


class OrrUpdateCtl(C.Structure):
    """include/openroborl_learner.h: orr_update_ctl, twelve 32-bit words in device memory (UPDATE_CTL_WORDS names them in order)."""
    _fields_ = [("lr_mult", C.c_float), ("kl_lr_mult", C.c_float), ("grad_scale", C.c_float), ("skip", C.c_int32),
                ("grad_norm", C.c_float), ("grad_norm_max", C.c_float), ("grad_norm_sum", C.c_float), ("n_calls", C.c_int32),
                ("n_clipped", C.c_int32), ("n_nonfinite", C.c_int32), ("n_kl_skipped", C.c_int32), ("reserved", C.c_int32)]


UPDATE_CTL_WORDS = tuple(n for n, _ in OrrUpdateCtl._fields_)
UPDATE_CTL_SKIP_NONFINITE, UPDATE_CTL_SKIP_KL = 1, 2          # the bits of orr_update_ctl::skip
UPDATE_CONTROL_BLOCK_FLOATS = 1024                            # ORR_UPDATE_CONTROL_BLOCK_FLOATS
# include/openroborl_learner.h: int32_t orr_update_control(const float* g, int64_t n, float pre_scale, float max_norm, const float* kl | NULL,
#   float kl_stop, float kl_target, float kl_lr_lo, float kl_lr_hi, float* partials, orr_update_ctl* ctl, void* stream)
UPDATE_CONTROL_ARGS = [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                       C.c_void_p]
# include/openroborl_learner.h: int32_t orr_adam_step_ctl(orr_adam_step's arguments up to state, const orr_update_ctl* ctl, void* stream)
ADAM_STEP_CTL_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_void_p]


# include/openroborl_policy.h: int32_t orr_policy_forward_teacher(const orr_policy_net* net, const float* obs, const float* priv, int32_t n,
#   const float* noise, float std, float clip, float* action, float* raw, float* value | NULL, float* mean, void* stream) - orr_policy_forward_priv's
# arguments; w0_pi is a packed (160 + 48) x 512 matrix as well
POLICY_FORWARD_TEACHER_ARGS = [C.POINTER(OrrPolicyNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_distill_head(const float* mean [m][12], const float* target [m][12], int32_t m, float* g_mean [m][12],
#   float* gb_mean [12], float* stats [1], float* workspace, void* stream)
DISTILL_HEAD_ARGS = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_policy.h: int32_t orr_history_push(const float* obs [n][160], const uint8_t* done [n] | NULL, const float* prev [n][512] | NULL,
#   float* next [n][512], int32_t n, void* stream)
HISTORY_PUSH_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
# include/openroborl_policy.h: int32_t orr_policy_forward_history(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs,
#   const float* hist [n][512], int32_t n, const float* noise, float std, float clip, float* action, float* raw, float* value | NULL, float* mean,
#   float* latent [n][48] | NULL, void* stream)
POLICY_FORWARD_HISTORY_ARGS = [C.POINTER(OrrPolicyNet), C.POINTER(OrrHistoryEncoder), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_float,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_regress_head(const float* pred [m][c], const float* target [m][c], int32_t m, int32_t c, float* g [m][c],
#   float* gb [c], float* stats [1], float* workspace, void* stream)
REGRESS_HEAD_ARGS = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_history_student_head(const orr_policy_net* net (the *_pi members), const float* w2t, const float* w1t,
#   const float* w0zt (the three packed transposes), const float* obs [m][160], const float* z [m][48], const float* target_mean [m][12],
#   const float* target_priv [m][48], int32_t m, float action_coef, float latent_coef, float* g_z [m][48], float* mean [m][12] | NULL,
#   float* partials [student_head_rows(m)][48] + [rows][2], void* stream)
HISTORY_STUDENT_HEAD_ARGS = [C.POINTER(OrrPolicyNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                             C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_ppo_head_logstd(const float* mean [m][12], const float* value [m], const float* batch [m][16],
#   const float* log_std [12] (device), int32_t m, float clip, float vf_coef, float ent_coef, float* g_mean [m][12], float* g_value [m],
#   float* g_logstd [12], float* gb_mean [12], float* gb_value [1], float* stats [5], float* workspace, void* stream)
PPO_HEAD_LOGSTD_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_gauss_prepare(const float* noise [n][12], const float* log_std [12] (device), float* scaled [n][12],
#   float* logp [n] | NULL, int32_t n, void* stream)
GAUSS_PREPARE_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
# include/openroborl_policy.h: int32_t orr_policy_forward_history_priv(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs,
#   const float* hist [n][512], const float* priv [n][48] | NULL with value NULL, int32_t n, const float* noise, float std, float clip, float* action,
#   float* raw, float* value | NULL, float* mean, float* latent [n][48] | NULL, void* stream)
POLICY_FORWARD_HISTORY_PRIV_ARGS = [C.POINTER(OrrPolicyNet), C.POINTER(OrrHistoryEncoder), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_learner.h: int32_t orr_latent_backward(const float* g0 [m][512], const float* w0zt (packed [512][48]), const float* z [m][48] | NULL,
#   const float* target_priv [m][48] | NULL (both NULL with latent_coef 0 only), int32_t m, float latent_coef, float* g_z [m][48],
#   float* partials [latent_backward_rows(m)][48] + [rows][1], void* stream)
LATENT_BACKWARD_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]


# include/openroborl_learner.h: the statistics record of running observation normalisation, ORR_RUNNING_STATS_* (32-bit words of a record of
# d columns: int64 count + pad, then mean [d], var [d], rstd [d]) and the streaming pass's geometry
RUNNING_STATS_THREADS = 320
RUNNING_STATS_PASSES = 32
# int32_t orr_running_stats_update(const float* x [n][d], int64_t n, int32_t d, float eps, float* rec, float* partials, void* stream)
RUNNING_STATS_UPDATE_ARGS = [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
# int32_t orr_normalize_rows(const float* x [n][d], int64_t n, int32_t d, const float* mean [d], const float* rstd [d], float* out [n][d], void* stream)
NORMALIZE_ROWS_ARGS = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# include/openroborl_policy.h: int32_t orr_policy_pack_norm(const float* w [k][n], int32_t k, int32_t n, const float* mean [k], const float* rstd [k],
#   const float* b [n], float* out_w (packed), float* out_b [n], void* stream)
POLICY_PACK_NORM_ARGS = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def running_stats_floats(d):
    """ORR_RUNNING_STATS_FLOATS"""
    return 4 + 3 * int(d)


def running_stats_offsets(d):
    """ORR_RUNNING_STATS_MEAN, _VAR, _RSTD: the word offsets of the three arrays"""
    return 4, 4 + int(d), 4 + 2 * int(d)


def running_stats_pass_rows(d):
    """ORR_RUNNING_STATS_PASS_ROWS: whole rows a workgroup of the streaming pass reads at once"""
    return RUNNING_STATS_THREADS // (int(d) // 4)


def running_stats_block_rows(d):
    """ORR_RUNNING_STATS_BLOCK_ROWS: rows per workgroup = rows behind one [2][d] partial"""
    return RUNNING_STATS_PASSES * running_stats_pass_rows(d)


def student_head_rows(m):
    """include/openroborl_learner.h: ORR_STUDENT_HEAD_ROWS - the rows of partial sums orr_history_student_head leaves, one per 16 samples."""
    return (int(m) + 15) // 16


def latent_backward_rows(m):
    """include/openroborl_learner.h: ORR_LATENT_BACKWARD_ROWS - the rows of partial sums orr_latent_backward leaves, one per 16 samples."""
    return (int(m) + 15) // 16
