"""Host side of the MI355X-native quadruped imitation environment.

VecQuadrupedEnv  tensor-native: reset(mask=None) -> obs[N,160]; step(actions[N,12]) ->
                 (obs[N,160], reward[N], done[N], info) on torch.float32 ROCm tensors, no host sync,
                 per-robot masked auto-reset.  Mirrors the attribute surface the reference's agent
                 reads: num_robot, observation_space, action_space, env_step_counter, seed(), close()
                 (wrapper_env.py:55-56,58-107; quadruped_gym_env.py:59-61,149-152).
LegacyListEnv    the reference's exact list-of-numpy protocol (wrapper_env.py:58-107) including the
                 "caller resets the whole env when any robot is done" flow of
                 agents/imitation_runners.py:185-205, so a stable-baselines-style loop runs unchanged.

PyTorch only owns the device buffers and the stream; all per-robot work happens inside the HIP
kernels behind the C-ABI (include/openroborl_hip.h).
"""
import ctypes as C
import math

import numpy as np

from . import _abi, _lib, config as cfgmod, motion, robots, state as statemod


class Box(object):
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency): low / high / shape / dtype."""

    def __init__(self, low, high, dtype=np.float32):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = np.dtype(dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and np.all(x >= self.low) and np.all(x <= self.high)

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)

    def __repr__(self):
        return "Box(%s, %s)" % (self.shape, self.dtype)


def proprio_bounds():
    """Sensor bounds in flattened (sorted-name) order: IMU x3 | LastAction x3 | MotorAngle x3
    (robot_sensors.py:52-71,111-133; environment_sensors.py:37-38; sensor_wrappers.py:108-110)."""
    imu = np.array([2 * np.pi, 2 * np.pi, 2000 * np.pi, 2000 * np.pi])
    high = np.concatenate([np.tile(imu, 3), np.ones(36), np.pi * np.ones(36)])
    return -high, high


def target_bounds(clips):
    """ImitationTask.get_target_obs_bounds (imitation_task.py:303-335)."""
    low = np.inf * np.ones(_abi.POSE_DIM)
    high = -np.inf * np.ones(_abi.POSE_DIM)
    for c in clips:
        lo, hi = c.joint_bounds()
        low = np.minimum(low, lo)
        high = np.maximum(high, hi)
    low[0:3], high[0:3] = -2.0, 2.0
    low[3:7], high[3:7] = -1.0, 1.0
    return np.tile(low, 4), np.tile(high, 4)


def observation_space(clips):
    """WrapperEnv._build_observation_space (wrapper_env.py:127-145)."""
    pl, ph = proprio_bounds()
    tl, th = target_bounds(clips)
    return Box(np.concatenate([pl, tl]), np.concatenate([ph, th]), dtype=np.float32)


def motion_spec(motion_file, robot_names, mixed=False):
    """The motion-file argument -> (files in clip-id order, {robot name: clip set = list of clip ids}).

    Homogeneous batch (robot_names[0]): a path, or a list of paths = the robot's clip set (ImitationTask's ref_motion_filenames:
    every reset draws the episode's clip from it, imitation_task.py:694-701,1077-1085).  Mixed batch: one entry per robot name, each a
    path or a list.  Nothing is de-duplicated: a file listed twice is two clips (twice the weight).  A robot's initial CLIP_ID is its
    set's first entry."""
    def as_list(e):
        if isinstance(e, (list, tuple)):
            if not e:
                raise ValueError("a motion-file list must not be empty")
            for f in e:
                if isinstance(f, (list, tuple)):
                    raise ValueError("a clip set is a flat list of motion files")
            return list(e)
        if e is None:
            raise ValueError("no input robot or task")
        return [e]
    names = list(robot_names)
    if mixed:
        if not isinstance(motion_file, (list, tuple)) or len(motion_file) != len(names):
            raise ValueError("mixed batch needs one motion file (or list of motion files) per robot name")
        entries = list(motion_file)
    else:
        names, entries = names[:1], [motion_file]
    files, sets = [], {}
    for name, e in zip(names, entries):
        ids = []
        for f in as_list(e):
            ids.append(len(files))
            files.append(f)
        sets[name] = ids
    if len(files) > _abi.MAX_CLIPS:
        raise ValueError("%d motion clips; a batch holds at most %d" % (len(files), _abi.MAX_CLIPS))
    return files, sets


CLIP_DRAW = 28      # index of the clip draw in a reset's Philox stream (block 7, word 0; draws 0..27: randomiser, ref-state-init, time offset)


def clip_draw_index(m, n):
    """The entry of an n-clip set a reset picks (csrc/orr_task.h, reset_robot_state<true>): (m * n) >> 24, m = the 24-bit integer of draw
    CLIP_DRAW (the draw in [0, 1) is m / 2^24).  Integer arithmetic; works on numpy integer arrays."""
    return (np.asarray(m, dtype=np.int64) * int(n)) >> 24


CLIP_CHANGE_DRAW = 29   # the first clip change of an episode: draw 29 of the reset's stream (block 7, word 1)


def clip_switch_draws(ep_step):
    """Draw indices (clip, next change, time offset) of a mid-episode clip switch in the step whose env-step counter before the step
    is ep_step (csrc/orr_env_kernels.h, orr_step_kernel<.., CLIPS>): 32 + 4 s, 33 + 4 s, 34 + 4 s = Philox block 8 + s, words 0..2 of the
    episode's (seed, robot index, episode) stream.  The clip is set[clip_draw_index(m, n)] with m the 24-bit integer of the first."""
    d = 32 + 4 * np.asarray(ep_step, dtype=np.int64)
    return d, d + 1, d + 2


def clip_change_time(t, tmin, tmax, u):
    """The next clip change at motion time t (_reset_clip_change_time, imitation_task.py:1057-1069): t + tmin + (tmax - tmin) u in
    float64, stored as float32 (the record's CLIP_CHANGE_TIME); +inf where switching is off."""
    if not math.isfinite(tmax):
        return np.float32(np.inf)
    return np.float32(float(t) + (float(np.float32(tmin)) + (float(np.float32(tmax)) - float(np.float32(tmin))) * float(u)))


def clip_switch_spec(clip_time_min, clip_time_max, robot_names):
    """clip_time_min / clip_time_max (ImitationTask's kwargs: a float, or a dict by robot name for mixed batches; None = +inf) ->
    {robot name: (tmin, tmax)}.  (+inf, +inf) = no switching (the reference's default); otherwise both finite, 0 <= tmin <= tmax.
    ValueError on anything the C-ABI (orr_set_clip_switch) would refuse."""
    def per_name(v, name, what):
        if isinstance(v, dict):
            unknown = set(v) - set(robot_names)
            if unknown:
                raise ValueError("%s names robots that are not in this batch: %s" % (what, sorted(unknown)))
            v = v.get(name)
        if v is None:
            return math.inf
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number or a dict by robot name, not %r" % (what, v))
        return float(v)
    out = {}
    for name in robot_names:
        lo, hi = per_name(clip_time_min, name, "clip_time_min"), per_name(clip_time_max, name, "clip_time_max")
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError("clip_time_min / clip_time_max of %s: NaN" % name)
        if lo < 0 or hi < 0:
            raise ValueError("clip_time_min / clip_time_max of %s must not be negative" % name)
        if lo > hi:
            raise ValueError("clip_time_min > clip_time_max for %s" % name)
        if math.isinf(lo) != math.isinf(hi):
            raise ValueError("clip_time_min / clip_time_max of %s: both finite, or both inf (no switching)" % name)
        out[name] = (lo, hi)
    return out


def torque_limit_spec(torque_limits, robot_names):
    """torque_limits (MotorModel's kwarg, minitaur_motor.py:57-66: None, a float, 12 floats in motor order, or a dict of robot name to
    either, for mixed batches) -> {robot name: float32 [12]}, +inf = no limit.  ValueError on anything the C-ABI
    (orr_set_torque_limits) would refuse: NaN, a negative limit, a wrong length."""
    def one(v, name):
        if v is None:
            return np.full(12, np.inf, dtype=np.float32)
        if isinstance(v, (bool, np.bool_, str, dict)):
            raise ValueError("torque_limits of %s must be None, a number or 12 numbers in motor order, not %r" % (name, v))
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("torque_limits of %s must be None, a number or 12 numbers in motor order, not %r" % (name, v))
        if a.ndim == 0:
            a = np.full(12, float(a))
        if a.shape != (12,):
            raise ValueError("torque_limits of %s must be a number or 12 numbers in motor order, got shape %s" % (name, a.shape))
        if np.isnan(a).any() or (a < 0).any():
            raise ValueError("torque_limits of %s must be >= 0 (0 = the motor is off, inf = no limit), got %r" % (name, v))
        return a.astype(np.float32)
    if isinstance(torque_limits, dict):
        unknown = set(torque_limits) - set(robot_names)
        if unknown:
            raise ValueError("torque_limits names robots that are not in this batch: %s" % sorted(unknown))
        return {name: one(torque_limits.get(name), name) for name in robot_names}
    return {name: one(torque_limits, name) for name in robot_names}


# ---- task noise (orr_set_task_noise; ImitationTask's perturb_init_state_prob and tar_obs_noise) ------------------------------------
NOISE_RESET_BLOCK = 0x20000000      # Philox blocks 0x20000000 .. 0x20000008 of the episode's stream: the 36 uniforms U(k) of a reset's perturbation
NOISE_HEADING_BLOCK = 0x30000000    # block 0x30000000 + i: the heading noise of target observation i of the episode (tar_noise_block)
# _apply_state_perturb's standard deviations (imitation_task.py:1201-1206), by the names of orr_task_noise's fields
INIT_PERTURB_STD = {"root_pos_std": 0.025, "root_rot_std": 0.025 * math.pi, "joint_pose_std": 0.05 * math.pi, "root_vel_std": 0.1,
                    "root_ang_vel_std": 0.05 * math.pi, "joint_vel_std": 0.05 * math.pi}


def normal_pair(ua, ub):
    """The pair of standard normals the device makes of two stream uniforms (csrc/orr_device.h, normal_pair), in float64:
    r = sqrt(-2 ln(1 - ua)), (z0, z1) = r (cos, sin)(2 pi ub).  ua, ub in [0, 1) (either may be 0); works on arrays."""
    ua, ub = np.asarray(ua, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    r = np.sqrt(-2.0 * np.log1p(-ua))
    phi = 2.0 * np.pi * ub
    return r * np.cos(phi), r * np.sin(phi)


def init_perturb_draw_indices():
    """Draw indices (4 * block + word) of U(0) .. U(35), the uniforms of a reset's perturbation."""
    return 4 * NOISE_RESET_BLOCK + np.arange(36, dtype=np.int64)


def init_perturb_draws(U, prob, std=None):
    """What a reset does with its 36 uniforms U(k) (the stream's draws init_perturb_draw_indices(); shape [..., 36]) - the draw rule of
    include/openroborl_hip.h, orr_set_task_noise, in float64 with the float32 deviations the device holds.  Returns a dict:
    perturbed [...] bool (U(0) < prob), z [..., 32] the normals, axis [..., 3] (normalised; zero where its squared norm is below 1e-30),
    and the offsets the perturbed robots get on top of the reference state - pos [..., 2] (x, y), angle [...] (about axis), joints
    [..., 12], vel [..., 2], ang_vel [..., 3], joint_vel [..., 12] - and rot [..., 4], the xyzw quaternion that multiplies the reference
    rotation from the left."""
    U = np.asarray(U, dtype=np.float64)
    sd = {k: float(np.float32(v)) for k, v in dict(INIT_PERTURB_STD, **(std or {})).items()}
    z0, z1 = normal_pair(U[..., 4:36:2], U[..., 5:36:2])
    z = np.stack([z0, z1], axis=-1).reshape(U.shape[:-1] + (32,))
    a = -1.0 + 2.0 * U[..., 1:4]
    n2 = (a * a).sum(axis=-1, keepdims=True)
    axis = np.where(n2 < 1e-30, 0.0, a / np.sqrt(np.maximum(n2, 1e-300)))
    angle = sd["root_rot_std"] * z[..., 2]
    rot = np.concatenate([axis * np.sin(0.5 * angle)[..., None], np.cos(0.5 * angle)[..., None]], axis=-1)
    rot = np.where(n2 < 1e-30, np.array([0.0, 0.0, 0.0, 1.0]), rot)
    return {"perturbed": U[..., 0] < float(np.float32(prob)), "z": z, "axis": axis, "pos": sd["root_pos_std"] * z[..., 0:2], "angle": angle,
            "joints": sd["joint_pose_std"] * z[..., 3:15], "vel": sd["root_vel_std"] * z[..., 15:17],
            "ang_vel": sd["root_ang_vel_std"] * z[..., 17:20], "joint_vel": sd["joint_vel_std"] * z[..., 20:32], "rot": rot}


def tar_noise_block(ep_step_or_reset=None):
    """Philox block of a target observation's heading noise: NOISE_HEADING_BLOCK for the observation of a reset (None; the auto-reset
    inside a step included: the NEW episode's stream), NOISE_HEADING_BLOCK + 1 + s for the step whose env-step counter before the step
    is s.  The noise is tar_heading_std * z0 of normal_pair(word 0, word 1) = draws 4 * block, 4 * block + 1.  Works on integer arrays."""
    if ep_step_or_reset is None:
        return NOISE_HEADING_BLOCK
    return NOISE_HEADING_BLOCK + 1 + np.asarray(ep_step_or_reset, dtype=np.int64)


def task_noise_spec(perturb_init_state_prob=0.0, tar_obs_noise=None, init_perturb_std=None):
    """ImitationTask's perturb_init_state_prob / tar_obs_noise (a float, or a list whose first entry is used: the reference reads only
    [0]; None = off) and an optional dict overriding some of INIT_PERTURB_STD -> the orr_task_noise struct.  ValueError on anything
    the C-ABI (orr_set_task_noise) would refuse."""
    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number, not %r" % (what, v))
        return float(v)
    prob = number(0.0 if perturb_init_state_prob is None else perturb_init_state_prob, "perturb_init_state_prob")
    if not (0.0 <= prob <= 1.0):
        raise ValueError("perturb_init_state_prob must be a probability in [0, 1], not %r" % (prob,))
    if isinstance(tar_obs_noise, (list, tuple, np.ndarray)):
        if len(tar_obs_noise) == 0:
            raise ValueError("tar_obs_noise must not be empty (its first entry is the heading's standard deviation)")
        tar_obs_noise = number(tar_obs_noise[0], "tar_obs_noise[0]")
    vals = dict(INIT_PERTURB_STD, tar_heading_std=0.0 if tar_obs_noise is None else number(tar_obs_noise, "tar_obs_noise"))
    unknown = set(init_perturb_std or {}) - set(INIT_PERTURB_STD)
    if unknown:
        raise ValueError("init_perturb_std: unknown entries %s (known: %s)" % (sorted(unknown), sorted(INIT_PERTURB_STD)))
    for k, v in (init_perturb_std or {}).items():
        vals[k] = number(v, "init_perturb_std[%r]" % k)
    for k, v in vals.items():
        if not (0.0 <= v < math.inf):
            raise ValueError("%s must be a finite standard deviation >= 0, not %r" % ("tar_obs_noise" if k == "tar_heading_std" else k, v))
    return _abi.OrrTaskNoise(perturb_init_state_prob=prob, **vals)


# ---- sensor noise (orr_set_sensor_noise; Minitaur._observation_noise_stdev) ---------------------------------------------------------
SENSOR_NOISE_BLOCK = 0x10000000     # block 0x10000000 + (i << 9) + (slot << 4) + lane of the episode's stream (sensor_noise_block)
SENSOR_SLOT_HIST, SENSOR_SLOT_FILTER, SENSOR_SLOT_TARGET = 17, 18, 19   # slots 0..16: the sub-steps' motor-angle readings, two sub-steps a slot


def sensor_noise_block(i, slot, lane):
    """Philox block of a sensor-noise draw (include/openroborl_hip.h, orr_set_sensor_noise): i = 0 for a reset of the episode (the
    auto-reset inside a step included: the NEW episode's stream), 1 + s for the step whose env-step counter before it is s; slot
    0..16 = sub-steps 2 slot (words 0, 1) and 2 slot + 1 (words 2, 3), lane = motor; 17 = the sensor histories, lane = column (0..11
    motor angle, 12 roll, 13 pitch, 14 roll rate, 15 pitch rate); 18 = the filter history's initial value, lane = motor; 19 = the
    target observation's rpy, lane 0.  Works on integer arrays."""
    i, slot, lane = np.asarray(i, dtype=np.int64), np.asarray(slot, dtype=np.int64), np.asarray(lane, dtype=np.int64)
    if (i < 0).any() or (i >= 1 << 19).any() or (slot < 0).any() or (slot >= 32).any() or (lane < 0).any() or (lane >= 16).any():
        raise ValueError("sensor_noise_block: i in [0, 2^19), slot in [0, 32), lane in [0, 16)")
    return SENSOR_NOISE_BLOCK + (i << 9) + (slot << 4) + lane


def sensor_noise_normals(u4):
    """The four normals of a sensor-noise block from its four uniforms (shape [..., 4]): z0, z1 of the pair (word 0, word 1), then z0,
    z1 of the pair (word 2, word 3), by normal_pair, in float64.  Which of them a slot uses: sensor_noise_block."""
    u4 = np.asarray(u4, dtype=np.float64)
    a0, a1 = normal_pair(u4[..., 0], u4[..., 1])
    b0, b1 = normal_pair(u4[..., 2], u4[..., 3])
    return np.stack([a0, a1, b0, b1], axis=-1)


def sensor_noise_spec(observation_noise_stdev=None):
    """Minitaur._observation_noise_stdev (None = off, or five numbers: motor angle, motor velocity, motor torque, base rpy, base rpy
    rate; velocity and torque are kept and have no consumer on this path) -> the orr_sensor_noise struct.  ValueError on anything the
    C-ABI (orr_set_sensor_noise) would refuse; the message names the field."""
    if observation_noise_stdev is None:
        return _abi.OrrSensorNoise()
    if isinstance(observation_noise_stdev, (str, dict, bool, np.bool_)) or np.ndim(observation_noise_stdev) != 1 or len(observation_noise_stdev) != 5:
        raise ValueError("observation_noise_stdev must be None or five numbers (%s), not %r" % (", ".join(_abi.SENSOR_NOISE_FIELDS), observation_noise_stdev))
    vals = {}
    for name, v in zip(_abi.SENSOR_NOISE_FIELDS, observation_noise_stdev):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number, not %r" % (name, v))
        if not (0.0 <= float(v) < math.inf):       # NaN fails the comparison
            raise ValueError("%s must be a finite standard deviation >= 0, not %r" % (name, v))
        vals[name] = float(v)
    return _abi.OrrSensorNoise(**vals)


def sensor_noise_on(spec):
    """Whether the setting selects the sensor variants of the kernels: a deviation with a consumer is above 0."""
    return spec.motor_angle_std > 0.0 or spec.base_rpy_std > 0.0 or spec.base_rpy_rate_std > 0.0


# ---- domain randomisation (orr_set_randomizer, orr_bind_randomizer_params; ControllableEnvRandomizerFromConfig) ----------------------
RAND_NOOP_NAMES = ("battery", "motor friction")       # accepted and ignored: no-ops in the reference (minitaur_motor.py:86-102)
RAND_REFUSED_NAMES = {"control step": "every robot of a batch takes the same number of sub-steps per step",
                      "individual mass": "the engine scales masses by two ratios (base, legs), not per link",
                      "individual inertia": "the engine scales inertias by two ratios (base, legs), not per link",
                      "restitution": "the contact model has no restitution"}
RAND_POSITIVE_NAMES = ("base mass", "inertia", "mass")   # ratios that scale a mass or an inertia: lo > 0
# row words of the params buffer (include/openroborl_hip.h, orr_bind_randomizer_params) by parameter
RAND_ROW_WORDS = {"inertia": slice(0, 2), "joint friction": slice(2, 10), "latency": slice(10, 11), "lateral friction": slice(11, 12),
                  "mass": slice(12, 14), "motor strength": slice(14, 26), "base mass": slice(26, 27), "global motor strength": slice(27, 28),
                  "leg weaken": slice(28, 30), "single leg weaken": slice(30, 31)}
RAND_LEG_WORD = 28                                       # the weakened leg, as a float 0..3: not a draw in [0, 1)


def randomizer_latency_max(sim_dt=0.001):
    """The largest latency bound orr_set_randomizer accepts, in float32 as the C-ABI computes it: the ring reader blends the entries
    int(latency / sim_dt) and int(latency / sim_dt) + 1 back from the newest, and a ring of RING_DEPTH entries holds those while
    int(latency / sim_dt) + 1 <= RING_DEPTH - 1."""
    return float(np.float32(_abi.RING_DEPTH - 2) * np.float32(sim_dt))


def randomizer_spec(config, sim_dt=0.001):
    """The reference's randomiser configuration -> the orr_randomizer struct.  config: None (the built-in six ranges: what
    orr_set_randomizer(NULL) restores), "all_params" (the reference's dictionary of that name: the same six, as a table), or a dict of
    name -> [lo, hi] with the reference's names (_abi.RAND_PARAM_NAMES; "battery" and "motor friction" are accepted and ignored).
    ValueError, naming the entry, on "control step", "individual mass", "individual inertia", "restitution", an unknown name, a
    four-entry rejection range and anything the C-ABI would refuse."""
    if config is None or (isinstance(config, str) and config == "all_params"):
        config = cfgmod.RANDOMIZER_ALL_PARAMS
    if not isinstance(config, dict):
        raise ValueError("randomizer config must be None, \"all_params\" or a dict of parameter name to [lo, hi], not %r" % (config,))
    spec = _abi.OrrRandomizer()
    for name, rng in config.items():
        if name in RAND_REFUSED_NAMES:
            raise ValueError("randomizer parameter %r is not supported: %s" % (name, RAND_REFUSED_NAMES[name]))
        if name not in _abi.RAND_PARAM_NAMES and name not in RAND_NOOP_NAMES:
            raise ValueError("unknown randomizer parameter %r (known: %s)" % (name, ", ".join(_abi.RAND_PARAM_NAMES + RAND_NOOP_NAMES)))
        if isinstance(rng, (str, dict, bool, np.bool_)) or np.ndim(rng) != 1:
            raise ValueError("randomizer parameter %r: the range must be [lo, hi], not %r" % (name, rng))
        if len(rng) == 4:
            raise ValueError("randomizer parameter %r: four-entry rejection ranges [lo, hi, reject_lo, reject_hi] are not supported" % (name,))
        if len(rng) != 2:
            raise ValueError("randomizer parameter %r: the range must be [lo, hi], not %r" % (name, rng))
        for v in rng:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("randomizer parameter %r: the bounds must be numbers, not %r" % (name, rng))
        lo, hi = float(np.float32(rng[0])), float(np.float32(rng[1]))    # as the device holds them
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError("randomizer parameter %r: the bounds must be finite numbers, not %r" % (name, rng))
        if lo > hi:
            raise ValueError("randomizer parameter %r: lo > hi in %r" % (name, rng))
        if name in RAND_NOOP_NAMES:
            continue
        if name in RAND_POSITIVE_NAMES and not lo > 0.0:
            raise ValueError("randomizer parameter %r: lo must be > 0 (a ratio of a mass or an inertia), not %r" % (name, rng))
        if lo < 0.0:
            raise ValueError("randomizer parameter %r: lo must be >= 0, not %r" % (name, rng))
        if name == "latency" and hi > randomizer_latency_max(sim_dt):
            raise ValueError("randomizer parameter 'latency': hi = %r is beyond what the latency ring holds, (RING_DEPTH - 2) * sim_dt = %g s"
                             % (rng[1], randomizer_latency_max(sim_dt)))
        p = _abi.RAND_PARAM_NAMES.index(name)
        spec.enabled[p], spec.lo[p], spec.hi[p] = 1, lo, hi
    return spec


def randomizer_draw_indices():
    """Draw indices (4 * block + word; beyond 32 bits) on the episode's stream of the 31 uniforms behind a row of the params buffer, in
    row order: draws 0..25, then block RAND_BLOCK words 0..3 (base mass, global motor strength, the weakened leg's draw, leg weaken's
    ratio) and block RAND_BLOCK + 1 word 0 (single leg weaken).  Row word 28 is not the draw itself but the leg made of it
    (randomizer_row)."""
    return np.concatenate([np.arange(26, dtype=np.int64), 4 * _abi.RAND_BLOCK + np.arange(4, dtype=np.int64),
                           4 * (_abi.RAND_BLOCK + 1) + np.arange(1, dtype=np.int64)])


def randomizer_row(U):
    """The params-buffer row [..., RAND_ROW] (float64) that a reset writes for the 31 uniforms U [..., 31] of randomizer_draw_indices():
    the draws as they are, word 28 = the weakened leg (m * 4) >> 24 with m the draw's 24-bit integer, word 31 = 0."""
    U = np.asarray(U, dtype=np.float64)
    row = np.zeros(U.shape[:-1] + (_abi.RAND_ROW,))
    row[..., :31] = U
    m = np.floor(U[..., RAND_LEG_WORD] * 16777216.0).astype(np.int64)
    row[..., RAND_LEG_WORD] = ((m * 4) >> 24).astype(np.float64)
    return row


def randomizer_apply(spec, row):
    """What a reset writes into the record for a params-buffer row [..., RAND_ROW] under the table `spec` (randomizer_spec's struct):
    float64 predictions by the C-ABI's rule - value = lo + u (hi - lo) with the float32 bounds the device holds, a disabled parameter
    writes nothing, parameters apply in the reference's order (sorted by name) and a later one overwrites an earlier one's words.
    Returns a dict of record field -> array: STRENGTH [..., 12], MASS_RATIO [..., 2], INERTIA_RATIO [..., 2], KNEE_FRICTION [..., 4],
    LATENCY [..., 1], FOOT_MU [..., 1]; NaN marks a word that no enabled parameter writes (the record keeps its value)."""
    row = np.asarray(row, dtype=np.float64)
    lead = row.shape[:-1]
    out = {k: np.full(lead + (n,), np.nan) for k, n in (("STRENGTH", 12), ("MASS_RATIO", 2), ("INERTIA_RATIO", 2), ("KNEE_FRICTION", 4),
                                                        ("LATENCY", 1), ("FOOT_MU", 1))}
    leg = row[..., RAND_LEG_WORD]
    for p, name in enumerate(_abi.RAND_PARAM_NAMES):        # the application order
        if not spec.enabled[p]:
            continue
        lo, hi = float(spec.lo[p]), float(spec.hi[p])
        w = row[..., RAND_ROW_WORDS[name]]
        v = lo + (w[..., -1:] if name == "leg weaken" else w) * (hi - lo)
        if name == "base mass":
            out["MASS_RATIO"][..., 0:1] = v
        elif name == "global motor strength":
            out["STRENGTH"][...] = v
        elif name == "inertia":
            out["INERTIA_RATIO"][...] = v
        elif name == "joint friction":
            out["KNEE_FRICTION"][...] = v[..., 0::2]      # the knee joints take the even ones of the eight draws
        elif name == "latency":
            out["LATENCY"][...] = v
        elif name == "lateral friction":
            out["FOOT_MU"][...] = v
        elif name == "mass":
            out["MASS_RATIO"][...] = v
        elif name == "motor strength":
            out["STRENGTH"][...] = v
        else:                                             # leg weaken (the drawn leg), single leg weaken (leg 0)
            which = leg if name == "leg weaken" else np.zeros(lead)
            on = (np.arange(12) // 3) == which[..., None]
            out["STRENGTH"][...] = np.where(on, v, 1.0)
    return out


# ---- external pushes (orr_set_push, orr_bind_push_outputs) --------------------------------------------------------------------------
PUSH_KEYS = ("prob", "interval_s", "lin_vel", "lin_vel_z", "ang_vel", "grace_steps")


def push_spec(push=None, action_repeat=cfgmod.ACTION_REPEAT, sim_dt=0.001, max_coord_velocity=100.0):
    """The push setting -> the orr_push struct.  push: None (off) or a dict with `prob` (probability of a kick per robot and env step) or
    `interval_s` (mean time between kicks: prob = action_repeat * sim_dt / interval_s), `lin_vel` = (lo, hi) the kick's horizontal
    speed in m/s, `lin_vel_z` (vertical component in U(-z, z)), `ang_vel` (each component of the angular kick in U(-a, a), rad/s) and
    `grace_steps` (no kick while the episode's env-step counter is below it); every key but one of prob / interval_s is optional (0).
    ValueError on anything the C-ABI (orr_set_push) would refuse; the message names the field."""
    if push is None:
        return _abi.OrrPush()
    if not isinstance(push, dict):
        raise ValueError("push must be None or a dict with the keys %s, not %r" % (", ".join(PUSH_KEYS), push))
    for k in push:
        if k not in PUSH_KEYS:
            raise ValueError("unknown push key %r (known: %s)" % (k, ", ".join(PUSH_KEYS)))

    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("push: %s must be a number, not %r" % (name, v))
        if not math.isfinite(float(v)):
            raise ValueError("push: %s must be a finite number, not %r" % (name, v))
        if float(v) < 0.0:
            raise ValueError("push: %s must be >= 0, not %r" % (name, v))
        return float(v)

    if ("prob" in push) == ("interval_s" in push):
        raise ValueError("push: give exactly one of prob and interval_s")
    if "prob" in push:
        prob = number("prob", push["prob"])
    else:
        interval = number("interval_s", push["interval_s"])
        if not interval > 0.0:
            raise ValueError("push: interval_s must be > 0, not %r" % (push["interval_s"],))
        prob = float(action_repeat) * float(sim_dt) / interval
    if prob > 1.0:
        raise ValueError("push: %s gives a probability of %r per env step; it must lie in [0, 1]" % ("prob" if "prob" in push else "interval_s", prob))
    lin = push.get("lin_vel", (0.0, 0.0))
    if isinstance(lin, (str, dict)) or np.ndim(lin) != 1 or len(lin) != 2:
        raise ValueError("push: lin_vel must be (lo, hi), not %r" % (lin,))
    lo, hi = number("lin_vel lo", lin[0]), number("lin_vel hi", lin[1])
    if lo > hi:
        raise ValueError("push: lin_vel lo > hi in %r" % (lin,))
    z, ang = number("lin_vel_z", push.get("lin_vel_z", 0.0)), number("ang_vel", push.get("ang_vel", 0.0))
    for name, v in (("lin_vel hi", hi), ("lin_vel_z", z), ("ang_vel", ang)):
        if float(np.float32(v)) > float(np.float32(max_coord_velocity)):
            raise ValueError("push: %s = %r is above max_coord_velocity = %g (the physics clamps every coordinate velocity there)" % (name, v, max_coord_velocity))
    grace = push.get("grace_steps", 0)
    if isinstance(grace, (bool, np.bool_)) or not isinstance(grace, (int, np.integer)):
        raise ValueError("push: grace_steps must be an integer, not %r" % (grace,))
    if grace < 0 or grace >= 1 << 31:
        raise ValueError("push: grace_steps must be >= 0 (and below 2^31), not %r" % (grace,))
    return _abi.OrrPush(prob=prob, lin_lo=lo, lin_hi=hi, lin_z=z, ang=ang, grace_steps=int(grace))


def push_on(spec):
    """Whether the setting selects the push variant of the step kernel: the probability is above 0."""
    return spec.prob > 0.0


def push_block(s):
    """Philox blocks (A, B) of the push of the step whose env-step counter before it is s (include/openroborl_hip.h, orr_set_push):
    A = PUSH_BLOCK + 2 s, B = A + 1, on the stream (seed, robot index, episode) as they are before the step.  Works on integer arrays."""
    s = np.asarray(s, dtype=np.int64)
    if (s < 0).any() or (s >= 1 << 27).any():
        raise ValueError("push_block: s in [0, 2^27)")
    return _abi.PUSH_BLOCK + 2 * s, _abi.PUSH_BLOCK + 2 * s + 1


def push_kick(spec, u8, s=None):
    """What a step does with the eight uniforms u8 [..., 8] of its blocks A (words 0..3) and B (4..7) under the setting `spec`
    (push_spec's struct) - the draw rule of orr_set_push in float64, with the float32 settings the device holds (lin_hi - lin_lo as
    its one float32 subtraction).  s: the env-step counter(s) before the step, for the grace period (None = past it).
    -> (kicked [...] bool, dv [..., 3], dw [..., 3]); dv = dw = 0 where not kicked."""
    u8 = np.asarray(u8, dtype=np.float64)
    prob, lo, z, ang = (float(np.float32(getattr(spec, k))) for k in ("prob", "lin_lo", "lin_z", "ang"))
    span = float(np.float32(spec.lin_hi) - np.float32(spec.lin_lo))
    kicked = u8[..., 0] < prob
    if s is not None:
        kicked = kicked & (np.asarray(s, dtype=np.int64) >= int(spec.grace_steps))
    theta = 2.0 * np.pi * u8[..., 1]
    m = u8[..., 2] * span + lo
    dv = np.stack([m * np.cos(theta), m * np.sin(theta), u8[..., 3] * (2.0 * z) - z], axis=-1)
    dw = u8[..., 4:7] * (2.0 * ang) - ang if ang > 0.0 else np.zeros(u8.shape[:-1] + (3,))
    return kicked, np.where(kicked[..., None], dv, 0.0), np.where(kicked[..., None], dw, 0.0)


# ---- the privileged observation (orr_privileged_obs): the words of a robot's row, include/openroborl_hip.h ----
PRIV_DIM = _abi.PRIV_DIM
PRIV_FIELDS = {"base_lin_vel": slice(0, 3),          # R^T LINVEL, R = the rotation of QUAT (x) INIT_QUAT^-1 (base frame)
               "base_ang_vel": slice(3, 6),          # R^T ANGVEL
               "gravity": slice(6, 9),               # R^T (0, 0, -1)
               "height": slice(9, 10),               # POS[2]
               "motor_strength": slice(10, 22),      # STRENGTH
               "latency": slice(22, 23),             # LATENCY / ((RING_DEPTH - 2) * sim_dt)
               "foot_friction": slice(23, 24),       # FOOT_MU
               "knee_friction": slice(24, 28),       # KNEE_FRICTION * 20
               "mass_ratio": slice(28, 30),          # MASS_RATIO
               "inertia_ratio": slice(30, 32),       # INERTIA_RATIO
               "foot_contact": slice(32, 36),        # 1.0 / 0.0 per leg (contact outputs)
               "foot_force": slice(36, 40),          # mean normal force per leg in units of 100 N (contact outputs)
               "push": slice(40, 46),                # dv, dw of the step (push outputs)
               "episode_progress": slice(46, 47),    # EP_STEP / max(MAX_EP_STEPS, 1)
               "reserved": slice(47, 48)}            # 0


def action_space():
    """minitaur.py:145-148."""
    return Box(np.array([-2 * math.pi] * 12), np.array([2 * math.pi] * 12), dtype=np.float32)


class VecQuadrupedEnv(object):
    """N independent quadrupeds on one GPU; four robots per wavefront, 16 lanes each (see csrc/orr_env_kernels.h, orr_physics.h)."""

    TERM_NAMES = _abi.REWARD_TERM_NAMES      # the columns of reward_terms / episode_term_sums / the term log, in orr_config::reward_w's order

    def __init__(self, task_name=None, training_yaml=None, sim_yaml=None, device="cuda", num_robot=None, seed=None,
                 robot=None, motion_file=None, mode=None, enable_randomizer=None, auto_reset=True, num_procs=1,
                 robot_index_offset=0, legacy_grid=False, mixed_robots=None, ep_log_capacity=65536, config_overrides=None,
                 model_overrides=None, clip_time_min=None, clip_time_max=None, perturb_init_state_prob=None, tar_obs_noise=None,
                 init_perturb_std=None, reward_terms=False, contact_outputs=False, torque_limits=None, actuator_outputs=False,
                 observation_noise_stdev=None, randomizer_config=None, randomizer_params=False, push=None, push_outputs=False):
        import torch
        if not isinstance(push_outputs, (bool, np.bool_)):
            raise ValueError("push_outputs must be True or False, got %r" % (push_outputs,))
        if not isinstance(randomizer_params, (bool, np.bool_)):
            raise ValueError("randomizer_params must be True or False, got %r" % (randomizer_params,))
        if not isinstance(reward_terms, (bool, np.bool_)):
            raise ValueError("reward_terms must be True or False, got %r" % (reward_terms,))
        if not isinstance(contact_outputs, (bool, np.bool_)):
            raise ValueError("contact_outputs must be True or False, got %r" % (contact_outputs,))
        if not isinstance(actuator_outputs, (bool, np.bool_)):
            raise ValueError("actuator_outputs must be True or False, got %r" % (actuator_outputs,))
        # the values here, ahead of everything that needs the device; a dict's robot names below, once the batch's robots are known
        torque_limit_spec(torque_limits, sorted(torque_limits) if isinstance(torque_limits, dict) else ["every robot"])
        # sensor noise (Minitaur._observation_noise_stdev): off by default, as the reference ships it
        self.sensor_noise = sensor_noise_spec(observation_noise_stdev)
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("VecQuadrupedEnv needs a ROCm GPU (the HIP path has no CPU fallback)")
        self.L = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a cuda (ROCm) device")
        if self.device.index is not None:
            torch.cuda.set_device(self.device)   # the C-ABI library allocates / launches on the current HIP device
        params = {}
        if task_name is not None:
            params = cfgmod.load_training_params(task_name, training_yaml)
        sim = cfgmod.load_sim_params(sim_yaml)
        robot = robot or params.get("robot", "laikago")
        if robot not in robots.ROBOTS:
            raise ValueError("wrong robot select")                       # minitaur.py:97
        mode = mode or params.get("mode", "train")
        if enable_randomizer is None:
            enable_randomizer = bool(params.get("enable_env_randomizer", True)) and mode == "train"   # run.py:205-206
        num_robot = int(num_robot if num_robot is not None else params.get("num_robot", 1))
        seed = int(seed if seed is not None else params.get("seed", 0))
        motion_file = motion_file if motion_file is not None else params.get("motion_file")
        if motion_file is None:
            raise ValueError("no input robot or task")                   # quadruped_gym_env.py:50-51
        self.num_robot = num_robot
        self.mode = mode
        self.cfg = cfgmod.make_config(num_robot, sim_params=sim, mode=mode, enable_randomizer=enable_randomizer, seed=seed,
                                      num_procs=num_procs, auto_reset=auto_reset, legacy_grid=legacy_grid)
        for k, v in (config_overrides or {}).items():     # e.g. a shorter episode-length curriculum (WrapperEnv arguments, run.py:54-75)
            if not hasattr(self.cfg, k):
                raise ValueError("unknown orr_config field %r" % (k,))
            setattr(self.cfg, k, v)
        # robots: homogeneous batch, or interleaved heterogeneous batch (BASELINE config 5)
        if mixed_robots:
            self.robot_names = list(mixed_robots)
            robot_type = np.array([robots.ROBOT_TYPE_ID[self.robot_names[i % len(self.robot_names)]]
                                   for i in range(num_robot)], dtype=np.int32)
        else:
            self.robot_names = [robot]
            robot_type = np.full(num_robot, robots.ROBOT_TYPE_ID[robot], dtype=np.int32)
        self.models = [None] * _abi.MAX_ROBOT_TYPES
        # model_overrides = {robot name: {table entry: value}}: experiments on the hand-authored (parity-unpinned) entries of robots.py;
        # the entry "_build" = {keyword: value} replaces arguments of the table builder (link masses, COMs, hip position, ...)
        model_overrides = {k: dict(v) for k, v in (model_overrides or {}).items()}
        for name in set(self.robot_names):
            self.models[robots.ROBOT_TYPE_ID[name]] = robots.ROBOTS[name](**model_overrides.get(name, {}).pop("_build", {}))
        for name, over in model_overrides.items():
            m = self.models[robots.ROBOT_TYPE_ID[name]] if name in robots.ROBOT_TYPE_ID else None
            if m is None:
                raise ValueError("model_overrides names robot %r, which is not in this batch" % (name,))
            for k, v in over.items():
                if k not in m:
                    raise ValueError("unknown model table entry %r" % (k,))
                m[k] = np.asarray(v, dtype=np.asarray(m[k]).dtype).reshape(np.shape(m[k])) if np.ndim(m[k]) else type(m[k])(v)
        # clips: a clip set per robot type (one clip or several: every reset draws the episode's clip from the set), see motion_spec
        motion_files, self.clip_sets = motion_spec(motion_file, self.robot_names, mixed=bool(mixed_robots))
        self.clips = [motion.MotionClip(f) for f in motion_files]
        type_to_clip = {robots.ROBOT_TYPE_ID[n]: ids[0] for n, ids in self.clip_sets.items()}
        clip_id = np.array([type_to_clip[t] for t in robot_type], dtype=np.int32)
        self.multi_clip = any(len(ids) > 1 for ids in self.clip_sets.values())
        # mid-episode clip switching (ImitationTask's clip_time_min / clip_time_max; the task YAML may carry the same keys): every
        # U(tmin, tmax) seconds of motion time a robot draws a new clip from its set.  Off (inf) by default, as in the reference
        clip_time_min = clip_time_min if clip_time_min is not None else params.get("clip_time_min")
        clip_time_max = clip_time_max if clip_time_max is not None else params.get("clip_time_max")
        self.clip_switch = clip_switch_spec(clip_time_min, clip_time_max, sorted(set(self.robot_names)))
        # task noise (ImitationTask's perturb_init_state_prob / tar_obs_noise; the task YAML may carry the same keys): off by default, as in
        # the reference.  Validated here, ahead of anything that needs the device
        if perturb_init_state_prob is None:
            perturb_init_state_prob = params.get("perturb_init_state_prob", 0.0)
        if tar_obs_noise is None:
            tar_obs_noise = params.get("tar_obs_noise")
        if init_perturb_std is None:
            init_perturb_std = params.get("init_perturb_std")
        self.task_noise = task_noise_spec(perturb_init_state_prob, tar_obs_noise, init_perturb_std)
        # the randomiser's table (ControllableEnvRandomizerFromConfig's config; the task YAML may carry it as env_randomizer_config):
        # None = the built-in six ranges and the kernels that have them built in.  Validated here, ahead of anything that needs the device
        if randomizer_config is None:
            randomizer_config = params.get("env_randomizer_config")
        self.randomizer = randomizer_spec(randomizer_config, self.cfg.sim_dt)
        self.randomizer_config = randomizer_config
        # external pushes (orr_set_push; the task YAML may carry the dict under `push`, which applies in train mode only, like its
        # enable_env_randomizer): off by default.  Validated here likewise
        if push is None and mode == "train":
            push = params.get(cfgmod.PUSH_KEY)
        self.push = push_spec(push, self.cfg.action_repeat, self.cfg.sim_dt, self.cfg.max_coord_velocity)
        # motor torque limits (MotorModel's torque_limits): the user's data, none by default - no shipped robot table carries any
        self.torque_limits = torque_limit_spec(torque_limits, sorted(set(self.robot_names)))
        self.robot_type = robot_type
        self.clip_id = clip_id

        h = C.c_void_p()
        _lib.check(self.L.orr_create(C.byref(self.cfg), C.byref(h)), self.L)
        self.h = h
        for t, m in enumerate(self.models):
            if m is not None:
                _lib.check(self.L.orr_set_model(self.h, t, C.byref(robots.to_struct(m))), self.L)
        self._clip_tensors = []
        for i, c in enumerate(self.clips):
            fr = torch.tensor(c.frames, dtype=torch.float32, device=self.device).contiguous()
            fv = torch.tensor(c.frame_vels, dtype=torch.float32, device=self.device).contiguous()
            self._clip_tensors.append((fr, fv))
            cd = (C.c_float * 4)(*[float(x) for x in c.cycle_delta])
            _lib.check(self.L.orr_set_motion(self.h, i, fr.data_ptr(), fv.data_ptr(), c.num_frames,
                                             float(c.frame_duration), c.flags, cd), self.L)
        for name, ids in self.clip_sets.items():
            arr = (C.c_int32 * len(ids))(*ids)
            _lib.check(self.L.orr_set_clip_set(self.h, robots.ROBOT_TYPE_ID[name], arr, len(ids)), self.L)
        for name, (lo, hi) in self.clip_switch.items():
            if math.isfinite(lo):
                _lib.check(self.L.orr_set_clip_switch(self.h, robots.ROBOT_TYPE_ID[name], lo, hi), self.L)
        if self.task_noise.perturb_init_state_prob > 0.0 or self.task_noise.tar_heading_std > 0.0:
            _lib.check(self.L.orr_set_task_noise(self.h, C.byref(self.task_noise)), self.L)
        self.layout = statemod.Layout(self.L, "orr")
        idx = np.arange(num_robot, dtype=np.int32) + int(robot_index_offset)
        st = statemod.default_state(self.layout, num_robot, self.models, robot_type, clip_id, idx,
                                    legacy_grid=legacy_grid, ctrl_latency=cfgmod.CTRL_LATENCY,
                                    max_ep_steps=self.cfg.ep_len_end)
        self.state = torch.from_numpy(st).to(self.device).contiguous()
        self.counters = torch.zeros(_abi.NUM_COUNTERS, dtype=torch.int64, device=self.device)
        self.ep_log = torch.zeros((max(int(ep_log_capacity), 1), 2), dtype=torch.float32, device=self.device)
        _lib.check(self.L.orr_bind(self.h, self.state.data_ptr(), self.counters.data_ptr(), self.ep_log.data_ptr(),
                                   int(ep_log_capacity)), self.L)
        # clip of each logged episode (row = episode-log row): only where some set has more than one clip (the multi-clip kernels write it)
        self.clip_log = None
        if self.multi_clip:
            self.clip_log = torch.zeros(max(int(ep_log_capacity), 1), dtype=torch.int32, device=self.device)
            _lib.check(self.L.orr_bind_clip_log(self.h, self.clip_log.data_ptr()), self.L)
        # per-term reward outputs (orr_bind_reward_terms): the five unweighted terms of every step's reward, their running sums over each
        # robot's current episode and, next to the episode log, the sums of every logged episode.  While bound, the steps run the
        # terms variant of the kernel
        self.reward_terms = self.episode_term_sums = self.term_log = None
        # foot contact outputs (orr_bind_contact_outputs): per leg the sums of every step's normal and friction impulses and its largest
        # normal impulse, stance steps and normal sum over each robot's current episode and, next to the episode log, those of every
        # logged episode.  While bound, the steps and the debug physics run the contact variants of the kernel
        self.contact_out = self.episode_contact = self.contact_log = None
        # actuator outputs (orr_bind_actuator_outputs): per motor the sum, the peak and the sum of squares of every step's sub-step torques
        # and its mechanical work, work / sum of squares / peak / saturated steps over each robot's current episode and, next to the
        # episode log, those of every logged episode.  While bound or while a type has a torque limit, the steps run the actuator variant
        self.actuator_out = self.episode_actuator = self.actuator_log = None
        # the three outputs of a step are views into ONE device buffer [obs N x 160 f32 | reward N f32 | done N u8], so that a host-side
        # consumer (LegacyListEnv) fetches them with a single copy
        nb_obs, nb_rew = num_robot * _abi.OBS_DIM * 4, num_robot * 4
        self._out = torch.zeros(nb_obs + nb_rew + num_robot, dtype=torch.uint8, device=self.device)
        self.obs = self._out[:nb_obs].view(torch.float32).view(num_robot, _abi.OBS_DIM)
        self.reward = self._out[nb_obs:nb_obs + nb_rew].view(torch.float32)
        self.done = self._out[nb_obs + nb_rew:]
        self.observation_space = observation_space(self.clips)
        self.action_space = action_space()
        self._env_step_counter = 0
        self._closed = False
        self.launch_params_generation = 0     # bumped whenever something a launch takes by value changes (seed()): see there
        if reward_terms:
            self.bind_reward_terms(True)
        if contact_outputs:
            self.bind_contact_outputs(True)
        if any(np.isfinite(v).any() for v in self.torque_limits.values()):
            self.set_torque_limits(torque_limits)
        if actuator_outputs:
            self.bind_actuator_outputs(True)
        if sensor_noise_on(self.sensor_noise):
            self.set_sensor_noise(observation_noise_stdev)
        # the episode's normalised samples per robot (orr_bind_randomizer_params): None while unbound
        self.randomizer_rows = None
        self.randomizer_suspended = False
        if randomizer_config is not None:
            self.set_randomizer(randomizer_config)
        if randomizer_params:
            self.bind_randomizer_params(True)
        # what the pushes did to each robot (orr_bind_push_outputs): None while unbound
        self.push_out = None
        if push_on(self.push):
            self.set_push(push)
        if push_outputs:
            self.bind_push_outputs(True)

    # ---- reference attribute surface -------------------------------------------------------
    @property
    def env_step_counter(self):
        """quadruped_gym_env.py:336-337 (env-global in the reference; here: steps since the last full reset)."""
        return self._env_step_counter

    @property
    def env_time_step(self):
        return self.cfg.action_repeat * self.cfg.sim_dt

    def seed(self, seed=None):
        """quadruped_gym_env.py:59-61.  The RNG is counter-based (Philox keyed by seed, global robot index, episode index):
        a new seed takes effect for every episode that starts after this call.  Returns [seed] like gym."""
        if seed is not None and (int(seed) & 0xFFFFFFFFFFFFFFFF) != int(self.cfg.seed):
            self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            _lib.check(self.L.orr_set_seed(self.h, self.cfg.seed), self.L)
            # orr_step / orr_reset pass the handle's configuration (seed included) BY VALUE as a kernel argument: a hipGraph captured
            # before this call replays the old seed.  Holders of such graphs (rollout.GraphRollout) compare this counter and re-capture
            self.launch_params_generation += 1
        return [int(self.cfg.seed)]

    def close(self):
        if not self._closed and self.h:
            self.torch.cuda.synchronize(self.device)
            self.L.orr_destroy(self.h)
            self.h = None
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_task_noise(self, perturb_init_state_prob=0.0, tar_obs_noise=None, init_perturb_std=None):
        """Change the task noise of a running env (orr_set_task_noise): read from the next launch on.  All defaults = off.  A launch
        takes nothing of it by value, but it selects the kernel variant: holders of captured graphs re-capture (launch_params_generation)."""
        spec = task_noise_spec(perturb_init_state_prob, tar_obs_noise, init_perturb_std)
        _lib.check(self.L.orr_set_task_noise(self.h, C.byref(spec)), self.L)
        self.task_noise = spec
        self.launch_params_generation += 1

    def set_sensor_noise(self, observation_noise_stdev=None):
        """Change the sensor noise of a running env (orr_set_sensor_noise; Minitaur._observation_noise_stdev: None = off, or the five
        standard deviations of motor angle, motor velocity, motor torque, base rpy and base rpy rate): read from the next launch on.
        It selects the kernel variant: holders of captured graphs re-capture (launch_params_generation)."""
        spec = sensor_noise_spec(observation_noise_stdev)
        _lib.check(self.L.orr_set_sensor_noise(self.h, C.byref(spec)), self.L)
        self.sensor_noise = spec
        self.launch_params_generation += 1

    def set_randomizer(self, config=None):
        """Change the randomiser's table of a running env (orr_set_randomizer; see randomizer_spec for `config`): read by every reset
        from the next launch on, while the env randomises at all (enable_randomizer).  None restores the built-in six ranges and the
        kernels that have them built in; anything else - "all_params" too - runs the randomiser variants.  It selects the kernel
        variant: holders of captured graphs re-capture (launch_params_generation)."""
        spec = randomizer_spec(config, self.cfg.sim_dt)
        _lib.check(self.L.orr_set_randomizer(self.h, None if config is None else C.byref(spec)), self.L)
        self.randomizer, self.randomizer_config = spec, config
        self.launch_params_generation += 1

    def bind_randomizer_params(self, on=True, suspend=False):
        """Bind (allocating on first use) or unbind the randomiser's params buffer (orr_bind_randomizer_params): env.randomizer_rows
        [N, 32], a robot's row = the normalised samples of its current episode (layout: include/openroborl_hip.h).  suspend=False: every
        reset writes the new episode's row.  suspend=True (the reference's suspend_randomization): resets draw nothing and apply the
        rows as they stand (set_randomization_parameters).  It selects the kernel variant: holders of captured graphs re-capture
        (launch_params_generation); the variant's first launch in a process loads its code object, so step once eagerly before a capture."""
        t = self.torch
        if on:
            rows = self.randomizer_rows
            if rows is None:
                rows = t.zeros((self.num_robot, _abi.RAND_ROW), dtype=t.float32, device=self.device)
                rows[:, :31] = 0.5          # mid-range until a reset writes them (suspended from the start: every parameter at its centre)
                rows[:, RAND_LEG_WORD] = 0.0
            t.cuda.synchronize(self.device)
            _lib.check(self.L.orr_bind_randomizer_params(self.h, rows.data_ptr(), 1 if suspend else 0), self.L)
            self.randomizer_rows, self.randomizer_suspended = rows, bool(suspend)
        else:
            t.cuda.synchronize(self.device)      # launches in flight still write the buffer
            _lib.check(self.L.orr_bind_randomizer_params(self.h, None, 0), self.L)
            self.randomizer_rows, self.randomizer_suspended = None, False
        self.launch_params_generation += 1

    def set_push(self, push=None):
        """Change the external pushes of a running env (orr_set_push; see push_spec for `push`, None = off): read from the next step on.
        A probability above 0 selects the push variant of the step kernel: holders of captured graphs re-capture
        (launch_params_generation); the variant's first launch in a process loads its code object, so step once eagerly before a capture."""
        spec = push_spec(push, self.cfg.action_repeat, self.cfg.sim_dt, self.cfg.max_coord_velocity)
        _lib.check(self.L.orr_set_push(self.h, None if push is None else C.byref(spec)), self.L)
        self.push = spec
        self.launch_params_generation += 1

    def bind_push_outputs(self, on=True):
        """Bind (allocating on first use) or unbind the push outputs (orr_bind_push_outputs): env.push_out [N, 8], a robot's row = dv x y
        z, dw x y z of the last step (world frame, zeros where the robot was not kicked), 1.0 / 0.0 whether it was kicked, and the
        number of kicks in its current episode including that step; None while unbound.  Privileged information: no observation holds
        it.  A bound buffer selects the push variant whatever the probability: holders of captured graphs re-capture
        (launch_params_generation); the variant's first launch in a process loads its code object, so step once eagerly before a capture."""
        t = self.torch
        t.cuda.synchronize(self.device)          # launches in flight still write the buffer
        if on:
            out = self.push_out if self.push_out is not None else t.zeros((self.num_robot, _abi.PUSH_ROW), dtype=t.float32, device=self.device)
            _lib.check(self.L.orr_bind_push_outputs(self.h, out.data_ptr()), self.L)
            self.push_out = out
        else:
            _lib.check(self.L.orr_bind_push_outputs(self.h, None), self.L)
            self.push_out = None
        self.launch_params_generation += 1

    def get_randomization_parameters(self):
        """ControllableEnvRandomizerFromConfig.get_randomization_parameters for the whole batch: a dict of parameter name -> tensor [N,
        k] of the current episodes' samples in the reference's param_bounds units, -1 + 2 u ("leg weaken": [leg index as it is, -1 + 2 u]),
        for the enabled parameters.  Needs the params buffer (randomizer_params=True / bind_randomizer_params)."""
        if self.randomizer_rows is None:
            raise ValueError("no randomizer params: the env was built without randomizer_params=True")
        out = {}
        for p, name in enumerate(_abi.RAND_PARAM_NAMES):
            if self.randomizer.enabled[p]:
                v = 2.0 * self.randomizer_rows[:, RAND_ROW_WORDS[name]] - 1.0
                if name == "leg weaken":
                    v[:, 0] = self.randomizer_rows[:, RAND_LEG_WORD]
                out[name] = v
        return out

    def set_randomization_parameters(self, parameters):
        """set_env_from_randomization_parameters for the whole batch: write the rows from a dict like get_randomization_parameters' (name
        -> [N, k] or [k], samples in [-1, 1]; "leg weaken": [leg 0..3, sample]).  Resets apply them while the buffer is bound with
        suspend=True; parameters that are left out keep their words."""
        if self.randomizer_rows is None:
            raise ValueError("no randomizer params: the env was built without randomizer_params=True")
        t = self.torch
        rows = self.randomizer_rows.clone()
        for name, v in parameters.items():
            if name not in RAND_ROW_WORDS:
                raise ValueError("unknown randomizer parameter %r (known: %s)" % (name, ", ".join(_abi.RAND_PARAM_NAMES)))
            sl = RAND_ROW_WORDS[name]
            v = t.as_tensor(v, dtype=t.float32, device=self.device)
            v = v.reshape(-1, sl.stop - sl.start).clone()
            if v.shape[0] not in (1, self.num_robot):
                raise ValueError("randomizer parameter %r: expected %d values per robot for 1 or %d robots" % (name, sl.stop - sl.start, self.num_robot))
            u = (v + 1.0) * 0.5
            if name == "leg weaken":
                u[:, 0] = v[:, 0]
                if bool(((v[:, 0] != v[:, 0].round()) | (v[:, 0] < 0) | (v[:, 0] > 3)).any()):
                    raise ValueError("randomizer parameter 'leg weaken': the leg must be 0, 1, 2 or 3")
                smp = v[:, 1]
            else:
                smp = v
            if bool(((smp < -1.0) | (smp > 1.0) | (smp != smp)).any()):
                raise ValueError("randomizer parameter %r: samples must lie in [-1, 1]" % (name,))
            rows[:, sl] = u
        self.randomizer_rows.copy_(rows)

    def bind_reward_terms(self, on=True):
        """Bind (allocating on first use) or unbind the per-term reward outputs (orr_bind_reward_terms): env.reward_terms [N, 5], valid
        after step / replay_step, env.episode_term_sums [N, 5] and env.term_log [ep_log_capacity, 5]; all None while unbound.  It
        selects the kernel variant: holders of captured graphs re-capture (launch_params_generation)."""
        t = self.torch
        if on:
            n = _abi.NUM_REWARD_TERMS
            bufs = (t.zeros((self.num_robot, n), dtype=t.float32, device=self.device), t.zeros((self.num_robot, n), dtype=t.float32, device=self.device),
                    t.zeros((self.ep_log.shape[0], n), dtype=t.float32, device=self.device))
            _lib.check(self.L.orr_bind_reward_terms(self.h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()), self.L)
            self.reward_terms, self.episode_term_sums, self.term_log = bufs
        else:
            t.cuda.synchronize(self.device)      # launches in flight still write the buffers
            _lib.check(self.L.orr_bind_reward_terms(self.h, None, None, None), self.L)
            self.reward_terms = self.episode_term_sums = self.term_log = None
        self.launch_params_generation += 1

    def bind_contact_outputs(self, on=True):
        """Bind (allocating on first use) or unbind the foot contact outputs (orr_bind_contact_outputs): env.contact_out [N, 16] (row =
        [leg][normal sum, friction x sum, friction y sum, largest normal], N s; valid after step / debug_physics), env.episode_contact
        [N, 8] (row = [leg][stance steps, normal sum] of the robot's current episode) and env.contact_log [ep_log_capacity, 8]; all None
        while unbound.  It selects the kernel variant: holders of captured graphs re-capture (launch_params_generation); the variant's
        first launch in a process loads its code object, so step once eagerly before a capture (GraphRollout's first segment does)."""
        t = self.torch
        if on:
            bufs = (t.zeros((self.num_robot, _abi.CONTACT_OUT_DIM), dtype=t.float32, device=self.device),
                    t.zeros((self.num_robot, _abi.CONTACT_EP_DIM), dtype=t.float32, device=self.device),
                    t.zeros((self.ep_log.shape[0], _abi.CONTACT_EP_DIM), dtype=t.float32, device=self.device))
            _lib.check(self.L.orr_bind_contact_outputs(self.h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()), self.L)
            self.contact_out, self.episode_contact, self.contact_log = bufs
        else:
            t.cuda.synchronize(self.device)      # launches in flight still write the buffers
            _lib.check(self.L.orr_bind_contact_outputs(self.h, None, None, None), self.L)
            self.contact_out = self.episode_contact = self.contact_log = None
        self.launch_params_generation += 1

    def _contact_rows(self):
        if self.contact_out is None:
            raise ValueError("no contact outputs: the env was built without contact_outputs=True")
        return self.contact_out.view(self.num_robot, 4, 4)

    def foot_contact(self):
        """bool [N, 4]: the leg touched the ground in the last step (its normal impulse sum is > 0).  Needs contact_outputs=True."""
        return self._contact_rows()[:, :, 0] > 0

    def foot_forces(self):
        """float32 [N, 4, 3]: each leg's mean contact force over the last step in N (normal, friction along world x, along world y):
        the impulse sums divided by action_repeat * sim_dt.  Needs contact_outputs=True."""
        return self._contact_rows()[:, :, 0:3] / (self.cfg.action_repeat * self.cfg.sim_dt)

    def foot_peak_force(self):
        """float32 [N, 4]: each leg's largest normal force of any one sub-step of the last step, in N.  Needs contact_outputs=True."""
        return self._contact_rows()[:, :, 3] / self.cfg.sim_dt

    def set_torque_limits(self, torque_limits=None):
        """Set the motors' torque limits (orr_set_torque_limits; MotorModel's torque_limits): None = none, a float, 12 floats in motor
        order, or a dict of robot name to either.  In N m, applied to the strength-scaled PD torque of every sub-step, read from the
        next launch on.  It selects the kernel variant: holders of captured graphs re-capture (launch_params_generation)."""
        spec = torque_limit_spec(torque_limits, sorted(set(self.robot_names)))
        for name, lim in spec.items():
            arr = (C.c_float * 12)(*[float(x) for x in lim])
            _lib.check(self.L.orr_set_torque_limits(self.h, robots.ROBOT_TYPE_ID[name], arr), self.L)
        self.torque_limits = spec
        self.launch_params_generation += 1

    def bind_actuator_outputs(self, on=True):
        """Bind (allocating on first use) or unbind the actuator outputs (orr_bind_actuator_outputs): env.actuator_out [N, 12, 4] (row
        [motor] = [sum tau, max |tau|, sum tau^2, work] over the step's sub-steps; valid after step / replay_step), env.episode_actuator
        [N, 4] (work, sum tau^2, largest |tau|, saturated steps of the robot's current episode) and env.actuator_log [ep_log_capacity,
        4]; all None while unbound.  It selects the kernel variant: holders of captured graphs re-capture (launch_params_generation); the
        variant's first launch in a process loads its code object, so step once eagerly before a capture."""
        t = self.torch
        if on:
            bufs = (t.zeros((self.num_robot, _abi.NUM_MOTORS, _abi.ACTUATOR_OUT_DIM), dtype=t.float32, device=self.device),
                    t.zeros((self.num_robot, _abi.ACTUATOR_EP_DIM), dtype=t.float32, device=self.device),
                    t.zeros((self.ep_log.shape[0], _abi.ACTUATOR_EP_DIM), dtype=t.float32, device=self.device))
            _lib.check(self.L.orr_bind_actuator_outputs(self.h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()), self.L)
            self.actuator_out, self.episode_actuator, self.actuator_log = bufs
        else:
            t.cuda.synchronize(self.device)      # launches in flight still write the buffers
            _lib.check(self.L.orr_bind_actuator_outputs(self.h, None, None, None), self.L)
            self.actuator_out = self.episode_actuator = self.actuator_log = None
        self.launch_params_generation += 1

    def _actuator_rows(self):
        if self.actuator_out is None:
            raise ValueError("no actuator outputs: the env was built without actuator_outputs=True")
        return self.actuator_out

    def motor_torque_mean(self):
        """float32 [N, 12]: each motor's mean torque over the last step's sub-steps, N m.  Needs actuator_outputs=True."""
        return self._actuator_rows()[:, :, 0] / self.cfg.action_repeat

    def motor_torque_peak(self):
        """float32 [N, 12]: each motor's largest |torque| of any one sub-step of the last step, N m.  Needs actuator_outputs=True."""
        return self._actuator_rows()[:, :, 1]

    def motor_torque_rms(self):
        """float32 [N, 12]: each motor's root mean square torque over the last step's sub-steps, N m.  Needs actuator_outputs=True."""
        return (self._actuator_rows()[:, :, 2] / self.cfg.action_repeat).sqrt()

    def motor_work(self):
        """float32 [N, 12]: each motor's mechanical work over the last step, J (sim_dt x sum of torque x joint rate after the
        sub-step).  Needs actuator_outputs=True."""
        return self._actuator_rows()[:, :, 3]

    def torque_saturated(self):
        """bool [N, 12]: the motor's peak torque of the last step equalled its limit.  Needs actuator_outputs=True."""
        lim = np.stack([self.torque_limits[self.robot_names[i % len(self.robot_names)]] for i in range(self.num_robot)])
        return self._actuator_rows()[:, :, 1] == self.torch.from_numpy(lim).to(self.device)

    # ---- hot path ------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, mask=None):
        """WrapperEnv.reset (wrapper_env.py:87-107).  mask: optional bool/uint8 tensor [N]; rows of robots
        that are not reset keep their previous observation."""
        mp = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
            mp = mask.data_ptr()
        else:
            self._env_step_counter = 0
        _lib.check(self.L.orr_reset(self.h, mp, self.obs.data_ptr(), self._stream()), self.L)
        return self.obs

    def step(self, actions):
        """WrapperEnv.step (wrapper_env.py:58-85).  actions: float32 [N,12] on the env device (policy
        outputs, clipped to +-2 pi by the caller as in imitation_runners.py:140-143)."""
        t = self.torch
        if actions.dtype != t.float32 or actions.device != self.obs.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(actions.shape) != (self.num_robot, _abi.NUM_MOTORS):
            raise ValueError("actions must have shape (%d, %d)" % (self.num_robot, _abi.NUM_MOTORS))
        _lib.check(self.L.orr_step(self.h, actions.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                                   self.done.data_ptr(), self._stream()), self.L)
        self._env_step_counter += 1
        return self.obs, self.reward, self.done, {}

    def step_into(self, actions, obs_out, reward_out, done_out):
        """step() writing its three outputs into the caller's tensors (rows of a rollout buffer) instead of env.obs / env.reward /
        env.done: contiguous float32 [N,160] (16-byte aligned), float32 [N], uint8 [N] on the env device.  Nothing here depends on
        host state that changes from call to call, so a sequence of these calls can be captured into a hipGraph and replayed - with ONE
        restriction: the launch takes the handle's configuration (the seed included) by value, so a graph captured before env.seed(new)
        replays the old seed; `launch_params_generation` counts such changes and rollout.GraphRollout re-captures when it moves."""
        t = self.torch
        n = self.num_robot
        for x, shape, dt in ((actions, (n, _abi.NUM_MOTORS), t.float32), (obs_out, (n, _abi.OBS_DIM), t.float32), (reward_out, (n,), t.float32),
                             (done_out, (n,), t.uint8)):
            if x.dtype != dt or x.device != self.obs.device or not x.is_contiguous() or tuple(x.shape) != shape:
                raise ValueError("step_into: expected a contiguous %s tensor of shape %s on %s" % (dt, shape, self.device))
        _lib.check(self.L.orr_step(self.h, actions.data_ptr(), obs_out.data_ptr(), reward_out.data_ptr(), done_out.data_ptr(), self._stream()), self.L)
        self._env_step_counter += 1

    def privileged_obs(self, out=None, done=None):
        """The privileged observation (orr_privileged_obs): float32 [N, PRIV_DIM], a robot's row = PRIV_FIELDS, built from its state record
        as it stands now (the state the current observation belongs to) and from the contact / push outputs while they are bound.
        done: the uint8 [N] flags of the step just taken - a robot that ended its episode gets zeros in the contact and push words, which
        still describe that episode; None (after a reset) zeroes them for everybody.  out: a contiguous float32 [N, PRIV_DIM] tensor on
        the env device (a row of a rollout buffer; 16-byte aligned), allocated when None.  One launch that reads the env and changes
        nothing; it can be captured into a hipGraph under step_into's conditions (run it once eagerly first: the first launch loads
        the code object), and a replay reads the buffers that are bound when it runs."""
        t = self.torch
        n = self.num_robot
        if out is None:
            out = t.empty((n, PRIV_DIM), dtype=t.float32, device=self.device)
        for x, shape, dt in ((out, (n, PRIV_DIM), t.float32),) + (((done, (n,), t.uint8),) if done is not None else ()):
            if x.dtype != dt or x.device != self.obs.device or not x.is_contiguous() or tuple(x.shape) != shape:
                raise ValueError("privileged_obs: expected a contiguous %s tensor of shape %s on %s" % (dt, shape, self.device))
        _lib.check(self.L.orr_privileged_obs(self.h, None if done is None else done.data_ptr(), out.data_ptr(), self._stream()), self.L)
        return out

    def time_steps(self, actions, num_steps):
        """Bench helper: num_steps back-to-back launches timed with hipEvents on the launch stream (ms)."""
        ms = C.c_float()
        _lib.check(self.L.orr_time_steps(self.h, actions.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                                         self.done.data_ptr(), self._stream(), int(num_steps), C.byref(ms)), self.L)
        self._env_step_counter += int(num_steps)
        return float(ms.value)

    def stress_actions(self, obs, noise, out):
        """Bench helper: the policy-free stress actions of SURVEY.md section 8d (i) for any mix of robot types, one launch:
        out[i] = clip((first target frame's joints of obs[i], joint -> motor space of robot i) - INIT_MOTOR_ANGLES + noise[i], +-2 pi)."""
        t = self.torch
        for x, cols in ((obs, _abi.OBS_DIM), (noise, _abi.NUM_MOTORS), (out, _abi.NUM_MOTORS)):
            if x.dtype != t.float32 or x.device != self.obs.device or not x.is_contiguous() or tuple(x.shape) != (self.num_robot, cols):
                raise ValueError("stress_actions: contiguous float32 [%d, %d] on the env device expected" % (self.num_robot, cols))
        _lib.check(self.L.orr_stress_actions(self.h, obs.data_ptr(), noise.data_ptr(), out.data_ptr(), self._stream()), self.L)
        return out

    def replay_reset(self, uniforms):
        """Parity entry: reset of all robots with the given draws ([N,28] in [0,1)) instead of the Philox stream."""
        _lib.check(self.L.orr_debug_replay_reset(self.h, uniforms.data_ptr(), self.obs.data_ptr(), self._stream()), self.L)
        self._env_step_counter = 0
        return self.obs

    def replay_step(self, actions, traj, eff, fall, tau_out):
        """Parity entry: one env step with the physics sub-steps replaced by recorded states (include/openroborl_hip.h)."""
        _lib.check(self.L.orr_debug_replay_step(self.h, actions.data_ptr(), traj.data_ptr(), eff.data_ptr(), fall.data_ptr(), self.obs.data_ptr(),
                                                self.reward.data_ptr(), self.done.data_ptr(), tau_out.data_ptr(), self._stream()), self.L)
        self._env_step_counter += 1
        return self.obs, self.reward, self.done

    def debug_physics(self, torques, nsub):
        fall = self.torch.zeros(self.num_robot, dtype=self.torch.uint8, device=self.device)
        _lib.check(self.L.orr_debug_physics(self.h, torques.data_ptr(), fall.data_ptr(), int(nsub), self._stream()), self.L)
        return fall

    # ---- state access (checkpoint / parity injection) -------------------------------------------
    def field(self, name):
        """View of a float field of the state tensor: [N, size]."""
        return self.state[:, self.layout.sl(name)]

    def field_int(self, name):
        return self.state.view(self.torch.int32)[:, self.layout.sl(name)]

    def state_dict(self):
        return {"state": self.state.clone(), "counters": self.counters.clone(), "env_step_counter": self._env_step_counter}

    def load_state_dict(self, d):
        self.state.copy_(d["state"])
        self.counters.copy_(d["counters"])
        self._env_step_counter = int(d["env_step_counter"])

    def stats(self):
        """Diagnostic counters (metrics): totals + histogram of the last done reasons.  Syncs."""
        c = self.counters.cpu().numpy()
        reasons = self.field_int("DONE_REASON")[:, 0].cpu().numpy()
        names = (("contact_fall", _abi.DONE_CONTACT_FALL), ("root_pos", _abi.DONE_ROOT_POS), ("root_rot", _abi.DONE_ROOT_ROT),
                 ("time_limit", _abi.DONE_TIME_LIMIT), ("non_finite", _abi.DONE_NAN), ("motion_over", _abi.DONE_MOTION_OVER))
        return {"total_timesteps": int(c[_abi.CNT_TOTAL_TIMESTEPS]), "curriculum_counter": int(c[_abi.CNT_TOTAL_STEP_COUNT]),
                "episodes_logged": int(c[_abi.CNT_EPISODES]), "episodes_dropped": int(c[_abi.CNT_EPLOG_DROPPED]),
                "last_done_reason": {k: int(((reasons & bit) != 0).sum()) for k, bit in names},
                "max_episode_steps": int(self.field_int("MAX_EP_STEPS").max().item())}

    def active_clip_ids(self):
        """The clip each robot is playing (its CLIP_ID word): int32 [N] on the device."""
        return self.field_int("CLIP_ID")[:, 0].clone()

    def episode_returns_by_clip(self):
        """{clip id: (mean return, episodes)} of the episodes logged since the log was last cleared, without clearing it (syncs).
        Needs a clip set of more than one clip (see episode_log)."""
        if self.clip_log is None:
            raise ValueError("no clip log: no robot type of this env has a clip set of more than one clip")
        k = int(self.torch.clamp(self.counters[_abi.CNT_EPISODES], max=self.ep_log.shape[0]).item())
        ret = self.ep_log[:k, 0].double().cpu().numpy()
        cid = self.clip_log[:k].cpu().numpy()
        return {int(c): (float(ret[cid == c].mean()), int((cid == c).sum())) for c in np.unique(cid)}

    def episode_reward_terms(self):
        """{term name: mean of the term per step} over the episodes logged since the log was last cleared (sum of the episodes' term
        sums / sum of their lengths), without clearing it (syncs); {} when no episode is logged.  Read it before a gather clears the
        log, like episode_returns_by_clip.  Needs reward_terms=True."""
        if self.term_log is None:
            raise ValueError("no term log: the env was built without reward_terms=True")
        k = int(self.torch.clamp(self.counters[_abi.CNT_EPISODES], max=self.ep_log.shape[0]).item())
        if k == 0:
            return {}
        steps = float(self.ep_log[:k, 1].double().sum().item())
        sums = self.term_log[:k].double().sum(0).cpu().numpy()
        return {name: float(sums[i] / steps) for i, name in enumerate(self.TERM_NAMES)}

    def episode_gait(self):
        """{"duty": [4], "normal_force": [4]} per leg over the episodes logged since the log was last cleared, without clearing it
        (syncs): duty = stance steps / steps, normal_force = the mean normal force in N (sum of the normal impulse sums / (steps x
        action_repeat x sim_dt)); {} when no episode is logged.  Read it before a gather clears the log.  Needs contact_outputs=True."""
        if self.contact_log is None:
            raise ValueError("no contact log: the env was built without contact_outputs=True")
        k = int(self.torch.clamp(self.counters[_abi.CNT_EPISODES], max=self.ep_log.shape[0]).item())
        if k == 0:
            return {}
        steps = float(self.ep_log[:k, 1].double().sum().item())
        sums = self.contact_log[:k].double().sum(0).cpu().numpy().reshape(4, 2)
        return {"duty": [float(x / steps) for x in sums[:, 0]],
                "normal_force": [float(x / (steps * self.cfg.action_repeat * self.cfg.sim_dt)) for x in sums[:, 1]]}

    def episode_actuator_stats(self):
        """{"work_per_step": J, "torque_rms": N m, "torque_peak": N m, "saturated_share": share of env steps} over the episodes logged
        since the log was last cleared, without clearing it (syncs): the work of all twelve motors per env step, the root mean square
        torque over motors and sub-steps, the largest |torque| and the share of env steps in which some motor's peak equalled its limit;
        {} when no episode is logged.  Read it before a gather clears the log.  Needs actuator_outputs=True."""
        if self.actuator_log is None:
            raise ValueError("no actuator log: the env was built without actuator_outputs=True")
        k = int(self.torch.clamp(self.counters[_abi.CNT_EPISODES], max=self.ep_log.shape[0]).item())
        if k == 0:
            return {}
        steps = float(self.ep_log[:k, 1].double().sum().item())
        rows = self.actuator_log[:k].double().cpu().numpy()
        return {"work_per_step": float(rows[:, 0].sum() / steps),
                "torque_rms": float(np.sqrt(rows[:, 1].sum() / (steps * self.cfg.action_repeat * _abi.NUM_MOTORS))),
                "torque_peak": float(rows[:, 2].max()), "saturated_share": float(rows[:, 3].sum() / steps)}

    def episode_log_device(self):
        """(log[K,2] snapshot, count, dropped) of the episodes finished since the last call, all on the device and
        without a host sync (count / dropped are 0-d int64 tensors; rows >= count are stale); clears the log."""
        t = self.torch
        log = self.ep_log.clone()
        cnt = self.counters[_abi.CNT_EPISODES].clone()
        dropped = self.counters[_abi.CNT_EPLOG_DROPPED].clone()
        self.counters[_abi.CNT_EPISODES:_abi.CNT_EPLOG_DROPPED + 1] = 0
        return log, t.clamp(cnt, max=log.shape[0]), dropped

    def episode_stats_packed(self, total_timesteps, capacity):
        """The rank's payload of the rollout-boundary all-gather (dist.py layout, float64 [6 + 2 capacity]) in one launch; clears the log."""
        out = self.torch.empty(6 + 2 * int(capacity), dtype=self.torch.float64, device=self.device)
        _lib.check(self.L.orr_episode_stats(self.h, float(total_timesteps), int(capacity), out.data_ptr(), self._stream()), self.L)
        return out

    def episode_log(self, with_dropped=False, with_clip=False, with_terms=False, with_contacts=False):
        """(returns[K], lengths[K]) of the episodes finished since the last call (+ clip_ids[K] int32, the clip each of them played,
        when with_clip; + term_sums[K, 5], each episode's sums of the five reward terms, when with_terms; + contacts[K, 8], each
        episode's [leg][stance steps, normal impulse sum], when with_contacts; + the number of episodes that did not fit the device
        log when with_dropped); clears the log.  Syncs.
        with_clip needs a clip set of more than one clip (the clip log exists only then), with_terms reward_terms=True, with_contacts
        contact_outputs=True: ValueError otherwise."""
        if with_clip and self.clip_log is None:
            raise ValueError("no clip log: no robot type of this env has a clip set of more than one clip")
        if with_terms and self.term_log is None:
            raise ValueError("no term log: the env was built without reward_terms=True")
        clip_log = self.clip_log.clone() if with_clip else None
        if with_contacts and self.contact_log is None:
            raise ValueError("no contact log: the env was built without contact_outputs=True")
        term_log = self.term_log.clone() if with_terms else None
        contact_log = self.contact_log.clone() if with_contacts else None
        log, cnt, dropped = self.episode_log_device()
        k = int(cnt.item())
        out = (log[:k, 0], log[:k, 1]) + ((clip_log[:k],) if with_clip else ()) + ((term_log[:k],) if with_terms else ())
        if with_contacts:
            out += (contact_log[:k],)
        if with_dropped:
            return out + (int(dropped.item()),)
        return out


class LegacyListEnv(object):
    """The reference's list-of-numpy env protocol on top of a VecQuadrupedEnv built with auto_reset=False.

    reset() -> list[N] of float64 arrays (160,)
    step(list[N] of arrays (12,)) -> (obs list, reward list[float], done list[bool], info list[dict])
    (wrapper_env.py:58-107).  As in the reference, the caller resets the WHOLE env when any (train,
    imitation_runners.py:185-205) or all (test, run.py:169) robots are done, `info[i]["terminated"]` aliases
    the done list, the time limit uses the env-global step counter, and the caller's action arrays get
    INIT_MOTOR_ANGLES added in place (minitaur.py:281).
    """

    def __init__(self, env, mutate_actions=True, torque_limits=None, actuator_outputs=False, observation_noise_stdev=None, push=None, push_outputs=False):
        if env.cfg.flags & _abi.FLAG_AUTO_RESET:
            raise ValueError("LegacyListEnv needs a VecQuadrupedEnv created with auto_reset=False")
        if not isinstance(actuator_outputs, (bool, np.bool_)):
            raise ValueError("actuator_outputs must be True or False, got %r" % (actuator_outputs,))
        if torque_limits is not None:        # MotorModel's torque_limits / the actuator outputs, passed through to the env
            env.set_torque_limits(torque_limits)
        if actuator_outputs:
            env.bind_actuator_outputs(True)
        if observation_noise_stdev is not None:     # Minitaur._observation_noise_stdev, passed through to the env
            env.set_sensor_noise(observation_noise_stdev)
        if not isinstance(push_outputs, (bool, np.bool_)):
            raise ValueError("push_outputs must be True or False, got %r" % (push_outputs,))
        if push is not None:                         # external pushes and their outputs, passed through to the env
            env.set_push(push)
        if push_outputs:
            env.bind_push_outputs(True)
        self._env = env
        self._mutate = mutate_actions
        self.num_robot = env.num_robot
        self.observation_space = env.observation_space
        self.action_space = env.action_space
        self._init_angles = [np.asarray(env.models[t]["init_motor_angles"], dtype=np.float64) for t in env.robot_type]
        # host <-> device staging in pinned memory: one asynchronous upload (actions), one asynchronous download (obs | reward | done)
        # and ONE synchronisation per step, instead of four blocking pageable copies
        t = env.torch
        n = env.num_robot
        self._act_host = t.empty((n, _abi.NUM_MOTORS), dtype=t.float32).pin_memory()
        self._act_dev = t.empty((n, _abi.NUM_MOTORS), dtype=t.float32, device=env.device)
        self._out_host = t.empty(env._out.shape, dtype=t.uint8).pin_memory()
        nb_obs, nb_rew = n * _abi.OBS_DIM * 4, n * 4
        out_np = self._out_host.numpy()
        self._obs_np = out_np[:nb_obs].view(np.float32).reshape(n, _abi.OBS_DIM)
        self._rew_np = out_np[nb_obs:nb_obs + nb_rew].view(np.float32)
        self._done_np = out_np[nb_obs + nb_rew:]

    def _fetch(self):
        """obs | reward | done of the last reset / step -> pinned host buffer (one copy, one sync)."""
        t = self._env.torch
        self._out_host.copy_(self._env._out, non_blocking=True)
        t.cuda.current_stream(self._env.device).synchronize()

    def __getattr__(self, attr):           # wrapper_env.py:55-56
        return getattr(self._env, attr)

    def reset(self):
        self._env.reset()
        self._fetch()
        return list(self._obs_np.astype(np.float64))

    def step(self, action):
        t = self._env.torch
        try:
            a = np.asarray(action, dtype=np.float32)              # list of equal-length arrays: one conversion
        except (ValueError, TypeError):
            a = np.stack([np.asarray(action[i], dtype=np.float32) for i in range(self.num_robot)])
        if a.shape != (self.num_robot, _abi.NUM_MOTORS):
            a = np.stack([np.asarray(action[i], dtype=np.float32).reshape(_abi.NUM_MOTORS) for i in range(self.num_robot)])
        self._act_host.numpy()[...] = a
        self._act_dev.copy_(self._act_host, non_blocking=True)
        self._env.step(self._act_dev)
        if self._mutate:                   # minitaur.py:281 adds INIT_MOTOR_ANGLES to the caller's arrays in place (done while the GPU works)
            init = self._init_angles
            for i in range(self.num_robot):
                ai = action[i]
                if isinstance(ai, np.ndarray):
                    ai += init[i]
        self._fetch()
        obs = self._obs_np.astype(np.float64)
        rew_list = self._rew_np.astype(np.float64).tolist()
        done_np = self._done_np.astype(bool)
        ndone = int(done_np.sum())
        if ndone > 0:
            # wrapper_env.py:82-83: the curriculum counter advances by num_robot per step in which ANY robot finished
            # (the kernel already added one per finished robot)
            self._env.counters[_abi.CNT_TOTAL_STEP_COUNT] += self.num_robot - ndone
        done_list = done_np.tolist()
        info = [{"terminated": done_list} for _ in range(self.num_robot)]
        return list(obs), rew_list, done_list, info


def build_env(task_name, num_robot=None, mode=None, enable_randomizer=None, legacy=False, **kw):
    """Counterpart of run.py:49-97 build_env for the two imitation tasks."""
    if task_name not in cfgmod.TASKS:
        raise ValueError("unknown task %r" % (task_name,))
    env = VecQuadrupedEnv(task_name=task_name, num_robot=num_robot, mode=mode, enable_randomizer=enable_randomizer,
                          auto_reset=not legacy, **kw)
    return LegacyListEnv(env) if legacy else env
