"""The env's argument validators: user arguments -> the C-ABI's structs (include/openroborl_hip.h), with a ValueError on anything the
C-ABI would refuse, so that a wrong argument fails before anything needs the device.  The float64 predictors of the device's draw
rules are in env_draws.py, the env classes in env.py."""
import math

import numpy as np

from . import _abi, config as cfgmod
from .env_draws import INIT_PERTURB_STD


def _number(v, wording, *shown):
    """float(v) of a real number that is no bool; ValueError(wording % shown) otherwise."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(wording % shown)
    return float(v)


def _for_robot(v, name, robot_names, what):
    """The entry for robot `name` of an argument that is one value for every robot or, for mixed batches, a dict by robot name
    (None for a robot the dict leaves out).  ValueError when the dict names a robot that is not in the batch."""
    if not isinstance(v, dict):
        return v
    unknown = set(v) - set(robot_names)
    if unknown:
        raise ValueError("%s names robots that are not in this batch: %s" % (what, sorted(unknown)))
    return v.get(name)


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


def clip_switch_spec(clip_time_min, clip_time_max, robot_names):
    """clip_time_min / clip_time_max (ImitationTask's kwargs: a float, or a dict by robot name for mixed batches; None = +inf) ->
    {robot name: (tmin, tmax)}.  (+inf, +inf) = no switching (the reference's default); otherwise both finite, 0 <= tmin <= tmax.
    ValueError on anything the C-ABI (orr_set_clip_switch) would refuse."""
    def bound(v, name, what):
        v = _for_robot(v, name, robot_names, what)
        return math.inf if v is None else _number(v, "%s must be a number or a dict by robot name, not %r", what, v)
    out = {}
    for name in robot_names:
        lo, hi = bound(clip_time_min, name, "clip_time_min"), bound(clip_time_max, name, "clip_time_max")
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


def clip_weights_spec(clip_weights, clip_sets):
    """clip_weights (None = uniform; a list of one weight per entry of the clip set; or a dict by robot name of either, for mixed
    batches) -> {robot name: None or float32 [n]} for the robots of clip_sets ({robot name: clip ids}, motion_spec's).  ValueError on
    anything the C-ABI (orr_set_clip_weights) would refuse: a wrong length, a negative, NaN or infinite weight, all weights zero."""
    def one(v, name):
        if v is None:
            return None
        if isinstance(v, (bool, np.bool_, str, dict)) or np.ndim(v) != 1:
            raise ValueError("clip_weights of %s must be None or a list of one weight per clip, not %r" % (name, v))
        for x in v:
            _number(x, "clip_weights of %s must be numbers, not %r", name, v)
        a = np.asarray(v, dtype=np.float32)
        if len(a) != len(clip_sets[name]):
            raise ValueError("clip_weights of %s: %d weights for a clip set of %d clips" % (name, len(a), len(clip_sets[name])))
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError("clip_weights of %s must be finite numbers >= 0, got %r" % (name, v))
        if not float(a.astype(np.float64).sum()) > 0.0:
            raise ValueError("clip_weights of %s: all weights are zero" % name)
        return a
    names = sorted(clip_sets)
    return {name: one(_for_robot(clip_weights, name, names, "clip_weights"), name) for name in names}


def clip_curriculum_spec(clip_curriculum, clip_sets, default_ref=None):
    """clip_curriculum -> the orr_clip_curriculum struct, or None for None.  A list (alpha, eps) or (alpha, eps, metric), or a dict with
    `alpha` (weight of an update's mean score in the running score, in (0, 1]), `eps` (share of the uniform distribution, in [0, 1]),
    `metric` ("length", the default, "return" or "step_reward") and `ref`: the metric's value that counts as mastered - a number for
    every clip, a list by clip id, or a dict by robot name of a number or a list by entry of that robot's clip set, for mixed batches.
    default_ref: the episode length that stands for ref when none is given (the env passes the task's final episode step limit) -
    "length" and "return" (one reward unit per step) take it, "step_reward" takes 1.  ValueError on anything the C-ABI (orr_set_clip_curriculum) would refuse."""
    if clip_curriculum is None:
        return None
    if isinstance(clip_curriculum, dict):
        unknown = set(clip_curriculum) - {"alpha", "eps", "metric", "ref"}
        if unknown:
            raise ValueError("clip_curriculum: unknown keys %s (known: alpha, eps, metric, ref)" % sorted(unknown))
        if "alpha" not in clip_curriculum or "eps" not in clip_curriculum:
            raise ValueError("clip_curriculum needs alpha and eps")
        cur = dict(clip_curriculum)
    elif isinstance(clip_curriculum, (list, tuple)) and len(clip_curriculum) in (2, 3):
        cur = dict(zip(("alpha", "eps", "metric"), clip_curriculum))
    else:
        raise ValueError("clip_curriculum must be None, (alpha, eps[, metric]) or a dict with alpha, eps, metric, ref, not %r" % (clip_curriculum,))
    alpha = _number(cur["alpha"], "clip_curriculum: alpha must be a number, not %r", cur["alpha"])
    eps = _number(cur["eps"], "clip_curriculum: eps must be a number, not %r", cur["eps"])
    if not (0.0 < alpha <= 1.0):
        raise ValueError("clip_curriculum: alpha must lie in (0, 1], not %r" % (alpha,))
    if not (0.0 <= eps <= 1.0):
        raise ValueError("clip_curriculum: eps must lie in [0, 1], not %r" % (eps,))
    metric = cur.get("metric", "length")
    if metric not in _abi.CLIP_METRICS:
        raise ValueError("clip_curriculum: unknown metric %r (known: %s)" % (metric, ", ".join(_abi.CLIP_METRICS)))
    ref = cur.get("ref")
    if ref is None:
        if metric != "step_reward" and default_ref is None:
            raise ValueError("clip_curriculum: the metric %r needs a ref (the value that counts as mastered)" % (metric,))
        ref = 1.0 if metric == "step_reward" else default_ref
    names = sorted(clip_sets)
    spec = _abi.OrrClipCurriculum(alpha=alpha, eps=eps, metric=_abi.CLIP_METRICS.index(metric))
    for c in range(_abi.MAX_CLIPS):
        spec.ref[c] = 1.0                 # clip ids outside every set: never read for a logged episode of this env
    for name in names:
        ids = clip_sets[name]
        r = _for_robot(ref, name, names, "clip_curriculum: ref")
        if isinstance(ref, dict) and r is None:
            raise ValueError("clip_curriculum: ref names no value for %s" % name)
        if isinstance(r, (bool, np.bool_, str, dict)) or np.ndim(r) > 1:
            raise ValueError("clip_curriculum: ref of %s must be a number or a list, not %r" % (name, r))
        if np.ndim(r) == 0:
            vals = {c: r for c in ids}
        elif isinstance(ref, dict):
            if len(r) != len(ids):
                raise ValueError("clip_curriculum: ref of %s: %d values for a clip set of %d clips" % (name, len(r), len(ids)))
            vals = dict(zip(ids, r))
        else:
            if len(r) <= max(ids):
                raise ValueError("clip_curriculum: ref lists %d values; clip id %d of %s needs one" % (len(r), max(ids), name))
            vals = {c: r[c] for c in ids}
        for c, v in vals.items():
            v = _number(v, "clip_curriculum: ref must hold numbers, not %r", v)
            if not (0.0 < float(np.float32(v)) < math.inf):      # NaN fails the comparison
                raise ValueError("clip_curriculum: ref of clip %d must be finite and > 0, not %r" % (c, v))
            spec.ref[c] = v
    return spec


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
    return {name: one(_for_robot(torque_limits, name, robot_names, "torque_limits"), name) for name in robot_names}


# ---- task noise (orr_set_task_noise; ImitationTask's perturb_init_state_prob and tar_obs_noise) ------------------------------------
def task_noise_spec(perturb_init_state_prob=0.0, tar_obs_noise=None, init_perturb_std=None):
    """ImitationTask's perturb_init_state_prob / tar_obs_noise (a float, or a list whose first entry is used: the reference reads only
    [0]; None = off) and an optional dict overriding some of INIT_PERTURB_STD -> the orr_task_noise struct.  ValueError on anything
    the C-ABI (orr_set_task_noise) would refuse."""
    def number(v, what):
        return _number(v, "%s must be a number, not %r", what, v)
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
        vals[name] = _number(v, "%s must be a number, not %r", name, v)
        if not (0.0 <= vals[name] < math.inf):       # NaN fails the comparison
            raise ValueError("%s must be a finite standard deviation >= 0, not %r" % (name, v))
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
            _number(v, "randomizer parameter %r: the bounds must be numbers, not %r", name, rng)
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
        x = _number(v, "push: %s must be a number, not %r", name, v)
        if not math.isfinite(x):
            raise ValueError("push: %s must be a finite number, not %r" % (name, v))
        if x < 0.0:
            raise ValueError("push: %s must be >= 0, not %r" % (name, v))
        return x

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


# ---- reward shaping (orr_set_reward_shaping, orr_bind_reward_shaping, orr_shaped_reward) ---------------------------------------------
SHAPING_KEYS = _abi.SHAPING_NAMES + ("floor",)


def reward_shaping_spec(spec=None, scale=1.0):
    """The shaping setting -> the orr_reward_shaping struct.  spec: None (all weights 0, no floor) or a dict with the weights `torque`,
    `work`, `action_rate`, `action_accel`, `impact`, `failure` (each >= 0; a missing key is 0) and `floor` (the smallest shaped reward;
    missing = -inf = none).  The weights - not the floor - are multiplied by `scale` (a ramp's factor, >= 0) in float64 and rounded to
    float32 once.  ValueError on an unknown key and on anything the C-ABI (orr_set_reward_shaping) would refuse; the message names the key."""
    out = _abi.OrrRewardShaping()
    out.floor = -math.inf
    scale = _number(scale, "reward_shaping: scale must be a number, not %r", scale)
    if not (0.0 <= scale < math.inf):
        raise ValueError("reward_shaping: scale must be a finite number >= 0, not %r" % (scale,))
    if spec is None:
        return out
    if not isinstance(spec, dict):
        raise ValueError("reward_shaping must be None or a dict with the keys %s, not %r" % (", ".join(SHAPING_KEYS), spec))
    for k in spec:
        if k not in SHAPING_KEYS:
            raise ValueError("unknown reward_shaping key %r (known: %s)" % (k, ", ".join(SHAPING_KEYS)))
    for i, name in enumerate(_abi.SHAPING_NAMES):
        w = _number(spec.get(name, 0.0), "reward_shaping: %s must be a number, not %r", name, spec.get(name)) * scale
        if not 0.0 <= w <= float(np.finfo(np.float32).max):        # NaN fails the comparison; beyond float32's range the C side would see +inf
            raise ValueError("reward_shaping: %s must be a finite weight >= 0, not %r (scale %r)" % (name, spec.get(name), scale))
        out.w[i] = w
    floor = _number(spec.get("floor", -math.inf), "reward_shaping: floor must be a number, not %r", spec.get("floor"))
    if not floor < math.inf:
        raise ValueError("reward_shaping: floor must be a number below +inf (-inf = none), not %r" % (spec.get("floor"),))
    out.floor = floor
    return out


def reward_shaping_needs(spec):
    """(actuator outputs, contact outputs): whether a non-zero weight of the struct needs them bound (torque or work; impact)."""
    i = _abi.SHAPING_NAMES.index
    return (spec.w[i("torque")] != 0.0 or spec.w[i("work")] != 0.0), spec.w[i("impact")] != 0.0
