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
kernels behind the C-ABI (include/openroborl_hip.h).  The validators that turn the arguments into the C-ABI's
structs are in env_spec.py, the float64 predictors of the device's draw rules (for tests and golden makers) in
env_draws.py; both are imported here by name, so `openroborl_amd.env.<name>` keeps resolving.
"""
import ctypes as C
import math

import numpy as np

from . import _abi, _lib, config as cfgmod, env_draws, env_spec, motion, robots, state as statemod
from .env_draws import (CLIP_CHANGE_DRAW, CLIP_DRAW, NOISE_HEADING_BLOCK, NOISE_RESET_BLOCK, PRIV_DIM, PRIV_FIELDS, RAND_LEG_WORD,  # noqa: F401
                        RAND_ROW_WORDS, SENSOR_NOISE_BLOCK, SENSOR_SLOT_FILTER, SENSOR_SLOT_HIST, SENSOR_SLOT_TARGET, clip_change_time,
                        clip_draw_index, clip_switch_draws, init_perturb_draw_indices, init_perturb_draws, normal_pair, push_block, push_kick,
                        randomizer_apply, randomizer_draw_indices, randomizer_row, sensor_noise_block, sensor_noise_normals, tar_noise_block)
from .env_spec import (INIT_PERTURB_STD, PUSH_KEYS, RAND_NOOP_NAMES, RAND_POSITIVE_NAMES, RAND_REFUSED_NAMES, clip_switch_spec,  # noqa: F401
                       motion_spec, push_on, push_spec, randomizer_latency_max, randomizer_spec, sensor_noise_on, sensor_noise_spec,
                       task_noise_spec, torque_limit_spec)


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


def action_space():
    """minitaur.py:145-148."""
    return Box(np.array([-2 * math.pi] * 12), np.array([2 * math.pi] * 12), dtype=np.float32)


def _check_flags(**flags):
    """The on / off arguments of the two env classes, in the order given."""
    for name, v in flags.items():
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("%s must be True or False, got %r" % (name, v))


class VecQuadrupedEnv(object):
    """N independent quadrupeds on one GPU; four robots per wavefront, 16 lanes each (see csrc/orr_env_kernels.h, orr_physics.h)."""

    TERM_NAMES = _abi.REWARD_TERM_NAMES      # the columns of reward_terms / episode_term_sums / the term log, in orr_config::reward_w's order

    def __init__(self, task_name=None, training_yaml=None, sim_yaml=None, device="cuda", num_robot=None, seed=None,
                 robot=None, motion_file=None, mode=None, enable_randomizer=None, auto_reset=True, num_procs=1,
                 robot_index_offset=0, legacy_grid=False, mixed_robots=None, ep_log_capacity=65536, config_overrides=None,
                 model_overrides=None, clip_time_min=None, clip_time_max=None, perturb_init_state_prob=None, tar_obs_noise=None,
                 init_perturb_std=None, reward_terms=False, contact_outputs=False, torque_limits=None, actuator_outputs=False,
                 observation_noise_stdev=None, randomizer_config=None, randomizer_params=False, push=None, push_outputs=False,
                 clip_weights=None, clip_curriculum=None, reward_shaping=None):
        import torch
        _check_flags(push_outputs=push_outputs, randomizer_params=randomizer_params, reward_terms=reward_terms,
                     contact_outputs=contact_outputs, actuator_outputs=actuator_outputs)
        env_spec.reward_shaping_spec(reward_shaping)     # the values here, ahead of everything that needs the device
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
        # weighted clip draws (orr_set_clip_weights; the task YAML may carry clip_weights) and the failure-adaptive clip curriculum
        # (orr_set_clip_curriculum): uniform draws and no curriculum by default.  Validated here, ahead of anything that needs the device
        if clip_weights is None:
            clip_weights = params.get("clip_weights")
        self.clip_weights = env_spec.clip_weights_spec(clip_weights, self.clip_sets)
        self.clip_curriculum = env_spec.clip_curriculum_spec(clip_curriculum, self.clip_sets, default_ref=float(self.cfg.ep_len_end))
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
        # the clip curriculum's stats of the last clip_curriculum_update ([MAX_CLIPS, 4] float64 on the device): None until it is set
        self.clip_stats = None
        if any(w is not None for w in self.clip_weights.values()):
            self.set_clip_weights(clip_weights)
        if self.clip_curriculum is not None:
            self.set_clip_curriculum(clip_curriculum)
        # what the pushes did to each robot (orr_bind_push_outputs): None while unbound
        self.push_out = None
        if push_on(self.push):
            self.set_push(push)
        if push_outputs:
            self.bind_push_outputs(True)
        # reward shaping (orr_set_reward_shaping; this project's own, the reference has none): None = off, and step() / step_into() issue the
        # one call they always issued.  The per-step rows, their sums over each robot's current episode and over its finished episodes,
        # and the imitation reward that orr_step writes while shaping is on: all None while off
        self.reward_shaping = None
        self.shaping_out = self.episode_shaping = self.shaping_totals = self.imitation_reward = self._shaping_prev = None
        if reward_shaping is not None:
            self.set_reward_shaping(reward_shaping)

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

    def _zeros(self, *shapes):
        t = self.torch
        return tuple(t.zeros(s, dtype=t.float32, device=self.device) for s in shapes)

    def _bind_outputs(self, bind, attrs, bufs):
        """The one rule of the output binds: hand the C-ABI entry `bind` the device pointers of the tensors `bufs` (None = unbind: NULL
        for each), then keep the tensors (or None) in the attributes `attrs`.  Synchronises first: launches in flight still write the
        buffers that an unbind or a new bind lets go.  A bound buffer selects the kernel variant, so launch_params_generation moves."""
        self.torch.cuda.synchronize(self.device)
        bufs = bufs if bufs is not None else (None,) * len(attrs)
        _lib.check(bind(self.h, *[None if b is None else b.data_ptr() for b in bufs]), self.L)
        for a, b in zip(attrs, bufs):
            setattr(self, a, b)
        self.launch_params_generation += 1

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

    def set_clip_weights(self, clip_weights=None):
        """Change the weights of the clip draws of a running env (orr_set_clip_weights; see env_spec.clip_weights_spec: None = uniform, a
        list of one weight per clip of the set, or a dict by robot name): every reset and every mid-episode switch from the next launch on
        draws entry k with probability w_k / sum w (to 2^-24).  The kernels read the thresholds in device memory: no kernel variant
        changes, launch_params_generation does not move and captured graphs stay valid."""
        spec = env_spec.clip_weights_spec(clip_weights, self.clip_sets)
        for name, w in spec.items():
            arr = None if w is None else (C.c_float * len(w))(*[float(x) for x in w])
            _lib.check(self.L.orr_set_clip_weights(self.h, robots.ROBOT_TYPE_ID[name], arr, len(self.clip_sets[name])), self.L)
        self.clip_weights = spec

    def clip_thresholds(self):
        """{robot name: int64 [n + 1]}: the 24-bit thresholds each type's clip draws go by, as the DEVICE holds them (set_clip_weights or
        the last clip_curriculum_update wrote them); env_draws.clip_draw_weighted predicts the draws from them.  Syncs."""
        out = {}
        for name, ids in self.clip_sets.items():
            buf, n = (C.c_uint32 * (_abi.MAX_CLIPS + 1))(), C.c_int32()
            _lib.check(self.L.orr_get_clip_thresholds(self.h, robots.ROBOT_TYPE_ID[name], buf, C.byref(n)), self.L)
            out[name] = np.array(buf[:n.value + 1], dtype=np.int64)
        return out

    def clip_probabilities(self):
        """{robot name: float64 [n]}: the probability of each entry of the type's clip set under clip_thresholds().  Syncs."""
        return {name: np.diff(cum) / float(1 << 24) for name, cum in self.clip_thresholds().items()}

    def set_clip_curriculum(self, clip_curriculum):
        """Give the failure-adaptive clip curriculum its settings (orr_set_clip_curriculum; see env_spec.clip_curriculum_spec) and zero
        its running scores; clip_curriculum_update then moves the thresholds.  Like set_clip_weights it changes no kernel variant."""
        spec = env_spec.clip_curriculum_spec(clip_curriculum, self.clip_sets, default_ref=float(self.cfg.ep_len_end))
        if spec is None:
            raise ValueError("set_clip_curriculum needs settings; to stop adapting, stop calling clip_curriculum_update (set_clip_weights(None) restores uniform draws)")
        _lib.check(self.L.orr_set_clip_curriculum(self.h, C.byref(spec)), self.L)
        self.clip_curriculum = spec
        if self.clip_stats is None:
            self.clip_stats = self.torch.zeros((_abi.MAX_CLIPS, _abi.CLIP_STATS_COLS), dtype=self.torch.float64, device=self.device)

    def clip_curriculum_update(self):
        """One launch (orr_clip_curriculum_update), no host sync: the episode log and the clip log as they stand -> per-clip scores, the
        running scores and new thresholds for every clip set of more than one clip.  It clears nothing: call it once between two clears
        of the log (episode_log*, dist.gather_env_episodes).  Returns env.clip_stats, float64 [MAX_CLIPS, 4] on the device, a clip id's
        row = (episodes, integer score sum, mean score, running score); the next call overwrites it.  Capturable into a hipGraph
        (run it once eagerly first: the first launch loads the code object).  Needs a clip set of more than one clip (the clip log) and
        set_clip_curriculum: RuntimeError otherwise."""
        _lib.check(self.L.orr_clip_curriculum_update(self.h, None if self.clip_stats is None else self.clip_stats.data_ptr(), self._stream()), self.L)
        return self.clip_stats

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
        rows = self.randomizer_rows if on else None
        if on and rows is None:
            rows, = self._zeros((self.num_robot, _abi.RAND_ROW))
            rows[:, :31] = 0.5          # mid-range until a reset writes them (suspended from the start: every parameter at its centre)
            rows[:, RAND_LEG_WORD] = 0.0
        suspend = bool(on and suspend)
        self._bind_outputs(lambda h, p: self.L.orr_bind_randomizer_params(h, p, int(suspend)), ("randomizer_rows",), (rows,) if on else None)
        self.randomizer_suspended = suspend

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
        bufs = None
        if on:       # the buffer is kept across binds
            bufs = (self.push_out,) if self.push_out is not None else self._zeros((self.num_robot, _abi.PUSH_ROW))
        self._bind_outputs(self.L.orr_bind_push_outputs, ("push_out",), bufs)

    def set_reward_shaping(self, spec=None, scale=1.0):
        """Switch the shaped reward on, change its weights, or switch it off (orr_set_reward_shaping; see env_spec.reward_shaping_spec for
        `spec` and `scale`; None = off).  While on, step() and step_into() hand orr_step env.imitation_reward [N] as its reward buffer
        and follow it with ONE more launch, orr_shaped_reward, which writes the caller's reward tensor = max(imitation reward - sum of the
        weighted penalties, floor) and env.shaping_out [N, 8] (a robot's row = the six unweighted terms in _abi.SHAPING_NAMES' order, the
        shaped reward, 1.0), env.episode_shaping [N, 8] (their sums over its current episode) and env.shaping_totals [N, 8] (the sums
        of its finished episodes; column 7 = their steps).  EP_RETURN, the episode log and the clip curriculum stay on the imitation
        reward.  Switching on allocates and binds those buffers and - where a non-zero weight needs them and they are unbound - the
        actuator / contact outputs.  Switching on or off changes the launch sequence: holders of captured graphs re-capture
        (launch_params_generation); step once eagerly before a capture, as for every kernel's first launch.  A change of the weights
        while on is read by the kernel in device memory, in stream order: launch_params_generation does not move and a captured graph
        follows it - unless the new weights need outputs that are not bound yet, which binds them and moves it."""
        struct = env_spec.reward_shaping_spec(spec, scale)
        was_on, on = self.reward_shaping is not None, spec is not None
        if on:
            need_act, need_contact = env_spec.reward_shaping_needs(struct)
            if need_act and self.actuator_out is None:
                self.bind_actuator_outputs(True)
            if need_contact and self.contact_out is None:
                self.bind_contact_outputs(True)
        if on and not was_on:
            n = self.num_robot
            bufs = self._zeros((n, _abi.SHAPING_ROW), (n, _abi.SHAPING_ROW), (n, _abi.SHAPING_ROW), (n, _abi.SHAPING_PREV))
            self.imitation_reward, = self._zeros((n,))
            self._bind_outputs(self.L.orr_bind_reward_shaping, ("shaping_out", "episode_shaping", "shaping_totals", "_shaping_prev"), bufs)
        _lib.check(self.L.orr_set_reward_shaping(self.h, C.byref(struct) if on else None, self._stream()), self.L)
        if was_on and not on:
            self._bind_outputs(self.L.orr_bind_reward_shaping, ("shaping_out", "episode_shaping", "shaping_totals", "_shaping_prev"), None)
            self.imitation_reward = None
        self.reward_shaping = struct if on else None

    def reward_shaping_stats(self):
        """{name: mean per step} of the six unweighted terms and `shaped_reward` over the episodes finished since the totals were last
        cleared (sum over robots of shaping_totals[:, k] / sum over robots of shaping_totals[:, 7], in float64); {} when no episode
        has finished or shaping is off.  Syncs."""
        if self.shaping_totals is None:
            return {}
        tot = self.shaping_totals.double().sum(0).cpu().numpy()
        if not tot[_abi.SHAPING_ROW - 1] > 0.0:
            return {}
        return {name: float(tot[k] / tot[_abi.SHAPING_ROW - 1]) for k, name in enumerate(_abi.SHAPING_COLUMNS[:-1])}

    def clear_shaping_totals(self):
        """Zero env.shaping_totals (a device fill in stream order, no sync): reward_shaping_stats then covers the episodes that finish from
        here on."""
        if self.shaping_totals is not None:
            self.shaping_totals.zero_()

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
        n = _abi.NUM_REWARD_TERMS
        self._bind_outputs(self.L.orr_bind_reward_terms, ("reward_terms", "episode_term_sums", "term_log"),
                           self._zeros((self.num_robot, n), (self.num_robot, n), (self.ep_log.shape[0], n)) if on else None)

    def bind_contact_outputs(self, on=True):
        """Bind (allocating on first use) or unbind the foot contact outputs (orr_bind_contact_outputs): env.contact_out [N, 16] (row =
        [leg][normal sum, friction x sum, friction y sum, largest normal], N s; valid after step / debug_physics), env.episode_contact
        [N, 8] (row = [leg][stance steps, normal sum] of the robot's current episode) and env.contact_log [ep_log_capacity, 8]; all None
        while unbound.  It selects the kernel variant: holders of captured graphs re-capture (launch_params_generation); the variant's
        first launch in a process loads its code object, so step once eagerly before a capture (GraphRollout's first segment does)."""
        shapes = ((self.num_robot, _abi.CONTACT_OUT_DIM), (self.num_robot, _abi.CONTACT_EP_DIM), (self.ep_log.shape[0], _abi.CONTACT_EP_DIM))
        self._bind_outputs(self.L.orr_bind_contact_outputs, ("contact_out", "episode_contact", "contact_log"), self._zeros(*shapes) if on else None)

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
        shapes = ((self.num_robot, _abi.NUM_MOTORS, _abi.ACTUATOR_OUT_DIM), (self.num_robot, _abi.ACTUATOR_EP_DIM), (self.ep_log.shape[0], _abi.ACTUATOR_EP_DIM))
        self._bind_outputs(self.L.orr_bind_actuator_outputs, ("actuator_out", "episode_actuator", "actuator_log"), self._zeros(*shapes) if on else None)

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
        if self.reward_shaping is not None:
            self._step_shaped(actions, self.obs, self.reward, self.done)
        else:
            _lib.check(self.L.orr_step(self.h, actions.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                                       self.done.data_ptr(), self._stream()), self.L)
        self._env_step_counter += 1
        return self.obs, self.reward, self.done, {}

    def _step_shaped(self, actions, obs_out, reward_out, done_out):
        """The two launches of a step while reward shaping is on: orr_step with env.imitation_reward as its reward buffer, then
        orr_shaped_reward from it into reward_out."""
        stream = self._stream()
        _lib.check(self.L.orr_step(self.h, actions.data_ptr(), obs_out.data_ptr(), self.imitation_reward.data_ptr(), done_out.data_ptr(), stream), self.L)
        _lib.check(self.L.orr_shaped_reward(self.h, actions.data_ptr(), self.imitation_reward.data_ptr(), done_out.data_ptr(), reward_out.data_ptr(),
                                            stream), self.L)

    def _check_tensors(self, who, *args):
        """Each of args = (tensor, shape, dtype): a contiguous tensor of exactly that on the env device, or ValueError in who's name."""
        for x, shape, dt in args:
            if x.dtype != dt or x.device != self.obs.device or not x.is_contiguous() or tuple(x.shape) != shape:
                raise ValueError("%s: expected a contiguous %s tensor of shape %s on %s" % (who, dt, shape, self.device))

    def step_into(self, actions, obs_out, reward_out, done_out):
        """step() writing its three outputs into the caller's tensors (rows of a rollout buffer) instead of env.obs / env.reward /
        env.done: contiguous float32 [N,160] (16-byte aligned), float32 [N], uint8 [N] on the env device.  Nothing here depends on
        host state that changes from call to call, so a sequence of these calls can be captured into a hipGraph and replayed - with ONE
        restriction: the launch takes the handle's configuration (the seed included) by value, so a graph captured before env.seed(new)
        replays the old seed; `launch_params_generation` counts such changes and rollout.GraphRollout re-captures when it moves."""
        t = self.torch
        n = self.num_robot
        self._check_tensors("step_into", (actions, (n, _abi.NUM_MOTORS), t.float32), (obs_out, (n, _abi.OBS_DIM), t.float32),
                            (reward_out, (n,), t.float32), (done_out, (n,), t.uint8))
        if self.reward_shaping is not None:
            self._step_shaped(actions, obs_out, reward_out, done_out)
        else:
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
        self._check_tensors("privileged_obs", (out, (n, PRIV_DIM), t.float32), *(((done, (n,), t.uint8),) if done is not None else ()))
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

    def _logged(self):
        """(k, steps) of the episode log as it stands (syncs): the episodes logged since it was last cleared and the sum of their lengths."""
        k = int(self.torch.clamp(self.counters[_abi.CNT_EPISODES], max=self.ep_log.shape[0]).item())
        return k, float(self.ep_log[:k, 1].double().sum().item())

    def episode_returns_by_clip(self):
        """{clip id: (mean return, episodes)} of the episodes logged since the log was last cleared, without clearing it (syncs).
        Needs a clip set of more than one clip (see episode_log)."""
        if self.clip_log is None:
            raise ValueError("no clip log: no robot type of this env has a clip set of more than one clip")
        k, _ = self._logged()
        ret = self.ep_log[:k, 0].double().cpu().numpy()
        cid = self.clip_log[:k].cpu().numpy()
        return {int(c): (float(ret[cid == c].mean()), int((cid == c).sum())) for c in np.unique(cid)}

    def episode_reward_terms(self):
        """{term name: mean of the term per step} over the episodes logged since the log was last cleared (sum of the episodes' term
        sums / sum of their lengths), without clearing it (syncs); {} when no episode is logged.  Read it before a gather clears the
        log, like episode_returns_by_clip.  Needs reward_terms=True."""
        if self.term_log is None:
            raise ValueError("no term log: the env was built without reward_terms=True")
        k, steps = self._logged()
        if k == 0:
            return {}
        sums = self.term_log[:k].double().sum(0).cpu().numpy()
        return {name: float(sums[i] / steps) for i, name in enumerate(self.TERM_NAMES)}

    def episode_gait(self):
        """{"duty": [4], "normal_force": [4]} per leg over the episodes logged since the log was last cleared, without clearing it
        (syncs): duty = stance steps / steps, normal_force = the mean normal force in N (sum of the normal impulse sums / (steps x
        action_repeat x sim_dt)); {} when no episode is logged.  Read it before a gather clears the log.  Needs contact_outputs=True."""
        if self.contact_log is None:
            raise ValueError("no contact log: the env was built without contact_outputs=True")
        k, steps = self._logged()
        if k == 0:
            return {}
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
        k, steps = self._logged()
        if k == 0:
            return {}
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

    def __init__(self, env, mutate_actions=True, torque_limits=None, actuator_outputs=False, observation_noise_stdev=None, push=None, push_outputs=False,
                 clip_weights=None, clip_curriculum=None, reward_shaping=None):
        if env.cfg.flags & _abi.FLAG_AUTO_RESET:
            raise ValueError("LegacyListEnv needs a VecQuadrupedEnv created with auto_reset=False")
        _check_flags(actuator_outputs=actuator_outputs)
        if torque_limits is not None:       # MotorModel's torque_limits / the actuator outputs, passed through to the env
            env.set_torque_limits(torque_limits)
        if actuator_outputs:
            env.bind_actuator_outputs(True)
        if observation_noise_stdev is not None:     # Minitaur._observation_noise_stdev, passed through to the env
            env.set_sensor_noise(observation_noise_stdev)
        _check_flags(push_outputs=push_outputs)      # where it always was: after the settings above have reached the env
        if push is not None:                        # external pushes and their outputs, passed through to the env
            env.set_push(push)
        if push_outputs:
            env.bind_push_outputs(True)
        if clip_weights is not None:                # weighted clip draws and the clip curriculum, passed through to the env
            env.set_clip_weights(clip_weights)
        if clip_curriculum is not None:
            env.set_clip_curriculum(clip_curriculum)
        if reward_shaping is not None:              # reward shaping, passed through to the env
            env.set_reward_shaping(reward_shaping)
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
