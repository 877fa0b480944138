"""The device's draw rules, predicted on the host in float64: which draws of an episode's Philox stream (seed, robot index, episode)
a reset or a step reads, and what it makes of them.  Tests and golden makers compare the kernels against these; the env itself needs
only the row layouts (RAND_ROW_WORDS, RAND_LEG_WORD, PRIV_FIELDS).  numpy and the ABI's constants only: nothing here touches the device.
The arguments' validators are in env_spec.py, the env classes in env.py."""
import math

import numpy as np

from . import _abi

CLIP_DRAW = 28      # index of the clip draw in a reset's Philox stream (block 7, word 0; draws 0..27: randomiser, ref-state-init, time offset)


def clip_draw_index(m, n):
    """The entry of an n-clip set a reset picks (csrc/orr_task.h, reset_robot_state<true>): (m * n) >> 24, m = the 24-bit integer of draw
    CLIP_DRAW (the draw in [0, 1) is m / 2^24).  Integer arithmetic; works on numpy integer arrays."""
    return (np.asarray(m, dtype=np.int64) * int(n)) >> 24


def clip_thresholds_uniform(n):
    """The thresholds orr_set_clip_set writes for an n-entry set: cum[k] = ceil(k 2^24 / n) in integer arithmetic, k = 0..n (int64 [n +
    1]).  They pick clip_draw_index(m, n) for every m."""
    n = int(n)
    if not 1 <= n <= _abi.MAX_CLIPS:
        raise ValueError("a clip set holds 1 .. %d clips" % _abi.MAX_CLIPS)
    return np.array([((k << 24) + n - 1) // n for k in range(n + 1)], dtype=np.int64)


def clip_thresholds(weights):
    """The thresholds orr_set_clip_weights writes (None: the uniform ones cannot be told without the set's size, so weights are
    required): cum[k] = ceil(2^24 W_k / W) in float64, W_k the running sum of the float32 weights in entry order, W their total.
    int64 [n + 1]; a zero weight gives an empty interval, equal weights the uniform thresholds."""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(-1)
    if not 1 <= len(w) <= _abi.MAX_CLIPS:
        raise ValueError("a clip set holds 1 .. %d clips" % _abi.MAX_CLIPS)
    if not (np.isfinite(w).all() and (w >= 0.0).all()):
        raise ValueError("clip weights must be finite numbers >= 0")
    run, total = 0.0, 0.0
    for x in w:
        total += float(x)
    if not total > 0.0:
        raise ValueError("all clip weights are zero")
    cum = [0]
    for x in w:
        run += float(x)
        cum.append(int(math.ceil(16777216.0 * run / total)))
    return np.array(cum, dtype=np.int64)


def clip_draw_weighted(m, thresholds):
    """The entry a draw's 24-bit integer m picks under the thresholds cum[0..n]: the k with cum[k] <= m < cum[k + 1] (csrc/orr_task.h,
    clip_drawn).  Works on numpy integer arrays."""
    cum = np.asarray(thresholds, dtype=np.int64)
    return np.searchsorted(cum[1:], np.asarray(m, dtype=np.int64), side="right")


def clip_episode_score(x, ref):
    """An episode's 16-bit score (orr_clip_curriculum_update): floor(65536 clamp(x / ref, 0, 1) + 0.5) with the float32 metric x and the
    float32 ref widened to float64; a NaN quotient scores 0.  int64; works on arrays."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    ref = np.asarray(ref, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.fmin(np.fmax(x / ref, 0.0), 1.0)
    return np.floor(65536.0 * r + 0.5).astype(np.int64)


def clip_curriculum_step(ema, n, S, sets, alpha, eps):
    """One orr_clip_curriculum_update in float64 from the per-clip-id counts n[c] and integer score sums S[c]: ema_c <- (1 - alpha) ema_c +
    alpha S_c / (65536 n_c) where n_c > 0; then for every set of more than one entry (sets: {type: list of clip ids}) f_k = 1 -
    ema[c_k], F = their sum in entry order, uniform thresholds if F < 1e-12, else p_k = (1 - eps) f_k / F + eps / len and
    clip_thresholds' rule on p.  alpha and eps as the device holds them (float32).  -> (ema' float64 [MAX_CLIPS], {type: int64
    thresholds}); sets of one entry are left out."""
    alpha, eps = float(np.float32(alpha)), float(np.float32(eps))
    ema = np.array(ema, dtype=np.float64).reshape(_abi.MAX_CLIPS).copy()
    for c in range(_abi.MAX_CLIPS):
        if int(n[c]) > 0:
            ema[c] = (1.0 - alpha) * ema[c] + alpha * (float(int(S[c])) / (65536.0 * float(int(n[c]))))
    out = {}
    for t, ids in sets.items():
        k = len(ids)
        if k < 2:
            continue
        f = [1.0 - ema[c] for c in ids]
        F = 0.0
        for x in f:
            F += x
        if F < 1e-12:
            out[t] = clip_thresholds_uniform(k)
            continue
        p = [(1.0 - eps) * x / F + eps / float(k) for x in f]
        run, total = 0.0, 0.0
        for x in p:
            total += x
        cum = [0]
        for x in p:
            run += x
            cum.append(int(math.ceil(16777216.0 * run / total)))
        out[t] = np.array(cum, dtype=np.int64)
    return ema, out


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


# ---- task noise (orr_set_task_noise; ImitationTask's perturb_init_state_prob and tar_obs_noise) ------------------------------------
NOISE_RESET_BLOCK = 0x20000000      # Philox blocks 0x20000000 .. 0x20000008 of the episode's stream: the 36 uniforms U(k) of a reset's perturbation
NOISE_HEADING_BLOCK = 0x30000000    # block 0x30000000 + i: the heading noise of target observation i of the episode (tar_noise_block)
# _apply_state_perturb's standard deviations (imitation_task.py:1201-1206), by the names of orr_task_noise's fields: the defaults of
# init_perturb_draws here and of env_spec.task_noise_spec
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


# ---- domain randomisation (orr_set_randomizer, orr_bind_randomizer_params; ControllableEnvRandomizerFromConfig) ----------------------
# row words of the params buffer (include/openroborl_hip.h, orr_bind_randomizer_params) by parameter
RAND_ROW_WORDS = {"inertia": slice(0, 2), "joint friction": slice(2, 10), "latency": slice(10, 11), "lateral friction": slice(11, 12),
                  "mass": slice(12, 14), "motor strength": slice(14, 26), "base mass": slice(26, 27), "global motor strength": slice(27, 28),
                  "leg weaken": slice(28, 30), "single leg weaken": slice(30, 31)}
RAND_LEG_WORD = 28                                       # the weakened leg, as a float 0..3: not a draw in [0, 1)


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
