"""What the GPU tests share: the robots' default clips, the env builders with the tests' usual keyword arguments, stress actions,
float64 copies of the device's records, crafted single-robot records (robot_state), and the canonical forms of the episode log that
the optional outputs' tests compare.
torch and the env are imported inside the functions that need them: CPU test helpers import this module for its constants."""
import os

import numpy as np

from openroborl_amd import state as statemod
from tests import oracle_lib as ol
from tests import phys_ref as pr

MIXED = ("laikago", "mini_cheetah")
CLIP = {"laikago": "laikago_pace", "mini_cheetah": "minicheetah_trot"}
EPS = 2.0 ** -24
SOFT_TOES = {"contact_stiffness": 30000.0, "contact_damping": 1000.0, "foot_friction": 3.0}
HIP, THIGH, KNEE = 0, 1, 2      # the parts of a leg: joint 3 * leg + part


def make_env(n, files="laikago_pace", **kw):
    from openroborl_amd.env import VecQuadrupedEnv
    kw.setdefault("robot", "laikago")
    kw.setdefault("mode", "test")
    kw.setdefault("enable_randomizer", False)
    kw.setdefault("auto_reset", True)
    kw.setdefault("seed", 5)
    return VecQuadrupedEnv(num_robot=n, motion_file=files, **kw)


def mixed_env(n, **kw):
    """Laikago and mini-cheetah interleaved, each on its clip"""
    from openroborl_amd.env import VecQuadrupedEnv
    kw.setdefault("seed", 3)
    kw.setdefault("mode", "train")
    kw.setdefault("enable_randomizer", True)
    return VecQuadrupedEnv(num_robot=n, mixed_robots=list(MIXED), motion_file=[CLIP[m] for m in MIXED], **kw)


def short_episodes():
    """ep_len_start = 8, ep_len_end = 24 with the curriculum as the task fixtures set it"""
    g = np.load(os.path.join(ol.GOLDEN, "task_laikago.npz"))
    return dict(ep_len_start=8, ep_len_end=24, curriculum_steps=int(g["curriculum_steps"]))


def stress(env, obs, rng):
    import torch
    noise = torch.from_numpy(rng.normal(0.0, 0.05, (env.num_robot, 12)).astype(np.float32)).to(env.device)
    return env.stress_actions(obs, noise, torch.empty_like(noise))


def gpu_state64(env):
    return statemod.to_float64(env.layout, env.state.detach().cpu().numpy())


def push_state(env, st64):
    import torch
    env.state.copy_(torch.from_numpy(statemod.from_float64(env.layout, st64)).to(env.device))


def leg_clearance(m, pos, quat, q):
    """height of the lowest contact sphere (toe or shank) of each leg above the plane"""
    bodies, _ = pr.kinematics(m, pos, quat, q)
    out = []
    for leg in range(4):
        b = bodies[1 + 3 * leg + 2]
        h = (b["o"] + b["R"] @ m["toe_pos"][leg])[2] - m["toe_radius"]
        if m["shank_radius"] > 0:
            h = min(h, (b["o"] + b["R"] @ m["shank_pos"][leg])[2] - m["shank_radius"])
        out.append(h)
    return np.array(out)


def robot_state(env, base_row, rng, lifted=(), height=0.0, limits=(), qd=None, fold=-0.3):
    """One record: the robot standing level in its initial pose, every toe 1 mm inside the plane; the legs in `lifted` folded at the knee
    until their toe is clear of the contact margin; `height` added to the base; limits = ((leg, part, side, gap, rate), ...): that joint
    `gap` away from its lower (side 0) / upper (side 1) bound, moving towards it at `rate`.  Small random velocities otherwise
    (qd: the twelve joint rates instead; fold: what folding a lifted leg adds to its knee angle - the mini-cheetah's knees bend the
    other way).  -> (record, down [4] bool, limited [12] bool) as the device will see them."""
    lay, m, cfg = env.layout, env.models[int(np.asarray(env.robot_type).flat[0])], env.cfg      # one robot type in the batch
    dirj, offj, _ = pr.joint_maps(m)
    ang = np.zeros(12)                                                  # kinematic angle a = dirj (q - offj) = the motor's angle
    for mot in range(12):
        ang[int(m["joint_of_motor"][mot])] = m["init_motor_angles"][mot]
    rate = rng.uniform(-0.5, 0.5, 12) if qd is None else np.array(qd, dtype=float)
    stand = leg_clearance(m, np.zeros(3), m["init_quat"], ang * dirj + offj)
    assert np.ptp(stand) < 1e-4, stand                                   # the initial pose stands level
    for leg in lifted:
        ang[3 * leg + KNEE] += fold                                      # folds the leg (Laikago: the bound is at -2.775, the pose at -1.25)
    for leg, part, side, gap, speed in limits:
        j = 3 * leg + part
        ang[j] = (m["joint_hi"][j] - gap) if side else (m["joint_lo"][j] + gap)
        rate[j] = speed if side else -speed
    q = ang * dirj + offj
    pos = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -stand.min() - 0.001 + height])
    st = base_row.copy()
    st[lay.sl("POS")] = pos
    st[lay.sl("QUAT")] = m["init_quat"]
    st[lay.sl("Q")] = q
    st[lay.sl("QD")] = rate * dirj
    st[lay.sl("LINVEL")] = rng.uniform(-0.1, 0.1, 3)
    st[lay.sl("ANGVEL")] = rng.uniform(-0.2, 0.2, 3)
    st[lay.sl("LAMBDA")] = 0.0
    st[lay.sl("KNEE_FRICTION")] = rng.uniform(0.0, 0.05, 4)
    st[lay.sl("FOOT_MU")] = rng.uniform(0.5, 1.25)
    clear = leg_clearance(m, pos, m["init_quat"], q)
    margin = float(cfg.contact_margin)
    assert (np.abs(clear - margin) > 5e-4).all(), clear                  # nobody sits on the threshold
    a = dirj * (q - offj)
    room = np.minimum(a - m["joint_lo"], m["joint_hi"] - a) - float(cfg.limit_activation)
    assert (np.abs(room) > 0.02).all(), room
    return st, clear < margin, room < 0.0


def canonical_log(env, k, side_log):
    """The first k rows of the episode log with their rows of a side log (term_log, contact_log), in an order that does not depend on
    which wave's slot request arrived first (the slots of one launch go by arrival)"""
    rows = np.concatenate([env.ep_log[:k].cpu().numpy(), side_log[:k].cpu().numpy()], axis=1)
    return rows[np.lexsort(rows.T[::-1])].tobytes()


def log_rows_match(ep_log, side_log, want, logged=None):
    """The log's (return, length, side row) triples (host arrays, the rows in use) are the host's per-episode ones, `want`, as a
    multiset; with a full log, `logged` of them."""
    want = sorted((np.float32(r).tobytes(), l, row.astype(np.float32).tobytes()) for r, l, row in want)
    got = sorted((ep_log[j, 0].tobytes(), int(ep_log[j, 1]), side_log[j].tobytes()) for j in range(len(ep_log)))
    if logged is None:
        assert got == want
    else:
        assert all(g in want for g in got) and len(got) == logged
