"""Configuration: the reference's two YAML files -> orr_config.

  training_param.yaml    task sections `imitation_learning_laikago` / `imitation_learning_minicheetah`
                         (keys read at OpenRoboRL/run.py:194-215)
  pybullet_sim_param.yaml section `quadruped_robot` (quadruped_gym_env.py:159-178)

Hyper-parameters the reference hard-codes in run.py:54-64 (episode-length curriculum 20 -> 600 over
3e7 steps, tar_frame_steps [1, 2, 10, 30], ref_state_init_prob 0.9, warmup 0.25 s) and in
imitation_task.py:45-55 (reward weights / scales) are defaults here.
"""
import math
import os

import yaml

from . import _abi

_PKG_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config")
DEFAULT_TRAINING_YAML = os.path.join(_PKG_CFG, "training_param.yaml")
DEFAULT_SIM_YAML = os.path.join(_PKG_CFG, "pybullet_sim_param.yaml")

TASKS = ("imitation_learning_laikago", "imitation_learning_minicheetah")
ACTION_REPEAT = 33          # laikago.py:26, mini_cheetah.py:26 NUM_ACTION_REPEAT
CTRL_LATENCY = 0.002        # laikago.py:27


# Solver constants.  PYBULLET_REMEMBERED = what PyBullet is REMEMBERED to set in place of the Bullet library's defaults
# (PhysicsServerCommandProcessor::createEmptyDynamicsWorld: m_erp2 = 0.08, m_warmstartingFactor = 0.1, m_frictionERP = 0.2; the contact
# breaking threshold is 0.02 x the shape's bounding radius, btCollisionShape::getContactBreakingThreshold, i.e. ~0.5 mm for a toe sphere and a few mm
# for a link: one 4 mm margin stands for both here).  A recollection of Bullet's public source, not verifiable in this environment.
# Rounds 1-5 shipped BULLET_LIBRARY_DEFAULTS.  Round 6 ADOPTED the remembered set as make_config's defaults by a cross-robot rule fixed
# before the run (tools/identify_r6.py P5; profiles/r06_constants_rule.json): preferred on each robot's policies (Laikago mean J 0.565 vs
# 0.560, minicheetah_trot J 0.648 vs 0.611 and F 0.947 vs 0.893) and costing the OTHER robot's policies nothing (no policy loses 0.02 in F or
# J).  The library set stays available: VecQuadrupedEnv(config_overrides=config.BULLET_LIBRARY_DEFAULTS).
BULLET_LIBRARY_DEFAULTS = {"contact_erp": 0.2, "warmstart_factor": 0.85, "friction_erp": 0.2, "contact_margin": 0.02}
PYBULLET_REMEMBERED = {"contact_erp": 0.08, "warmstart_factor": 0.1, "friction_erp": 0.2, "contact_margin": 0.004}


# The reference's randomiser configuration "all_params" (minitaur_env_randomizer_config.py:22-36), name -> [lower, upper]: what
# ORR_FLAG_RANDOMIZER alone applies.  A task section of the training YAML may carry a dictionary of this form (or the name "all_params")
# under the key `env_randomizer_config`; env_spec.randomizer_spec lists the accepted names
RANDOMIZER_ALL_PARAMS = {"mass": [0.8, 1.2], "inertia": [0.5, 1.5], "motor strength": [0.8, 1.2], "motor friction": [0, 0.05],
                         "latency": [0.0, 0.04], "lateral friction": [0.5, 1.25], "battery": [14.0, 16.8], "joint friction": [0, 0.05]}


# External pushes (orr_set_push): a task section of the training YAML may carry the env's `push` dictionary under the key `push`, e.g.
# push: {interval_s: 5.0, lin_vel: [0.2, 0.6], lin_vel_z: 0.2, ang_vel: 0.5, grace_steps: 10}; env_spec.push_spec lists the accepted keys
PUSH_KEY = "push"


def load_training_params(task_name, path=None):
    """run.py:194-200: section lookup by --task; ValueError when missing."""
    path = path or DEFAULT_TRAINING_YAML
    with open(path) as f:
        d = yaml.safe_load(f)
    if task_name not in d:
        raise ValueError("Hyperparameters not found for %s in %s" % (task_name, path))
    return d[task_name]


def load_sim_params(path=None):
    """quadruped_gym_env.py:159-165."""
    path = path or DEFAULT_SIM_YAML
    with open(path) as f:
        d = yaml.safe_load(f)
    if "quadruped_robot" not in d:
        raise ValueError("Hyperparameters not found for pybullet_sim_config.yaml")
    return d["quadruped_robot"]


def make_config(num_robots, sim_params=None, mode="train", enable_randomizer=None, seed=0, num_procs=1,
                auto_reset=True, legacy_grid=False, curriculum=None):
    sim = dict(sim_time_step_s=0.001, num_sim_iter_step=300)
    sim.update(sim_params or {})
    c = _abi.OrrConfig()
    c.abi_version = _abi.ABI_VERSION
    c.num_robots = int(num_robots)
    c.action_repeat = ACTION_REPEAT
    c.solver_iters = int(sim["num_sim_iter_step"] / ACTION_REPEAT)   # quadruped_gym_env.py:177-178
    if c.action_repeat < 1 or c.solver_iters < 1:
        raise ValueError("num_sim_iter_step / action_repeat must be >= 1")
    c.sim_dt = float(sim["sim_time_step_s"])
    c.gravity_z = -10.0                                               # quadruped_gym_env.py:200
    c.reward_w[:] = [0.5, 0.05, 0.2, 0.15, 0.1]                       # imitation_task.py:45-49
    c.reward_scale[:] = [5.0, 0.1, 40.0, 3.0, 20.0, 2.0]              # imitation_task.py:50-55
    c.tar_frame_steps[:] = [1, 2, 10, 30]                             # run.py:62
    c.ref_state_init_prob = 0.9                                       # run.py:63
    c.warmup_time = 0.25                                              # run.py:64
    c.ep_len_end = 600                                                # run.py:55
    c.ep_len_start = 600 if mode == "test" else 20                    # run.py:54,66-67
    c.curriculum_steps = int(math.ceil(30000000 / float(num_procs)))  # run.py:75; wrapper_env.py:45-46
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if enable_randomizer is None:
        enable_randomizer = mode == "train"                           # run.py:205-206
    if curriculum is None:
        curriculum = True                                             # wrapper_env.py:147-149 (steps > 0)
    c.flags = ((_abi.FLAG_AUTO_RESET if auto_reset else 0) | (_abi.FLAG_RANDOMIZER if enable_randomizer else 0) |
               _abi.FLAG_CYCLE_SYNC | (_abi.FLAG_LEGACY_GRID if legacy_grid else 0) |
               (_abi.FLAG_CURRICULUM if curriculum else 0))
    c.contact_erp = PYBULLET_REMEMBERED["contact_erp"]
    c.contact_margin = PYBULLET_REMEMBERED["contact_margin"]
    c.warmstart_factor = PYBULLET_REMEMBERED["warmstart_factor"]
    c.max_coord_velocity = 100.0
    c.plane_friction = 1.0
    c.limit_activation = 0.1
    c.max_angle_change = 0.2                                          # laikago.py:71
    c.dist_fail_threshold = 1.0                                       # imitation_task.py:518
    c.rot_fail_threshold = 0.5 * math.pi
    c.friction_erp = PYBULLET_REMEMBERED["friction_erp"]
    return c
