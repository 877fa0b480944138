"""Every termination reason and every fall proxy on the device, exactly (tests/termination_refs.py holds the float64 reference, the
derived float32 bounds and the case grids; tests/test_termination_refs_cpu.py shows that the comparison used here rejects a float32
mimic with each of twelve seeded defects).

  fall proxies   one physics sub-step (orr_debug_physics, nsub = 1): each of the 16 proxies 1 mm inside the contact threshold with
                 every other one at least 1 mm clear and the same pose 2 mm higher, hit and clear robots mixed within waves and over all
                 four slots; 256 tumbled poses around first touch; and, through a live env step in free flight, WHICH pose the step's
                 flag refers to (the one before the last sub-step integrates).  The debug physics has no two-wave form (the variant
                 rule: tests/test_variant_rule_cpu.py, "never kTwoWave"), so its units here are the default and the contact-outputs one.
  reason bits    the replay step (orr_debug_replay_step) sees exactly the rigid state and the fall flag the test chose: the whole
                 DONE_REASON word of 97 robots, one case each, near cases 16 bounds to 1e-4 from their threshold
                 (and the position cases again with a 0.75 m threshold: thr^2 = thr at the shipped 1 m)
  every unit     one live env step per row of tests/test_gpu_variant_cells.py's ROWS, far cases only, and the same step on an auto-reset
                 twin: the same done, the same DONE_REASON word, LAST_EP_LEN and the episode counter (orr_debug_replay_step refuses a
                 handle with ORR_FLAG_AUTO_RESET, so the twin cannot run the replay grid)

Mini-cheetah's proxies 0, 2, 4, 6 (the chassis's upper corners) are never the lowest proxy of a pose (hips and knees stand proud of
them): they are isolated on a table whose other twelve proxies have fall_radius = -1 m.  Laikago's are all isolated by pose; the same
table is run for Laikago too, because only there proxies 2k and 2k + 1 differ in radius (a radius read from the neighbour lane shows).

Left out, with the reason: the ROOT_ROT bit of the four cases whose injected word is in QUAT (NaN, +-Inf: float64 has no angle to
compare with; 2e30: its square overflows float32, not float64 - there is no margin to build), everything else of their word is compared.
(Measured once on an MI355X: the device wrote float64's word for all four - 16, 16, 16 and, for 2e30, 20.  atan2_bf makes a finite
angle of a NaN by its sign bit, so that is not a property to assert.)
"""
import numpy as np
import pytest

from openroborl_amd import _abi, config
from tests import gpu_kit as kit
from tests import oracle_lib as ol
from tests import termination_refs as tr
from tests.test_gpu_variant_cells import ROWS

pytestmark = pytest.mark.gpu

ROBOTS = ("laikago", "mini_cheetah")
MODEL_ISOLATED = {"laikago": [], "mini_cheetah": [0, 2, 4, 6]}
PHYSICS_UNITS = {"default": {}, "contacts": dict(contact_outputs=True)}
PROXY_F32 = 1e-6            # a 3-term dot product on values below 1 m


def words(lay):
    return slice(lay.sl("POS").start, lay.sl("POS").start + tr.WORDS)


# ---- fall proxies through one sub-step --------------------------------------------------------------------------------------------
def physics_flags(env, base_row, launch):
    import torch
    kit.push_state(env, tr.pose_records(base_row, launch))
    fall = env.debug_physics(torch.zeros((len(launch), 12), dtype=torch.float32, device=env.device), 1).cpu().numpy().astype(int)
    assert np.isfinite(kit.gpu_state64(env)[:, words(env.layout)]).all()
    return fall


def physics_env(robot, n, unit, fall_radius=None):
    over = {robot: {"fall_radius": fall_radius}} if fall_radius is not None else None
    env = kit.make_env(n, kit.CLIP[robot], robot=robot, auto_reset=False, model_overrides=over, **PHYSICS_UNITS[unit])
    env.reset()
    return env, kit.gpu_state64(env)[0]


@pytest.mark.parametrize("unit", list(PHYSICS_UNITS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_one_fall_proxy_at_a_time(robot, unit):
    from tests.stage_refs import model_of
    rng = np.random.RandomState(2)
    shipped = model_of(robot)
    margin = float(ol.dec32(config.PYBULLET_REMEMBERED["contact_margin"]))
    checked, by_pose, by_model = 0, [], []
    for table in ("shipped", "isolating"):
        group = list(MODEL_ISOLATED[robot] or tr.MODEL_GROUP) if table == "isolating" else None
        radius = tr.isolating_model(shipped, group) if group else None
        model = model_of(robot, {"fall_radius": radius} if group else None)
        found, missing = tr.isolated_proxy_cases(model, margin, only=group)
        if group is None:
            assert missing == MODEL_ISOLATED[robot]          # the proxies that needed the table
            by_pose = sorted(found)
        else:
            assert not missing
            by_model = sorted(found)
            np.testing.assert_array_equal(np.asarray(model["fall_radius"])[group], np.asarray(shipped["fall_radius"])[group])     # as shipped
        env, base = physics_env(robot, 2 * len(found) + 3, unit, radius)
        table_of = env.models[int(env.robot_type[0])]
        assert margin == float(ol.dec32(env.cfg.contact_margin)) and int(table_of["num_fall_proxies"]) == 16
        for key in ("fall_body", "fall_pos", "fall_radius"):
            np.testing.assert_array_equal(np.asarray(table_of[key]), np.asarray(model[key]))
        for launch in tr.mixed_launches(found, tr.airborne_case(model, margin, rng)):
            assert len(launch) == env.num_robot
            got = physics_flags(env, base, launch)
            want = np.array([c["flag"] for c in launch])
            wrong = [(i, launch[i]["proxy"], want[i], got[i]) for i in np.nonzero(got != want)[0]]
            assert not wrong, (table, wrong)
            checked += len(launch)
        env.close()
    assert sorted(set(by_pose) | set(MODEL_ISOLATED[robot])) == list(range(16)) and set(MODEL_ISOLATED[robot]) <= set(by_model)
    print("%s: proxies isolated by pose %s, by the table %s" % (robot, by_pose, by_model))
    tr.report("one_proxy_%s_%s" % (robot, unit), checked, tr.DELTA, PROXY_F32, 0)


@pytest.mark.parametrize("unit", list(PHYSICS_UNITS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_the_shipped_proxy_table_on_tumbled_poses(robot, unit):
    env, base = physics_env(robot, 256, unit)
    model, margin = env.models[int(env.robot_type[0])], float(ol.dec32(env.cfg.contact_margin))
    cases, decided = tr.tumbled_cases(model, margin, seed=1)
    got = physics_flags(env, base, cases)
    want = np.array([c["flag"] for c in cases])
    print("%s: %d of 256 poses within 1 mm of the threshold, hit share %.3f" % (robot, (~decided).sum(), want.mean()))
    assert (~decided).mean() <= 0.10 and 0.3 <= want.mean() <= 0.7
    np.testing.assert_array_equal(got[decided], want[decided])
    env.close()
    tr.report("tumbled_%s_%s" % (robot, unit), int(decided.sum()), float(min(np.abs(c["clearance"]).min() for c, d in zip(cases, decided) if d)), PROXY_F32,
              int((~decided).sum()))


def falling_pose(model, margin):
    """Laikago upside down with a chassis corner lowest by 5 mm or more and every contact sphere (toes, shanks) 15 cm or more above it"""
    rng = np.random.RandomState(0)
    quat, q = tr.random_poses(model, rng, 4000)
    c0 = tr.proxy_clearance_batch(model, np.zeros((4000, 3)), quat, q, margin)
    order = np.sort(c0, axis=1)
    for p in np.nonzero((np.argmin(c0, axis=1) < 8) & (order[:, 1] - order[:, 0] > 5e-3))[0]:
        R = kit.pr.quat_to_mat(kit.pr.qmul(quat[p], kit.pr.qconj(np.asarray(model["init_quat"], dtype=float))))
        if R[2, 2] < -0.5 and (kit.leg_clearance(model, [0, 0, -c0[p].min()], quat[p], q[p]) > 0.15).all():
            return tr.f32r(quat[p]), tr.f32r(q[p]), float(c0[p].min())
    raise AssertionError("no pose")


def test_the_steps_fall_flag_is_of_the_pose_before_the_last_substep():
    """Free flight, upside down, descending at 1 - 3 m/s from heights at which the lowest corner crosses the contact threshold well before
    the last sub-step, between the starts of the last two, only while the last one integrates, or not at all.  The oracle judges the
    proxies on the pose before the last sub-step integrates (margins_out[:, 0]); cases it sees within 0.3 mm of the threshold (a tenth
    of a sub-step's travel, far above float32's drift over 33 contact-free sub-steps) are not selected."""
    import ctypes as C
    import torch
    n = 42
    env = kit.make_env(n, "laikago_pace", auto_reset=False)
    orc = ol.OracleEnv(env.cfg, env.models, env.clips, n, robot_type=env.robot_type, clip_id=env.clip_id, threads=8)
    orc.L.orc_set_margins_out.argtypes = [C.c_void_p, ol.dp]
    margins = np.zeros((n, 3))
    orc.L.orc_set_margins_out(orc.h, ol.P(margins))
    env.reset()
    lay, cfg = env.layout, env.cfg
    model, margin = env.models[0], float(ol.dec32(env.cfg.contact_margin))
    quat, q, low = falling_pose(model, margin)
    dt, rep = float(ol.dec32(cfg.sim_dt)), cfg.action_repeat
    rec = kit.gpu_state64(env)
    speed = np.tile([1.0, 2.0, 3.0], n // 3)
    # the corner's clearance at the START of the last sub-step, in sub-steps of travel: the ladder, two early crossings, two that never cross
    ladder = np.concatenate([np.linspace(-1.4, 1.4, n // 3 - 4), [-25.0, -20.0, 6.0, 9.0]])
    target = np.repeat(ladder, 3) * speed * dt
    # the action that asks for the joint angles the robot has: the legs hold still
    jom = np.asarray(model["joint_of_motor"], dtype=int)
    hold = (q[jom] - np.asarray(model["motor_offset"])) * np.asarray(model["motor_dir"]) - np.asarray(model["init_motor_angles"])
    act = np.tile(hold, (n, 1)).astype(np.float32)
    for i in range(n):
        rec[i, lay.sl("POS")] = [0.1 * i, 0.0, -low + 0.15]
        rec[i, lay.sl("QUAT")], rec[i, lay.sl("Q")] = quat, q
        rec[i, lay.sl("LINVEL")] = [0.0, 0.0, -speed[i]]
        rec[i, lay.sl("ANGVEL")], rec[i, lay.sl("QD")], rec[i, lay.sl("LAMBDA")] = 0.0, 0.0, 0.0
    # without a contact the flight does not depend on the height: a first pass of the oracle from 15 cm up measures how far the corner
    # comes down before the last sub-step, the start heights follow from it
    orc.state[:] = rec
    orc.step(act.astype(np.float64))
    assert (orc.field("LAMBDA") == 0.0).all() and (margins[:, 0] > 0.02).all()
    rec[:, lay.sl("POS")][:, 2] -= margins[:, 0] - target
    for i in range(n):
        assert tr.proxy_clearance64(model, rec[i, lay.sl("POS")], quat, q, margin).min() > 5e-3          # starts clear
        assert (kit.leg_clearance(model, rec[i, lay.sl("POS")], quat, q) - (speed[i] * rep * dt + 0.02) > 0.1).all()      # no sphere reaches the plane
    rec = kit.statemod.to_float64(lay, kit.statemod.from_float64(lay, rec))
    kit.push_state(env, rec)
    orc.state[:] = rec
    env.step(torch.from_numpy(act).to(env.device))
    orc.step(act.astype(np.float64))
    assert (orc.field("LAMBDA") == 0.0).all()                                                            # contact-free
    got = (env.field_int("DONE_REASON")[:, 0].cpu().numpy() & tr.CONTACT_FALL) != 0
    want = (orc.field("DONE_REASON")[:, 0].astype(int) & tr.CONTACT_FALL) != 0
    m = margins[:, 0]
    np.testing.assert_array_equal(want, m < 0)
    sel = np.abs(m) >= 3e-4
    step = speed * dt
    before, during = sel & (m < 0) & (m > -step), sel & (m > 0) & (m < step)
    assert before.sum() >= 2 and during.sum() >= 2, (before.sum(), during.sum())
    assert (sel & (m < -10 * step)).sum() >= 2 and (sel & (m > 3 * step)).sum() >= 2                  # well before, and not at all
    end = np.array([tr.proxy_clearance64(model, *(orc.state[i, lay.sl(k)] for k in ("POS", "QUAT", "Q")), margin).min() for i in range(n)])
    assert (end[during] < 0).all() and not want[during].any()       # crossed while the last sub-step integrated: the pose after it touches, the flag is clear
    np.testing.assert_array_equal(got[sel], want[sel])
    tr.report("step_flag_pose", int(sel.sum()), float(np.abs(m[sel]).min()), 3e-4, int((~sel).sum()))
    env.close(); orc.close()


# ---- every reason bit through the replay step ------------------------------------------------------------------------------------
class GpuReplay(object):
    """run_replay_grid's backend on the device"""

    def __init__(self, env, uniforms=None):
        import torch
        self.torch, self.env = torch, env
        if uniforms is not None:
            env.replay_reset(torch.from_numpy(uniforms).to(env.device))
        n = env.num_robot
        self.eff = torch.zeros((n, 2, 8, 3), dtype=torch.float32, device=env.device)
        self.tau = torch.zeros((n, env.cfg.action_repeat, 12), dtype=torch.float32, device=env.device)
        self.act = torch.zeros((n, 12), dtype=torch.float32, device=env.device)

    def records(self):
        return kit.gpu_state64(self.env)

    def set_records(self, rec):
        kit.push_state(self.env, rec)

    def replay_step(self, traj, fall):
        t, env = self.torch, self.env
        tj = t.from_numpy(np.ascontiguousarray(traj, dtype=np.float32)).to(env.device)
        fl = t.from_numpy(np.ascontiguousarray(fall, dtype=np.uint8)).to(env.device)
        _, reward, done = env.replay_step(self.act, tj, self.eff, fl, self.tau)
        t.cuda.synchronize(env.device)
        return done.cpu().numpy().astype(bool), reward.cpu().numpy().astype(np.float64)


REPLAY_UNITS = {
    "default": {},
    "two_wave": {},
    "randomizer": dict(enable_randomizer=True, randomizer_config={"mass": [1.0, 1.0], "inertia": [1.0, 1.0], "motor strength": [1.0, 1.0]},
                       randomizer_params=True),
    "position_0.75": dict(config_overrides={"dist_fail_threshold": tr.OTHER_DIST_THRESHOLD}),
}


def check_grid(env, run, cfg, clip, group):
    """what is asserted for every robot of a replay grid"""
    lay = env.layout
    bits, masks, nearest, left_out = tr.expected_of_grid(run, cfg, clip)
    got = run["after"][:, lay.sl("DONE_REASON")][:, 0].astype(int)
    wrong = [(run["cases"][i]["name"], got[i], bits[i]) for i in range(len(bits)) if (got[i] ^ bits[i]) & masks[i]]
    assert not wrong, wrong
    np.testing.assert_array_equal(run["done"], got != 0)
    np.testing.assert_array_equal(run["after"][:, lay.sl("EP_STEP")][:, 0], run["start"][:, lay.sl("EP_STEP")][:, 0] + 1)
    nan = (bits & tr.NAN) != 0
    assert (run["reward"][nan] == 0.0).all() and np.isfinite(run["reward"][~nan]).all()
    np.testing.assert_array_equal(run["after"][:, lay.sl("REF_POSE")], run["ref_after"])      # the step's own reference pose is the scouted one
    hist = env.stats()["last_done_reason"]
    whole = [c["mask"] == tr.ALL_BITS for c in run["cases"]]
    assert hist == tr.histogram(got) and tr.histogram(got[whole]) == tr.histogram(bits[whole])
    tr.report(group, len(bits), nearest, tr.ang_bound(), left_out)
    return got


@pytest.mark.parametrize("unit", list(REPLAY_UNITS))
def test_every_reason_bit_through_the_replay_step(unit, monkeypatch):
    if unit == "two_wave":
        monkeypatch.setenv("ORR_STEP_WAVES_PER_EU", "2")            # read when the handle is created
    kw = REPLAY_UNITS[unit]
    probe = kit.make_env(1, "laikago_pace", auto_reset=False, **kw)
    cases = tr.replay_cases(probe.cfg, only_pos=unit == "position_0.75")
    probe.close()
    n = len(cases)
    env = kit.make_env(n, "laikago_pace", auto_reset=False, **kw)
    cfg, clip, lay = env.cfg, env.clips[0], env.layout
    assert clip.flags & _abi.CLIP_WRAP and float(cfg.dist_fail_threshold) == (tr.OTHER_DIST_THRESHOLD if unit == "position_0.75" else 1.0)
    backend = GpuReplay(env, tr.replay_uniforms(n))
    reset = backend.records()
    run = tr.run_replay_grid(backend, cases, cfg, clip)
    got = check_grid(env, run, cfg, clip, "replay_" + unit)
    # the same grid without the injected words: the wave-mates of an injected robot carry the same word in both runs, and what an injected
    # robot carries without its injection is what its case says without it
    backend.set_records(reset)
    twin = tr.run_replay_grid(backend, cases, cfg, clip, inject=False)
    got_twin = twin["after"][:, lay.sl("DONE_REASON")][:, 0].astype(int)
    injected = np.array([c["inject"] is not None for c in cases])
    np.testing.assert_array_equal(got[~injected], got_twin[~injected])
    for i in np.nonzero(injected)[0]:
        assert got_twin[i] == tr.claimed_bits(dict(cases[i], inject=None), cfg)[0], cases[i]["name"]
    env.close()


def test_motion_over_through_the_replay_step(tmp_path):
    from tests.test_oracle_env import clamp_clip
    clip = clamp_clip(tmp_path)
    probe = kit.make_env(1, clip.path, auto_reset=False)
    cases = tr.motion_over_cases(probe.cfg)
    probe.close()
    env = kit.make_env(len(cases), clip.path, auto_reset=False)
    assert not env.clips[0].flags & _abi.CLIP_WRAP
    backend = GpuReplay(env, tr.replay_uniforms(len(cases)))
    run = tr.run_replay_grid(backend, cases, env.cfg, env.clips[0])
    got = check_grid(env, run, env.cfg, env.clips[0], "replay_motion_over")
    assert tr.histogram(got)["motion_over"] == 3
    env.close()


# ---- every instantiation of the live step, far cases only ---------------------------------------------------------------------------
def _rotated(quat, axis, angle):
    axis = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    return kit.pr.qmul(np.concatenate([axis * np.sin(0.5 * angle), [np.cos(0.5 * angle)]]), quat)


LIVE_NAMES = ["on the reference", "displaced 1.5 m", "turned 2.5 rad in the air", "upside down on the plane", "one step before the time limit",
              "displaced, turned, out of time", "padding", "padding"]
LIVE_CLAIMED = [0, tr.ROOT_POS, tr.ROOT_ROT, tr.CONTACT_FALL | tr.ROOT_ROT, tr.TIME_LIMIT, tr.ROOT_POS | tr.ROOT_ROT | tr.TIME_LIMIT, 0, 0]


def live_records(rec, lay, model, margin):
    """The eight robots of a live step from their records after a reset -> (records of float32 values, the proxies' clearances at the start)"""
    rng = np.random.RandomState(6)
    n = len(LIVE_NAMES)
    rec = rec.copy()
    P, Q, E, M = lay.sl("POS"), lay.sl("QUAT"), lay.sl("EP_STEP"), lay.sl("MAX_EP_STEPS")
    for i in range(n):                                   # everybody starts on the reference, at rest in its joints
        rec[i, P], rec[i, Q], rec[i, lay.sl("Q")] = rec[i, lay.sl("REF_POSE")][0:3], rec[i, lay.sl("REF_POSE")][3:7], rec[i, lay.sl("REF_POSE")][7:19]
    rec[1, P] += 1.5 * np.array([0.6, -0.8, 0.0])
    rec[2, P] += [0.0, 0.0, 0.6]
    rec[2, Q] = _rotated(rec[2, Q], rng.randn(3), 2.5)
    rec[3, Q] = _rotated(rec[3, Q], [1.0, 0.0, 0.0], np.pi)
    rec[3, P][2] = 0.0
    low = np.sort(tr.proxy_clearance64(model, rec[3, P], rec[3, Q], rec[3, lay.sl("Q")], margin))
    k = 4 + int(np.argmax(np.diff(low)[3:8]))            # the contact threshold in the middle of the widest gap behind 4 to 8 proxies
    assert low[k] - low[k - 1] >= 0.02
    rec[3, P][2] = -0.5 * (low[k - 1] + low[k])
    rec[4, E] = rec[4, M] - 1
    rec[5, P] += [1.2, 0.9, 0.6]
    rec[5, Q] = _rotated(rec[5, Q], rng.randn(3), 2.5)
    rec[5, E] = rec[5, M] - 1
    for name in ("LINVEL", "ANGVEL", "QD", "LAMBDA"):
        rec[:, lay.sl(name)] = 0.0
    rec = kit.statemod.to_float64(lay, kit.statemod.from_float64(lay, rec))
    start_clear = np.array([tr.proxy_clearance64(model, rec[i, P], rec[i, Q], rec[i, lay.sl("Q")], margin) for i in range(n)])
    assert (np.abs(start_clear) >= 0.01).all() and ((start_clear[3] < -0.01).sum() >= 4)
    return rec, start_clear


@pytest.mark.parametrize("row", list(ROWS))
def test_every_unit_of_the_live_step_gives_the_reasons(row, monkeypatch):
    import torch
    if row == "two_wave":
        monkeypatch.setenv("ORR_STEP_WAVES_PER_EU", "2")
    kw = dict(ROWS[row][0])
    files = kw.pop("files", "laikago_pace")
    if "push" in kw:
        kw["push"] = dict(kw["push"], prob=0.0)          # the unit runs, nobody is kicked
    n = 8
    env = kit.make_env(n, files, auto_reset=False, **kw)
    orc = ol.OracleEnv(env.cfg, env.models, env.clips, n, robot_type=env.robot_type, clip_id=env.clip_id)
    env.reset()
    lay, cfg, model = env.layout, env.cfg, env.models[0]
    margin = float(ol.dec32(cfg.contact_margin))
    rec, start_clear = live_records(kit.gpu_state64(env), lay, model, margin)
    E = lay.sl("EP_STEP")
    names, claimed = LIVE_NAMES, LIVE_CLAIMED
    fall = (start_clear < 0).any(axis=1)
    kit.push_state(env, rec)
    orc.state[:] = rec
    act = np.zeros((n, 12), dtype=np.float32)
    _, reward, done, _ = env.step(torch.from_numpy(act).to(env.device))
    orc.step(act.astype(np.float64))
    np.testing.assert_array_equal((orc.field("DONE_REASON")[:, 0].astype(int) & tr.CONTACT_FALL) != 0, fall)      # the oracle's flag for the same step
    after = kit.gpu_state64(env)
    got = after[:, lay.sl("DONE_REASON")][:, 0].astype(int)
    nearest = np.inf
    for i in range(n):
        clip = env.clips[int(after[i, lay.sl("CLIP_ID")][0])]
        bits, m = tr.reason64(after[i], cfg, clip, int(fall[i]), ep_step_before=int(rec[i, E][0]))
        assert abs(m["pos"]) >= 0.05 and abs(m["rot"]) >= 0.05 and m["motion"] is None, (names[i], m)
        assert bits == claimed[i], (names[i], bits, m)
        assert got[i] == bits, (names[i], got[i], bits, m)
        nearest = min(nearest, abs(m["pos"]), abs(m["rot"]))
    np.testing.assert_array_equal(done.cpu().numpy().astype(bool), got != 0)
    assert np.isfinite(reward.cpu().numpy()).all()
    # auto-reset twin: the same done and the same word (the reset keeps the ended episode's reason, which orr_task.h's reset_robot_state
    # promises and the shaping kernel relies on), the ended episode's length and the episode counter
    auto = kit.make_env(n, files, auto_reset=True, **kw)
    auto.reset()
    kit.push_state(auto, rec)
    before = int(auto.counters[_abi.CNT_EPISODES].item())
    _, _, done_auto, _ = auto.step(torch.from_numpy(act).to(auto.device))
    twin = kit.gpu_state64(auto)
    ended = got != 0
    np.testing.assert_array_equal(done_auto.cpu().numpy().astype(bool), ended)
    np.testing.assert_array_equal(twin[:, lay.sl("DONE_REASON")][:, 0].astype(int), got)
    np.testing.assert_array_equal(twin[ended][:, lay.sl("LAST_EP_LEN")][:, 0], rec[ended][:, E][:, 0] + 1)
    assert (twin[ended][:, E][:, 0] == 0).all() and int(auto.counters[_abi.CNT_EPISODES].item()) - before == int(ended.sum()) == 5
    tr.report("live_" + row, n, nearest, max(tr.ang_bound(), tr.pos_bound(1.0)), 0)
    env.close(); orc.close(); auto.close()
