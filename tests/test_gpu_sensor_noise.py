"""Sensor noise on the MI355X (orr_set_sensor_noise; Minitaur._observation_noise_stdev): the sensor variants of the kernels
(csrc/orr_kernels_sensor.hip) add zero-mean Gaussian noise to every reading of the noisy getters - the motor angle that each sub-step's
+-0.2 rad command clip is centred on, the interpolation's start value and the filter history's initial value of an episode's first step,
the three-deep sensor histories and the rpy that the target observation's heading is formed from.  Every draw is keyed by the episode's
Philox stream, so the host predicts each of them from orc_uniform (env.sensor_noise_block, env.sensor_noise_normals); the reference's
own Python, driven with the same draws, is the fixture tests/golden/task_laikago_sensor_noise.npz.  The CPU oracle never adds noise.

Bounds.  normal_pair: |z - z_float64| <= 1e-6 (tests/test_gpu_init_noise.py), so a noisy word carries stdev x 1e-6 of it and a torque
kp x motor_angle_std x 1e-6.  Replay: the bounds of tests/test_gpu_golden_task.py for the same quantities, plus those.  Product path: a
noisy word is one fused multiply-add, reading + stdev z rounded once: 2^-23 |x| + stdev x 1e-6."""
import ctypes as C
import os

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, robots
from openroborl_amd import env as envmod
from tests import oracle_lib as ol
from tests.gpu_kit import make_env

pytestmark = pytest.mark.gpu

GOLDEN = "task_laikago_sensor_noise.npz"
ALL_ON = [0.02, 0.0, 0.0, 0.03, 0.1]
HIST, FILTER, TARGET = envmod.SENSOR_SLOT_HIST, envmod.SENSOR_SLOT_FILTER, envmod.SENSOR_SLOT_TARGET
f32v = lambda x: float(np.float32(x))        # what the device holds


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32 if x.element_size() == 4 else np.uint8)


def normals(L, seed, robot, ep, i, slot, lane):
    """the four normals of a block of robot `robot`'s episode `ep`: z0, z1 of the words (0, 1), z0, z1 of the words (2, 3)"""
    blk = int(envmod.sensor_noise_block(i, slot, lane))
    return envmod.sensor_noise_normals([L.orc_uniform(int(seed), int(robot), int(ep), 4 * blk + w) for w in range(4)])


def stream(env):
    I = lambda k: env.field_int(k)[:, 0].cpu().numpy().astype(np.int64)
    return I("ROBOT_INDEX"), I("EPISODE_IDX"), I("EP_STEP")


def hist(env, name, width):
    return env.field(name).cpu().numpy().reshape(env.num_robot, 3, width)      # [N][entry: newest first][column]


def short(n_steps):
    """every episode runs into a time limit of n_steps: inline auto-resets within a few steps"""
    return dict(config_overrides=dict(ep_len_start=n_steps, ep_len_end=n_steps))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_hip_replay_reproduces_the_reference_sensor_noise():
    """tests/golden/task_laikago_sensor_noise.npz - the reference's own WrapperEnv / Minitaur with _observation_noise_stdev = (0.02, 0.5,
    0.5, 0.03, 0.1), its normals taken from the device's Philox stream by call site - replayed through orr_debug_replay_reset / _step on
    a handle with the fixture's deviations (the sensor variants' MODE 2 kernel and reset): observations, reward, done, torques
    [n, 33, 12] and the post-reset state at tests/test_gpu_golden_task.py's bounds plus the propagated normal_pair bound."""
    import torch
    g = np.load(os.path.join(ol.GOLDEN, GOLDEN))
    n = int(g["num_robot"])
    sd = [float(x) for x in g["sensor_noise"]]
    env = envmod.VecQuadrupedEnv(num_robot=n, robot=str(g["robot"]), motion_file=str(g["clip"]), mode="train", enable_randomizer=bool(g["randomizer"]),
                                 auto_reset=False, legacy_grid=True, seed=int(g["seed"]), observation_noise_stdev=sd,
                                 config_overrides=dict(ep_len_start=int(g["ep_start"]), ep_len_end=int(g["ep_end"]), curriculum_steps=int(g["curriculum_steps"])))
    dev = env.device
    m = env.models[int(env.robot_type[0])]
    jom = np.asarray(m["joint_of_motor"])
    mdir = np.asarray(m["motor_dir"])
    kp = float(np.max(np.asarray(m["kp"])))
    za, zr, zd = sd[0] * 1e-6, sd[3] * 1e-6, sd[4] * 1e-6          # the propagated normal_pair bound of a word
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    F = lambda name: env.field(name).cpu().numpy()
    count, worst = 0, {"obs": 0.0, "tau": 0.0, "rew": 0.0, "imu": 0.0}
    tau_out = torch.zeros((n, 33, 12), dtype=torch.float32, device=dev)

    def check_obs(obs, ro, what):
        imu, rimu = obs[:, 0:12].reshape(n, 3, 4), ro[:, 0:12].reshape(n, 3, 4)
        np.testing.assert_allclose(imu[:, :, 0:2], rimu[:, :, 0:2], atol=1e-5 + zr, rtol=0, err_msg=what + "IMU roll / pitch")
        np.testing.assert_allclose(imu[:, :, 2:4], rimu[:, :, 2:4], atol=1e-3 + zd, rtol=1e-5, err_msg=what + "IMU rates")
        np.testing.assert_allclose(obs[:, 12:48], ro[:, 12:48], atol=1e-5, rtol=0, err_msg=what + "last actions")
        np.testing.assert_allclose(obs[:, 48:84], ro[:, 48:84], atol=1e-5 + za, rtol=0, err_msg=what + "motor angles")
        np.testing.assert_allclose(obs[:, 84:], ro[:, 84:], atol=1e-5 + zr, rtol=0, err_msg=what + "target frames")
        worst["obs"] = max(worst["obs"], float(np.abs(obs[:, 12:] - ro[:, 12:]).max()))
        worst["imu"] = max(worst["imu"], float(np.abs(imu[:, :, 0:2] - rimu[:, :, 0:2]).max()))

    for kind, idx in g["marks"]:
        idx = int(idx)
        if kind == 0.0:
            env.counters[_abi.CNT_TOTAL_STEP_COUNT] = count
            obs = env.replay_reset(f32(g["reset/uniforms"][idx])).cpu().numpy()
            R = lambda key: g["reset/" + key][idx]
            what = "reset %d " % idx
            st = env.state[:, 0:37].cpu().numpy()
            check_obs(obs.astype(np.float64), R("obs").astype(np.float64), what)
            np.testing.assert_array_equal(env.field_int("MAX_EP_STEPS")[:, 0].cpu().numpy(), R("max_episode_steps").astype(int), err_msg=what + "time limit")
            np.testing.assert_array_equal(env.field_int("WARMUP")[:, 0].cpu().numpy(), R("warmup").astype(int), err_msg=what + "warm-up flag")
            np.testing.assert_array_equal(env.field_int("RING_LEN")[:, 0].cpu().numpy(), R("ring_len").astype(int))
            np.testing.assert_allclose(st[:, 0:7], R("state37")[:, 0:7], atol=2e-6, err_msg=what + "teleported base pose")
            np.testing.assert_allclose(st[:, 13:25], R("state37")[:, 13:25], atol=2e-6, err_msg=what + "teleported joints")
            np.testing.assert_allclose(st[:, 7:13], R("state37")[:, 7:13], atol=2e-4, err_msg=what + "teleported base velocity")
            np.testing.assert_allclose(st[:, 25:37], R("state37")[:, 25:37], atol=2e-3, rtol=1e-5, err_msg=what + "teleported joint rates")
            np.testing.assert_allclose(F("TIME_OFFSET")[:, 0], R("time_offset"), atol=1e-6)
            np.testing.assert_allclose(F("ORIGIN_POS"), R("origin_pos"), atol=2e-6)
            np.testing.assert_allclose(F("ORIGIN_ROT"), R("origin_rot"), atol=2e-6)
            np.testing.assert_allclose(F("PREV_PHASE")[:, 0], R("prev_phase"), atol=1e-6, err_msg=what + "phase")
            np.testing.assert_allclose(F("REF_POSE"), R("ref_pose"), atol=5e-6, err_msg=what + "reference pose")
        else:
            S = lambda key: g["step/" + key][idx]
            eff = np.stack([S("eff_sim"), S("eff_ref")], axis=1)
            fall = torch.tensor(S("fall").astype(np.uint8), device=dev)
            obs, rew, done = env.replay_step(f32(S("action")), f32(S("traj")), f32(eff), fall, tau_out)
            obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
            what = "step %d " % idx
            tau = tau_out.cpu().numpy().astype(np.float64) * mdir[None, None, :]
            ref_tau = S("tau_urdf").astype(np.float64)[:, :, jom]
            print("GOLDEN_SENSOR step %d: worst |d tau| %.3e" % (idx, float(np.abs(tau - ref_tau).max())))
            np.testing.assert_allclose(tau, ref_tau, atol=2e-3 + kp * za, rtol=2e-5, err_msg=what + "motor torques")
            check_obs(obs.astype(np.float64), S("obs").astype(np.float64), what)
            np.testing.assert_allclose(rew, S("reward"), atol=5e-6, err_msg=what + "reward")
            np.testing.assert_array_equal(done, S("done").astype(bool), err_msg=what + "done")
            np.testing.assert_allclose(F("ORIGIN_POS"), S("origin_pos"), atol=5e-6, err_msg=what + "origin (cycle sync)")
            np.testing.assert_allclose(F("REF_POSE"), S("ref_pose"), atol=1e-5, err_msg=what + "reference pose")
            worst["tau"] = max(worst["tau"], float(np.abs(tau - ref_tau).max()))
            worst["rew"] = max(worst["rew"], float(np.abs(rew - S("reward")).max()))
            if done.any():
                count += n     # wrapper_env.py:82-83
    print("GOLDEN_SENSOR worst |d tau| %.2e  |d obs[12:]| %.2e  |d IMU roll / pitch| %.2e  |d reward| %.2e" % (worst["tau"], worst["obs"], worst["imu"], worst["rew"]))
    env.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_held_robot_shows_every_substep_draw():
    """Replay reset, then two replay steps whose trajectory holds the robot at its reset state, action +1 rad on every motor, on a handle
    with motor_angle_std = 0.02 and on one without the call.  The PD law's angle and rate are the same in both, so the difference of the
    two handles' tau_out[k, m] is strength x kp x (cmd_noisy - cmd_free), and the command is predicted on the host in float64 from the
    reference's formulas: filter history initialised with the reading of slot 18, interpolation from the reading z1 of the sub-step in
    step 1 (from the previous filtered action in step 2), clip centred on the reading z0 of the sub-step.  Where the clip binds on its
    upper side in both handles that is strength x kp x motor_angle_std x z0(i, k, m); step 2 does not depend on any z1.  (With +1 rad the
    clip binds in 1643 of the 2376 entries of step 2 and in none of step 1, where the filter passes 11 % of the step change.)  The control
    latency is set to 0 in both records, so that the delayed motor angle is the held one in every sub-step.
    Bound: kp x motor_angle_std x 1e-6 (normal_pair) + 2^-22 of each torque (float32 rounding of the torque and of the PD law's two
    products) + kp x 8 x 2^-24 x |cmd| (the command of each handle goes through about four float32 operations at its own magnitude)."""
    import torch
    L = ol.lib()
    n, sa = 6, 0.02
    kw = dict(auto_reset=False, mode="test", enable_randomizer=False, seed=9)
    noisy, free = make_env(n, observation_noise_stdev=[sa, 0, 0, 0, 0], **kw), make_env(n, **kw)
    dev = noisy.device
    rng = np.random.RandomState(2)
    uni = rng.uniform(0.0, 1.0, (n, 28)).astype(np.float32)
    uni[:, 26] = 0.0            # reference state initialisation for every robot: the clip's pose at a drawn time
    m = noisy.models[int(noisy.robot_type[0])]
    jom, mdir, moff = np.asarray(m["joint_of_motor"]), np.asarray(m["motor_dir"], dtype=np.float64), np.asarray(m["motor_offset"], dtype=np.float64)
    kp, init = np.asarray(m["kp"], dtype=np.float64), np.asarray(m["init_motor_angles"], dtype=np.float64)
    taus = {}
    for name, env in (("noisy", noisy), ("free", free)):
        env.replay_reset(torch.from_numpy(uni).to(dev))
        env.field("LATENCY")[:] = 0.0
        st = env.state[:, 0:37].clone()
        traj = st[:, None, :].repeat(1, 33, 1).contiguous()
        eff = torch.zeros((n, 2, 8, 3), dtype=torch.float32, device=dev)
        fall = torch.zeros(n, dtype=torch.uint8, device=dev)
        act = torch.ones((n, 12), dtype=torch.float32, device=dev)
        out = []
        for k in range(2):
            tau = torch.zeros((n, 33, 12), dtype=torch.float32, device=dev)
            env.replay_step(act, traj, eff, fall, tau)
            out.append(tau.cpu().numpy().astype(np.float64))
        taus[name] = out
    assert np.array_equal(bits(noisy.state[:, 0:37]), bits(free.state[:, 0:37]))          # the same held state
    index, ep, ep_step = stream(noisy)
    assert (ep_step == 2).all()
    q = noisy.state[:, 13:25].cpu().numpy().astype(np.float64)
    co = (q[:, jom] - moff) * mdir                      # the held motor angles = the control observation at latency 0
    assert np.abs(co).max() < np.pi - 0.5
    strength = noisy.field("STRENGTH").cpu().numpy().astype(np.float64)
    fb, fa = np.zeros(3), np.zeros(3)
    fs = 1.0 / (float(noisy.cfg.sim_dt) * noisy.cfg.action_repeat)
    K = np.tan(np.pi * (4.0 / (0.5 * fs)) / 2.0)
    den = 1.0 + np.sqrt(2.0) * K + K * K
    fb[:] = [f32v(K * K / den), f32v(2.0 * K * K / den), f32v(K * K / den)]
    fa[:] = [1.0, f32v(2.0 * (K * K - 1.0) / den), f32v((1.0 - np.sqrt(2.0) * K + K * K) / den)]
    seed, sig, step_max = int(noisy.cfg.seed), f32v(sa), float(noisy.cfg.max_angle_change)
    z = np.zeros((2, n, 33, 12, 2))                     # [step][robot][sub-step][motor][z0, z1]
    zf = np.zeros((n, 12))
    for r in range(n):
        for mtr in range(12):
            zf[r, mtr] = normals(L, seed, index[r], ep[r], 1, FILTER, mtr)[0]
            for s in range(2):
                for slot in range(17):
                    z4 = normals(L, seed, index[r], ep[r], 1 + s, slot, mtr)
                    z[s, r, 2 * slot, mtr] = z4[0:2]
                    if 2 * slot + 1 < 33:
                        z[s, r, 2 * slot + 1, mtr] = z4[2:4]
    act = 1.0 + init[None, :]
    lerp = (np.arange(33) + 1.0)[None, :, None] / 33.0

    def commands(sigma):
        d = co + sigma * zf
        y1 = fb[0] * act + (fb[1] + fb[2]) * d - (fa[1] + fa[2]) * d
        y2 = fb[0] * act + fb[1] * act + fb[2] * d - fa[1] * y1 - fa[2] * d
        out, raw = [], []
        for s, (y, prev) in enumerate(((y1, None), (y2, y1))):
            cur = co[:, None, :] + sigma * z[s, :, :, :, 0]
            p = co[:, None, :] + sigma * z[s, :, :, :, 1] if prev is None else prev[:, None, :]
            c = p + lerp * (y[:, None, :] - p)
            raw.append(c - cur)
            out.append(np.clip(c, cur - step_max, cur + step_max))
        return out, raw
    cmd_n, raw_n = commands(sig)
    cmd_f, raw_f = commands(0.0)
    shown = 0
    for s in range(2):
        want = strength[:, None, :] * kp[None, None, :] * (cmd_n[s] - cmd_f[s])
        got = taus["noisy"][s] - taus["free"][s]
        tol = kp * sig * 1e-6 + 2.0 ** -22 * (np.abs(taus["noisy"][s]) + np.abs(taus["free"][s])) + kp * 8 * 2.0 ** -24 * np.maximum(np.abs(cmd_n[s]), np.abs(cmd_f[s]))
        # a command within float32 rounding of a clip bound may fall on either side of it: those entries are checked against both outcomes
        edge = np.minimum(np.abs(np.abs(raw_n[s]) - step_max), np.abs(np.abs(raw_f[s]) - step_max)) < 1e-5
        err = np.abs(got - want)
        print("HELD step %d: worst |d tau - prediction| / bound %.3f; upper clip in both handles in %d of %d entries; near a bound %d"
              % (s + 1, float((err / tol)[~edge].max()), int(((raw_n[s] > step_max) & (raw_f[s] > step_max)).sum()), err.size, int(edge.sum())))
        assert (err[~edge] <= tol[~edge]).all(), (s, float((err / tol)[~edge].max()))
        assert (err[edge] <= tol[edge] + kp.max() * 2e-5).all()
        both = (raw_n[s] > step_max + 1e-5) & (raw_f[s] > step_max + 1e-5)
        bound = (strength[:, None, :] * kp[None, None, :] * sig * z[s, :, :, :, 0])
        assert (np.abs(got - bound)[both] <= tol[both]).all()            # the clip binds on its upper side: kp sigma z0, nothing else
        shown += int(both.sum())
        assert (np.abs(got) > 10 * tol).mean() > 0.9                     # the draws are in nearly every torque
    assert shown > 0
    # step 1 depends on z1 where the clip does not bind: there the noise-free handle's prediction without z1 is off by far more than the bound
    open1 = (np.abs(raw_n[0]) < step_max - 1e-5) & (np.abs(raw_f[0]) < step_max - 1e-5)
    assert open1.any()
    noisy.close(); free.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_imu_and_target_noise_touch_the_imu_words_and_the_heading_only():
    """motor_angle_std = 0, rpy 0.03, rate 0.1: 10 robots, fixed actions, episodes of 2 and 3 steps (inline auto-resets), 6 steps.  Against
    an env that never had the call: the whole record but the IMU history bit for bit (rigid state, ring, motor-angle history included);
    the newest IMU words = that env's + sigma z of slot 17 (all three entries after a reset), within 2^-23 |x| + sigma x 1e-6; the target
    frames' joint words bit for bit, their z and planar norm to 1e-6, and one planar rotation for all four frames (1e-5), non-zero."""
    import torch
    L = ol.lib()
    n, sr, sd = 10, 0.03, 0.1
    a, b = make_env(n, observation_noise_stdev=[0, 0, 0, sr, sd], **short(3)), make_env(n, **short(3))
    oa, ob = a.reset(), b.reset()
    for env in (a, b):     # robots 0, 3, 6, 9 end after two steps, the others after three
        env.field_int("MAX_EP_STEPS")[:, 0] = torch.tensor([2 if r % 3 == 0 else 3 for r in range(n)], dtype=torch.int32, device=env.device)
    seed = int(a.cfg.seed)
    lay = a.layout
    imu = lay.sl("IMU_HIST")
    g = torch.Generator(device="cpu"); g.manual_seed(3)
    sig = np.array([f32v(sr), f32v(sr), f32v(sd), f32v(sd)])
    resets, angles = 0, []

    def check(k, done, prev_a):
        sa_, sb_ = a.state.clone(), b.state.clone()
        sa_[:, imu] = 0.0; sb_[:, imu] = 0.0
        np.testing.assert_array_equal(bits(sa_), bits(sb_), err_msg="record outside the IMU history, step %d" % k)
        index, ep, ep_step = stream(b)
        ha, hb = hist(a, "IMU_HIST", 4).astype(np.float64), hist(b, "IMU_HIST", 4).astype(np.float64)
        for r in range(n):
            if done[r]:      # three readings of the new episode's stream, i = 0; the first one is the oldest entry
                zz = np.stack([normals(L, seed, index[r], ep[r], 0, HIST, 12 + c)[0:3] for c in range(4)], axis=1)      # [reading][channel]
                want = hb[r, ::-1] + sig * zz
                got = ha[r, ::-1]
                assert len({got[j].tobytes() for j in range(3)}) == 3
            else:
                zz = np.array([normals(L, seed, index[r], ep[r], ep_step[r], HIST, 12 + c)[0] for c in range(4)])
                want, got = hb[r, 0] + sig * zz, ha[r, 0]
                if prev_a is not None:      # the older entries moved down by one
                    np.testing.assert_array_equal(ha[r, 1:3], prev_a[r, 0:2])
            tol = 2.0 ** -23 * np.abs(want) + sig * 1e-6
            assert (np.abs(got - want) <= tol).all(), (k, r, float((np.abs(got - want) / tol).max()))
        # the observation: IMU words are the history's, everything up to the target frames is the noise-free env's
        xa, xb = a.obs.cpu().numpy(), b.obs.cpu().numpy()
        np.testing.assert_array_equal(xa[:, 0:12].view(np.uint32), a.field("IMU_HIST").cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(xa[:, 12:84].view(np.uint32), xb[:, 12:84].view(np.uint32))
        fa_, fb_ = xa[:, 84:].reshape(n, 4, 19).astype(np.float64), xb[:, 84:].reshape(n, 4, 19).astype(np.float64)
        np.testing.assert_array_equal(xa[:, 84:].reshape(n, 4, 19)[:, :, 7:].view(np.uint32), xb[:, 84:].reshape(n, 4, 19)[:, :, 7:].view(np.uint32))
        np.testing.assert_allclose(fa_[:, :, 2], fb_[:, :, 2], atol=1e-6, rtol=0)
        np.testing.assert_allclose(np.hypot(fa_[:, :, 0], fa_[:, :, 1]), np.hypot(fb_[:, :, 0], fb_[:, :, 1]), atol=1e-6, rtol=0)
        # rotation about z from the noise-free frame to the noisy one: from the orientations (q_a = dq (x) q_b) and, where the frame's
        # planar offset is long enough to carry an angle, from the positions
        qa, qb = fa_[:, :, 3:7], fb_[:, :, 3:7]
        qbc = qb * np.array([-1.0, -1.0, -1.0, 1.0])
        x1, y1, z1, w1 = (qa[..., j] for j in range(4))
        x0, y0, z0, w0 = (qbc[..., j] for j in range(4))
        dz = x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0
        dw = -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0
        ang = 2.0 * np.arctan2(dz, dw)
        ang = (ang + np.pi) % (2.0 * np.pi) - np.pi
        assert (np.abs(ang - ang[:, 0:1]) <= 1e-5).all(), (k, float(np.abs(ang - ang[:, 0:1]).max()))
        assert (np.abs(ang[:, 0]) > 1e-5).all(), k
        long_enough = np.hypot(fb_[:, :, 0], fb_[:, :, 1]) > 5e-3
        pang = np.arctan2(fb_[:, :, 0] * fa_[:, :, 1] - fb_[:, :, 1] * fa_[:, :, 0], fb_[:, :, 0] * fa_[:, :, 0] + fb_[:, :, 1] * fa_[:, :, 1])
        dev_ = np.abs(pang - ang)[long_enough]
        assert long_enough.any() and (dev_ <= 1e-5 + 2e-8 / np.hypot(fb_[:, :, 0], fb_[:, :, 1])[long_enough]).all(), (k, float(dev_.max()))
        angles.append(ang[:, 0])
        return ha

    prev = check(-1, np.ones(n, dtype=bool), None)
    for k in range(6):
        act = (torch.randn(n, 12, generator=g) * 0.125).to(a.device)
        _, ra, da, _ = a.step(act)
        _, rb, db, _ = b.step(act)
        assert torch.equal(da, db) and np.array_equal(bits(ra), bits(rb)), k
        done = db.cpu().numpy().astype(bool)
        resets += int(done.sum())
        prev = check(k, done, prev)
    assert resets >= n
    assert len({x.tobytes() for x in angles}) == len(angles)             # a new draw every observation
    a.close(); b.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_reset_takes_three_motor_angle_readings():
    """motor_angle_std = 0.02 alone: after reset() each of the three motor-angle history entries is the noise-free reset's entry plus
    sigma z of its reading - z0, z1 of the words (0, 1), z0 of the words (2, 3) of slot 17, i = 0, the first reading in the oldest
    entry - and the three differ pairwise.  Everything else of the record is the noise-free reset's, bit for bit."""
    L = ol.lib()
    n, sa = 10, 0.02
    a, b = make_env(n, observation_noise_stdev=[sa, 0, 0, 0, 0]), make_env(n)
    oa, ob = a.reset(), b.reset()
    index, ep, _ = stream(a)
    ha, hb = hist(a, "MOTORANG_HIST", 12).astype(np.float64), hist(b, "MOTORANG_HIST", 12).astype(np.float64)
    assert np.array_equal(hb[:, 0], hb[:, 1]) and np.array_equal(hb[:, 0], hb[:, 2]) and np.abs(hb).max() < np.pi - 0.5
    sig = f32v(sa)
    for r in range(n):
        zz = np.stack([normals(L, int(a.cfg.seed), index[r], ep[r], 0, HIST, c)[0:3] for c in range(12)], axis=1)     # [reading][motor]
        want, got = hb[r, ::-1] + sig * zz, ha[r, ::-1]
        tol = 2.0 ** -23 * np.abs(want) + sig * 1e-6
        assert (np.abs(got - want) <= tol).all(), (r, float((np.abs(got - want) / tol).max()))
        assert (got[0] != got[1]).all() and (got[1] != got[2]).all() and (got[0] != got[2]).all()
    lay = a.layout
    sa_, sb_ = a.state.clone(), b.state.clone()
    sa_[:, lay.sl("MOTORANG_HIST")] = 0.0; sb_[:, lay.sl("MOTORANG_HIST")] = 0.0
    np.testing.assert_array_equal(bits(sa_), bits(sb_))
    np.testing.assert_array_equal(bits(oa[:, 48:84]), bits(a.field("MOTORANG_HIST")))
    np.testing.assert_array_equal(bits(oa[:, 0:48]), bits(ob[:, 0:48]))
    np.testing.assert_array_equal(bits(oa[:, 84:]), bits(ob[:, 84:]))
    a.close(); b.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_inline_reset_equals_explicit_reset():
    """All three deviations on: a robot reset inside a step carries, bit for bit, the record and the observation that orr_reset gives a
    copy - every reset pattern of a wave, by the protocol of tests/test_gpu_step_end_order.py."""
    from tests.test_gpu_step_end_order import run
    run(observation_noise_stdev=ALL_ON)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_shards_and_determinism():
    """Two 8-robot shards (robot_index_offset 0 and 8) against the 16-robot env, all three deviations on, reset + 5 steps with episodes of
    two steps (inline resets): outputs and whole records bit for bit; a second run of the 16-robot env is bit for bit the first."""
    import torch
    from tests.test_gpu_shards import _run
    kw = dict(seed=11, mode="train", enable_randomizer=True, observation_noise_stdev=ALL_ON, **short(2))
    big, again = make_env(16, **kw), make_env(16, **kw)
    a, b = make_env(8, robot_index_offset=0, num_procs=2, **kw), make_env(8, robot_index_offset=8, num_procs=2, **kw)
    f1, o1 = _run(torch, [big], [0], 16, 5)
    f2, o2 = _run(torch, [a, b], [0, 8], 16, 5)
    f3, o3 = _run(torch, [again], [0], 16, 5)
    assert torch.equal(f1, f2) and torch.equal(f1, f3)
    n_done = 0
    for k, (x, y, w) in enumerate(zip(o1, o2, o3)):
        for j, what in enumerate(("observation", "reward", "done")):
            assert torch.equal(x[j], y[j]), "%s, step %d (shards)" % (what, k)
            assert torch.equal(x[j], w[j]), "%s, step %d (second run)" % (what, k)
        n_done += int(x[2].sum())
    assert n_done >= 16
    assert torch.equal(big.state.view(torch.int32), torch.cat([a.state, b.state]).view(torch.int32))
    assert torch.equal(big.state.view(torch.int32), again.state.view(torch.int32))
    quiet = make_env(16, **dict(kw, observation_noise_stdev=None))
    f4, _ = _run(torch, [quiet], [0], 16, 1)
    assert not torch.equal(f1, f4)                     # the noise is there
    for e in (big, again, a, b, quiet):
        e.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [False, True], ids=["plain", "outputs_bound"])
def test_off_is_off(bound):
    """All zeros, and only the velocity / torque deviations above 0 (no consumer): observations, rewards, done flags, records - and, bound,
    the reward terms, contact and actuator outputs - over reset + 5 steps are bit for bit those of an env that never had the call; so
    are those of an env whose noise was set and cleared again."""
    import torch
    n = 10
    kw = dict(mode="train", enable_randomizer=True, **short(2))
    if bound:
        kw.update(reward_terms=True, contact_outputs=True, actuator_outputs=True)
    ref = make_env(n, **kw)
    zeros, inert, cleared = make_env(n, **kw), make_env(n, observation_noise_stdev=[0.0, 0.5, 0.5, 0.0, 0.0], **kw), make_env(n, observation_noise_stdev=ALL_ON, **kw)
    zeros.set_sensor_noise([0.0] * 5)
    cleared.set_sensor_noise(None)
    envs = [ref, zeros, inert, cleared]
    obs = [e.reset() for e in envs]
    g = torch.Generator(device="cpu"); g.manual_seed(1)

    def same(k):
        for e, o in zip(envs[1:], obs[1:]):
            assert torch.equal(obs[0], o), k
            assert torch.equal(ref.state.view(torch.int32), e.state.view(torch.int32)), k
            assert torch.equal(ref.counters, e.counters), k
            if bound:
                for name in ("reward_terms", "episode_term_sums", "contact_out", "episode_contact", "actuator_out", "episode_actuator"):
                    assert np.array_equal(bits(getattr(ref, name)), bits(getattr(e, name))), (k, name)
    same(-1)
    dones = 0
    for k in range(5):
        act = (torch.randn(n, 12, generator=g) * 0.125).to(ref.device)
        outs = [e.step(act) for e in envs]
        obs = [o[0] for o in outs]
        for o in outs[1:]:
            assert np.array_equal(bits(outs[0][1]), bits(o[1])) and torch.equal(outs[0][2], o[2]), k
        same(k)
        dones += int(outs[0][2].sum())
    assert dones >= n
    for e in envs:
        e.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """A NaN, a negative and an infinite value in each field fail with a status and an orr_last_error() that names the field; the handle
    then steps as an untouched twin does.  Friction anchors: orr_set_sensor_noise refuses them on the handle, and an anchor model set on
    a noisy handle makes the launches fail and launch nothing."""
    import torch
    L = _lib.load()
    env, twin = make_env(8, observation_noise_stdev=ALL_ON), make_env(8, observation_noise_stdev=ALL_ON)
    for name in _abi.SENSOR_NOISE_FIELDS:
        for bad in (float("nan"), -0.1, float("inf")):
            s = envmod.sensor_noise_spec([0.5, 0.5, 0.5, 0.5, 0.5])
            setattr(s, name, bad)
            assert L.orr_set_sensor_noise(env.h, C.byref(s)) == -1, (name, bad)
            assert name.encode() in L.orr_last_error() and b"orr_set_sensor_noise" in L.orr_last_error(), (name, bad, L.orr_last_error())
    oe, ot = env.reset(), twin.reset()
    assert torch.equal(oe, ot)
    act = torch.zeros(8, 12, device=env.device)
    for k in range(3):
        env.step(act); twin.step(act)
    assert torch.equal(env.state.view(torch.int32), twin.state.view(torch.int32)) and torch.equal(env.obs, twin.obs)
    twin.close()
    # friction anchors on the handle: the setter refuses, the env constructor reports it
    with pytest.raises(RuntimeError, match="friction anchors"):
        make_env(8, observation_noise_stdev=ALL_ON, model_overrides={"laikago": {"friction_anchor": 1}})
    quiet = make_env(8, model_overrides={"laikago": {"friction_anchor": 1}})           # all-off and inert noise on an anchor handle is fine
    assert L.orr_set_sensor_noise(quiet.h, C.byref(envmod.sensor_noise_spec([0.0, 0.5, 0.5, 0.0, 0.0]))) == 0 and L.orr_set_sensor_noise(quiet.h, None) == 0
    assert L.orr_set_sensor_noise(quiet.h, C.byref(envmod.sensor_noise_spec([0.0, 0.0, 0.0, 0.0, 0.1]))) == -1 and b"friction anchors" in L.orr_last_error()
    quiet.close()
    # an anchor model on the noisy handle: every launch is refused and nothing runs
    t = robots.ROBOT_TYPE_ID["laikago"]
    m = dict(env.models[t])
    m["friction_anchor"] = 1
    assert L.orr_set_model(env.h, t, C.byref(robots.to_struct(m))) == 0
    torch.cuda.synchronize()
    before_state, before_obs = env.state.clone(), env.obs.clone()
    with pytest.raises(RuntimeError, match="friction anchors"):
        env.reset()
    with pytest.raises(RuntimeError, match="friction anchors"):
        env.step(act)
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), before_state.view(torch.int32)) and torch.equal(env.obs, before_obs)
    env.close()
