"""Task noise on the MI355X (orr_set_task_noise; ImitationTask's perturb_init_state_prob with _apply_state_perturb, and tar_obs_noise[0]):
the noise variants of the kernels (csrc/orr_kernels_noise.hip) start an episode on a Gaussian-perturbed copy of the reference state with
the given probability and express every target observation in a noisy heading.  Every draw is keyed by the episode's Philox stream, so
the host predicts each of them exactly from orc_uniform (env.init_perturb_draws, env.tar_noise_block, env.normal_pair); the reference's
own Python, driven with the same draws, is the fixture tests/golden/task_laikago_noise.npz.  The CPU oracle never perturbs.

Bounds.  normal_pair: |z - z_float64| <= 1e-6 for every radius uniform (derived in csrc/orr_device.h: the largest deviation the noise
multiplies it by is 0.05 pi, so a state word is off by at most 1.6e-7, below the 2e-6 of the replay tests).  Replay: the bounds of
tests/test_gpu_golden_task.py for the same quantities.  Product path: a perturbed word is one fused multiply-add, reference + std z
rounded once: 2^-24 (|ref| + 5.77 std) of rounding + std x the error of z <= 2^-23 |ref| + std x 1e-6."""
import ctypes as C
import os

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, robots
from openroborl_amd import env as envmod
from tests import oracle_lib as ol
from tests.gpu_kit import make_env, stress

pytestmark = pytest.mark.gpu

GOLDEN = "task_laikago_noise.npz"
STD = {k: float(np.float32(v)) for k, v in envmod.INIT_PERTURB_STD.items()}     # what the device holds


def qmul(a, b):      # Hamilton product, xyzw, on [..., 4] arrays (transformations.quaternion_multiply)
    x1, y1, z1, w1 = (a[..., k] for k in range(4))
    x0, y0, z0, w0 = (b[..., k] for k in range(4))
    return np.stack([x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0, x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0,
                     -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0], axis=-1)


def rigid(env):
    """Host copies (float32) of what a reset writes, and the keys of the robots' streams."""
    F = lambda k: env.field(k).cpu().numpy()
    I = lambda k: env.field_int(k)[:, 0].cpu().numpy().astype(np.int64)
    return dict(pos=F("POS"), quat=F("QUAT"), lin=F("LINVEL"), ang=F("ANGVEL"), q=F("Q"), qd=F("QD"), ref_pose=F("REF_POSE"), ref_vel=F("REF_VEL"),
                ep=I("EPISODE_IDX"), index=I("ROBOT_INDEX"), ep_step=I("EP_STEP"))


def uniforms36(L, seed, index, ep):
    return np.array([[L.orc_uniform(seed, int(i), int(e), int(d)) for d in envmod.init_perturb_draw_indices()] for i, e in zip(index, ep)])


def check_reset_states(L, env, r, who, prob, what):
    """The robots `who` have just been reset: the perturbed ones (U(0) < prob on the NEW episode's stream) carry reference + std z, the
    others the reference state bit for bit.  Returns (#perturbed, #unperturbed)."""
    who = np.asarray(who)
    if len(who) == 0:
        return 0, 0
    p = envmod.init_perturb_draws(uniforms36(L, int(env.cfg.seed), r["index"][who], r["ep"][who]), prob)
    pert = p["perturbed"]
    f64 = lambda a: a[who].astype(np.float64)
    rp, rv = f64(r["ref_pose"]), f64(r["ref_vel"])

    def close(got, ref, delta, std, name):
        err = np.abs((got - ref) - delta)[pert]
        tol = (2.0 ** -23 * np.abs(ref) + std * 1e-6)[pert]
        assert (err <= tol).all(), "%s %s: |error| / bound up to %.3f" % (what, name, (err / tol).max())
    close(f64(r["pos"])[:, 0:2], rp[:, 0:2], p["pos"], STD["root_pos_std"], "root position")
    close(f64(r["lin"])[:, 0:2], rv[:, 0:2], p["vel"], STD["root_vel_std"], "root velocity")
    close(f64(r["ang"]), rv[:, 3:6], p["ang_vel"], STD["root_ang_vel_std"], "root angular velocity")
    close(f64(r["q"]), rp[:, 7:19], p["joints"], STD["joint_pose_std"], "joint angles")
    close(f64(r["qd"]), rv[:, 6:18], p["joint_vel"], STD["joint_vel_std"], "joint rates")
    np.testing.assert_allclose(f64(r["quat"])[pert], qmul(p["rot"], rp[:, 3:7])[pert], atol=1e-6, rtol=0, err_msg=what + " orientation")
    # z of the root position / velocity is never perturbed; nothing of an unperturbed robot is
    np.testing.assert_array_equal(r["pos"][who][:, 2], r["ref_pose"][who][:, 2], err_msg=what)
    np.testing.assert_array_equal(r["lin"][who][:, 2], r["ref_vel"][who][:, 2], err_msg=what)
    keep = who[~pert]
    for a, b in ((r["pos"], r["ref_pose"][:, 0:3]), (r["quat"], r["ref_pose"][:, 3:7]), (r["q"], r["ref_pose"][:, 7:19]),
                 (r["lin"], r["ref_vel"][:, 0:3]), (r["ang"], r["ref_vel"][:, 3:6]), (r["qd"], r["ref_vel"][:, 6:18])):
        np.testing.assert_array_equal(a[keep].view(np.int32), b[keep].view(np.int32), err_msg=what + " unperturbed robots")
    if pert.any():      # a perturbation that was applied is visible
        assert (np.abs(f64(r["q"]) - rp[:, 7:19])[pert].max(axis=1) > 1e-4).all(), what
    return int(pert.sum()), int((~pert).sum())


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_normal_pair_on_the_device():
    """All 2^24 radius uniforms x 64 angle uniforms (0, 1/4, 1/2, 3/4 and 60 others) through the probe of csrc/orr_device.h's
    normal_pair: the largest |z - z_float64| is at most 1e-6 and nothing is non-finite.  The probe reduces on the device against its own
    float64 evaluation; that evaluation is checked against numpy first, on a sample and on a range small enough to repeat on the host."""
    from tests import probe_noise_lib as pn
    rng = np.random.RandomState(7)
    ub = np.concatenate([[0.0, 0.25, 0.5, 0.75], rng.randint(0, 1 << 24, 60) / float(1 << 24)]).astype(np.float32)
    # a sample of pairs, the ends of the radius' range among them, against numpy
    ua_s = np.concatenate([[0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5], rng.randint(0, 1 << 24, 4092) / float(1 << 24)]).astype(np.float32)
    ub_s = np.concatenate([[0.0, 0.25, 0.5, 0.75], rng.randint(0, 1 << 24, 4092) / float(1 << 24)]).astype(np.float32)
    z0, z1 = pn.normal_pair(ua_s, ub_s)
    w0, w1 = envmod.normal_pair(ua_s, ub_s)
    assert np.isfinite(z0).all() and np.isfinite(z1).all()
    sample = max(np.abs(z0 - w0).max(), np.abs(z1 - w1).max())
    assert sample <= 1e-6, sample
    assert z0[0] == 0.0 and z1[0] == 0.0                                            # ua = 0: the radius is exactly 0
    # a small range, reduced on the device and again here from the plain entry point's results
    first, count = 16770000, 5000
    e_dev, i_dev, bad, covered = pn.sweep(ub[:4], first, count)
    assert bad == 0 and covered == count
    ua_r = (np.arange(first, first + count) / float(1 << 24)).astype(np.float32)
    for j in range(4):
        z0, z1 = pn.normal_pair(ua_r, np.full(count, ub[j], dtype=np.float32))
        w0, w1 = envmod.normal_pair(ua_r, np.full(count, ub[j], dtype=np.float32))
        e_host = np.maximum(np.abs(z0 - w0), np.abs(z1 - w1))
        assert abs(e_dev[j] - e_host.max()) <= 2.0 ** -27 * e_host.max() + 1e-12, (j, e_dev[j], e_host.max())
        assert first <= i_dev[j] < first + count
    # the whole sweep
    err, idx, bad, covered = pn.sweep(ub)
    worst = float(err.max()) * (1.0 + 2.0 ** -27)          # the device reports the maximum rounded down by at most 2^-28 of itself
    j = int(err.argmax())
    print("NORMAL_PAIR max |z - z_float64| over 2^24 ua x %d ub: %.3e (ua = %d / 2^24, ub = %.8f); sample of %d pairs %.3e; non-finite %d"
          % (len(ub), worst, idx[j], ub[j], len(ua_s), sample, bad))
    assert covered == 1 << 24 and bad == 0
    assert worst <= 1e-6, worst


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_hip_replay_reproduces_the_reference_noise():
    """tests/golden/task_laikago_noise.npz - the reference's own WrapperEnv / ImitationTask with perturb_init_state_prob = 0.5 and
    tar_obs_noise = [0.1], its draws taken from the device's Philox stream - replayed through orr_debug_replay_reset / _step on a handle
    with the fixture's noise (the noise variants' MODE 2 kernels): observations, reward, done, torques and the post-reset rigid state at
    tests/test_gpu_golden_task.py's bounds; the set of perturbed resets exactly."""
    import torch
    g = np.load(os.path.join(ol.GOLDEN, GOLDEN))
    n = int(g["num_robot"])
    prob, sigma = (float(x) for x in g["noise"])
    env = envmod.VecQuadrupedEnv(num_robot=n, robot=str(g["robot"]), motion_file=str(g["clip"]), mode="train", enable_randomizer=bool(g["randomizer"]),
                                 auto_reset=False, legacy_grid=True, seed=int(g["seed"]), perturb_init_state_prob=prob, tar_obs_noise=[sigma],
                                 config_overrides=dict(ep_len_start=int(g["ep_start"]), ep_len_end=int(g["ep_end"]), curriculum_steps=int(g["curriculum_steps"])))
    dev = env.device
    m = env.models[int(env.robot_type[0])]
    jom = np.asarray(m["joint_of_motor"])
    mdir = np.asarray(m["motor_dir"])
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    F = lambda name: env.field(name).cpu().numpy()
    count, npert, worst = 0, 0, {"obs": 0.0, "tau": 0.0, "rew": 0.0, "state": 0.0}
    tau_out = torch.zeros((n, 33, 12), dtype=torch.float32, device=dev)
    for kind, idx in g["marks"]:
        idx = int(idx)
        if kind == 0.0:
            env.counters[_abi.CNT_TOTAL_STEP_COUNT] = count
            obs = env.replay_reset(f32(g["reset/uniforms"][idx])).cpu().numpy()
            R = lambda key: g["reset/" + key][idx]
            what = "reset %d " % idx
            st = env.state[:, 0:37].cpu().numpy()
            ref37 = np.concatenate([F("REF_POSE")[:, 0:7], F("REF_VEL")[:, 0:6], F("REF_POSE")[:, 7:19], F("REF_VEL")[:, 6:18]], axis=1)
            moved = (st.view(np.int32) != ref37.view(np.int32)).any(axis=1)
            np.testing.assert_array_equal(moved, R("perturbed").astype(bool), err_msg=what + "the set of perturbed robots")
            np.testing.assert_allclose(obs, R("obs"), atol=2e-5, err_msg=what + "observation")
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
            np.testing.assert_allclose(F("REF_POSE"), R("ref_pose"), atol=5e-6, err_msg=what + "reference pose (unperturbed)")
            npert += int(moved.sum())
            worst["state"] = max(worst["state"], float(np.abs(st[:, 0:7] - R("state37")[:, 0:7]).max()), float(np.abs(st[:, 13:25] - R("state37")[:, 13:25]).max()))
        else:
            S = lambda key: g["step/" + key][idx]
            eff = np.stack([S("eff_sim"), S("eff_ref")], axis=1)
            fall = torch.tensor(S("fall").astype(np.uint8), device=dev)
            obs, rew, done = env.replay_step(f32(S("action")), f32(S("traj")), f32(eff), fall, tau_out)
            obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
            what = "step %d " % idx
            tau = tau_out.cpu().numpy().astype(np.float64) * mdir[None, None, :]
            ref_tau = S("tau_urdf").astype(np.float64)[:, :, jom]
            np.testing.assert_allclose(tau, ref_tau, atol=2e-3, rtol=2e-5, err_msg=what + "motor torques")
            ro = S("obs").astype(np.float64)
            np.testing.assert_allclose(obs[:, 0:12].reshape(n, 3, 4)[:, :, 0:2], ro[:, 0:12].reshape(n, 3, 4)[:, :, 0:2], atol=1e-5, err_msg=what + "IMU roll / pitch")
            np.testing.assert_allclose(obs[:, 0:12].reshape(n, 3, 4)[:, :, 2:4], ro[:, 0:12].reshape(n, 3, 4)[:, :, 2:4], atol=1e-3, rtol=1e-5, err_msg=what + "IMU rates")
            np.testing.assert_allclose(obs[:, 12:], ro[:, 12:], atol=1e-5, err_msg=what + "last actions / motor angles / target frames")
            np.testing.assert_allclose(rew, S("reward"), atol=5e-6, err_msg=what + "reward")
            np.testing.assert_array_equal(done, S("done").astype(bool), err_msg=what + "done")
            np.testing.assert_allclose(F("ORIGIN_POS"), S("origin_pos"), atol=5e-6, err_msg=what + "origin (cycle sync)")
            np.testing.assert_allclose(F("REF_POSE"), S("ref_pose"), atol=1e-5, err_msg=what + "reference pose")
            worst["tau"] = max(worst["tau"], float(np.abs(tau - ref_tau).max()))
            worst["obs"] = max(worst["obs"], float(np.abs(obs[:, 12:] - ro[:, 12:]).max()))
            worst["rew"] = max(worst["rew"], float(np.abs(rew - S("reward")).max()))
            if done.any():
                count += n     # wrapper_env.py:82-83
    print("GOLDEN_NOISE %d perturbed resets, worst |d tau| %.2e  |d obs| %.2e  |d reward| %.2e  |d teleported pose| %.2e"
          % (npert, worst["tau"], worst["obs"], worst["rew"], worst["state"]))
    assert npert == int(g["reset/perturbed"].sum()) > 0
    env.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_perturbed_resets_follow_the_host_prediction():
    """70 robots (a partial last wave), prob 0.5, train semantics with auto-reset and 5-step episodes, 40 steps: after reset() and after
    every step, each robot that was just reset is perturbed iff U(0) < prob on its new episode's stream, by std x z of the predictor."""
    L = ol.lib()
    n, prob = 70, 0.5
    env = make_env(n, mode="train", enable_randomizer=True, perturb_init_state_prob=prob,
                   config_overrides=dict(ep_len_start=5, ep_len_end=5))
    obs = env.reset()
    a, b = check_reset_states(L, env, rigid(env), np.arange(n), prob, "reset()")
    rng = np.random.RandomState(1)
    inline = 0
    for k in range(40):
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        who = np.nonzero(done.cpu().numpy())[0]
        r = rigid(env)
        assert (r["ep_step"][who] == 0).all()
        da, db = check_reset_states(L, env, r, who, prob, "step %d" % k)
        a, b, inline = a + da, b + db, inline + len(who)
    print("INIT_NOISE %d perturbed and %d unperturbed resets checked, %d of them inline" % (a, b, inline))
    assert a >= 20 and b >= 20 and inline >= 20
    env.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_heading_noise_touches_the_observation_only():
    """Twin envs, same seed, same given actions (stress_actions reads the target joints only), one with sigma = 0.1: after reset + 30
    steps (auto-reset, 7-step episodes) the records are byte-identical throughout, the proprioceptive observation and the target joints
    bit-identical, and each target root position / orientation of the noisy env is the quiet env's turned by -sigma z about z."""
    import torch
    L = ol.lib()
    n, sigma = 70, 0.1
    kw = dict(mode="train", enable_randomizer=True, config_overrides=dict(ep_len_start=7, ep_len_end=7))
    quiet, noisy = make_env(n, **kw), make_env(n, tar_obs_noise=sigma, **kw)
    assert noisy.task_noise.tar_heading_std == np.float32(sigma) and quiet.task_noise.tar_heading_std == 0.0
    sig = float(np.float32(sigma))
    seed = int(noisy.cfg.seed)
    rng = np.random.RandomState(3)
    reach, resets, rows = 0.0, 0, []

    def compare(oq, on, what):
        nonlocal reach
        assert torch.equal(quiet.state.view(torch.int32), noisy.state.view(torch.int32)), what + ": records"
        oq, on = oq.cpu().numpy(), on.cpu().numpy()
        np.testing.assert_array_equal(oq[:, :84].view(np.int32), on[:, :84].view(np.int32), err_msg=what + ": proprioception")
        tq, tn = oq[:, 84:].reshape(n, 4, 19), on[:, 84:].reshape(n, 4, 19)
        np.testing.assert_array_equal(tq[:, :, 7:].view(np.int32), tn[:, :, 7:].view(np.int32), err_msg=what + ": target joints")
        ep = noisy.field_int("EPISODE_IDX")[:, 0].cpu().numpy()
        index = noisy.field_int("ROBOT_INDEX")[:, 0].cpu().numpy()
        blk = envmod.NOISE_HEADING_BLOCK + noisy.field_int("EP_STEP")[:, 0].cpu().numpy().astype(np.int64)   # 0 after a reset, 1 + s after a step
        z = np.array([float(envmod.normal_pair(L.orc_uniform(seed, int(i), int(e), int(4 * b)), L.orc_uniform(seed, int(i), int(e), int(4 * b + 1)))[0])
                      for i, e, b in zip(index, ep, blk)])
        ang = -sig * z
        c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
        p = tq[:, :, 0:3].astype(np.float64)
        want_p = np.stack([c * p[..., 0] - s * p[..., 1], s * p[..., 0] + c * p[..., 1], p[..., 2]], axis=-1)
        d = np.zeros((n, 1, 4)); d[:, 0, 2] = np.sin(0.5 * ang); d[:, 0, 3] = np.cos(0.5 * ang)
        want_q = qmul(np.broadcast_to(d, (n, 4, 4)), tq[:, :, 3:7].astype(np.float64))
        want_q = want_q * np.where(want_q[..., 3:4] < 0.0, -1.0, 1.0)                # standardize_quaternion
        got_q = tn[:, :, 3:7].astype(np.float64)
        eq = np.minimum(np.abs(got_q - want_q).max(axis=-1), np.abs(got_q + want_q).max(axis=-1))   # w = 0: either sign
        reach = max(reach, float(np.abs(p).max()))
        rows.append((float(np.abs(tn[:, :, 0:3] - want_p).max()), float(eq.max())))
        assert np.abs(z).max() > 1.0 and np.abs(tn[:, :, 0:2] - tq[:, :, 0:2]).max() > 1e-4, what + ": the noise is there"

    oq, on = quiet.reset(), noisy.reset()
    compare(oq, on, "reset")
    for k in range(30):
        jitter = torch.from_numpy(rng.normal(0.0, 0.05, (n, 12)).astype(np.float32)).to(quiet.device)
        act = quiet.stress_actions(oq, jitter, torch.empty_like(jitter))
        assert torch.equal(act, noisy.stress_actions(on, jitter, torch.empty_like(jitter))), k      # the target joints carry no noise
        oq, rq, dq, _ = quiet.step(act)
        on, rn, dn, _ = noisy.step(act)
        assert torch.equal(rq, rn) and torch.equal(dq, dn), k
        resets += int(dq.sum())
        compare(oq, on, "step %d" % k)
    tol = 2e-6 + sig * 1e-6 * reach
    worst = max(max(r) for r in rows)
    print("HEADING_NOISE worst |d target root| %.2e (bound %.2e, largest target offset %.2f m), %d inline resets" % (worst, tol, reach, resets))
    assert worst <= tol and resets >= 20
    quiet.close(); noisy.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_clip_draws_do_not_move():
    """A clip set of three with a switch interval, with and without both noises, 60 steps without auto-reset (the perturbed robots move
    differently, so only the time decides) and a second reset() half way: CLIP_ID, CLIP_CHANGE_TIME and TIME_OFFSET are identical."""
    files = ["laikago_pace", "laikago_trot", "laikago_spin"]
    kw = dict(auto_reset=False, clip_time_min=0.1, clip_time_max=0.3)
    plain, noisy = make_env(64, files, **kw), make_env(64, files, perturb_init_state_prob=0.5, tar_obs_noise=[0.1], **kw)
    rngs = [np.random.RandomState(9), np.random.RandomState(9)]
    obs = [plain.reset(), noisy.reset()]
    first = plain.active_clip_ids().cpu().numpy()
    changed = 0
    for k in range(60):
        if k == 30:
            obs = [plain.reset(), noisy.reset()]
        for j, e in enumerate((plain, noisy)):
            obs[j] = e.step(stress(e, obs[j], rngs[j]))[0]
        for name in ("CLIP_ID", "CLIP_CHANGE_TIME", "TIME_OFFSET"):
            a, b = (e.field(name).cpu().numpy().view(np.int32) for e in (plain, noisy))
            np.testing.assert_array_equal(a, b, err_msg="%s after step %d" % (name, k))
        changed += int((plain.active_clip_ids().cpu().numpy() != first).sum())
    assert changed > 64                                               # the clips did switch
    assert (noisy.field("POS") != plain.field("POS")).any()          # and the noisy env did move differently
    plain.close(); noisy.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    """perturb_init_state_prob = 0.0 and tar_obs_noise = None written out: the bytes of an env built without the kwargs (observations,
    rewards, done flags, records) over reset + 20 steps.  orr_set_task_noise(NULL) on a handle that ran with noise: from the next reset
    on, the bytes of a handle that never had any (records and counters copied over first: the noisy steps ended other episodes)."""
    import torch
    L = _lib.load()
    n = 70
    kw = dict(mode="train", enable_randomizer=True)
    a, b = make_env(n, **kw), make_env(n, perturb_init_state_prob=0.0, tar_obs_noise=None, **kw)
    c = make_env(n, perturb_init_state_prob=0.5, tar_obs_noise=0.1, **kw)
    rng = np.random.RandomState(4)
    oc = c.reset()
    for k in range(5):
        oc = c.step(stress(c, oc, rng))[0]
    oa, ob = a.reset(), b.reset()
    assert not torch.equal(c.state.view(torch.int32), a.state.view(torch.int32))

    def run20(envs, obs):
        for k in range(20):
            act = torch.from_numpy(rng.uniform(-0.3, 0.3, (n, 12)).astype(np.float32)).to(a.device)
            outs = [e.step(act) for e in envs]
            for o in outs[1:]:
                assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) and torch.equal(outs[0][2], o[2]), k
            for e in envs[1:]:
                assert torch.equal(envs[0].state.view(torch.int32), e.state.view(torch.int32)), k
    assert torch.equal(oa, ob) and torch.equal(a.state.view(torch.int32), b.state.view(torch.int32))
    run20([a, b], None)
    assert L.orr_set_task_noise(c.h, None) == 0
    c.load_state_dict(a.state_dict())
    oa, oc = a.reset(), c.reset()
    assert torch.equal(oa, oc) and torch.equal(a.state.view(torch.int32), c.state.view(torch.int32))
    run20([a, c], None)
    for e in (a, b, c):
        e.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_more_waves_than_simds():
    """4100 robots = 1025 waves: more than the device has SIMDs, where the default path picks the two-wave kernel; the noise variant runs
    one wave per SIMD at any batch size.  prob = 1: every robot is perturbed as predicted; reset + 3 steps leave nothing non-finite."""
    import torch
    L = ol.lib()
    n = 4100
    env = make_env(n, perturb_init_state_prob=1.0, tar_obs_noise=0.1)
    obs = env.reset()
    a, b = check_reset_states(L, env, rigid(env), np.arange(n), 1.0, "reset()")
    assert (a, b) == (n, 0)
    rng = np.random.RandomState(5)
    for k in range(3):
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
    assert bool(torch.isfinite(env.state[:, 0:37]).all())
    assert int(env.field_int("EPISODE_IDX").min()) >= 1 and int(env.counters[_abi.CNT_TOTAL_TIMESTEPS]) == 3 * n
    env.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Each invalid struct fails and orr_last_error() names the field; the handle then steps as an untouched twin does.  Friction anchors:
    orr_set_task_noise refuses them on the handle, and an anchor model set on a noisy handle makes the launches fail and launch nothing."""
    import torch
    L = _lib.load()
    env, twin = make_env(8, perturb_init_state_prob=0.5, tar_obs_noise=0.1), make_env(8, perturb_init_state_prob=0.5, tar_obs_noise=0.1)
    nan, inf = float("nan"), float("inf")
    fields = [f[0] for f in _abi.OrrTaskNoise._fields_]
    for name in fields:
        for bad in ((nan, -0.1, 1.5, inf) if name == "perturb_init_state_prob" else (nan, -0.1, inf)):
            s = envmod.task_noise_spec(0.5, 0.1)
            setattr(s, name, bad)
            assert L.orr_set_task_noise(env.h, C.byref(s)) == -1, (name, bad)
            assert name.encode() in L.orr_last_error(), (name, bad, L.orr_last_error())
    oe, ot = env.reset(), twin.reset()
    assert torch.equal(oe, ot)
    act = torch.zeros(8, 12, device=env.device)
    for k in range(10):
        env.step(act); twin.step(act)
    assert torch.equal(env.state.view(torch.int32), twin.state.view(torch.int32)) and torch.equal(env.obs, twin.obs)
    assert (env.field("POS") != env.field("REF_POSE")[:, 0:3]).any()
    twin.close()
    # friction anchors on the handle: the setter refuses, the env constructor reports it
    with pytest.raises(RuntimeError, match="friction anchors"):
        make_env(8, perturb_init_state_prob=0.5, model_overrides={"laikago": {"friction_anchor": 1}})
    quiet = make_env(8, model_overrides={"laikago": {"friction_anchor": 1}})           # all-off noise on an anchor handle is fine
    assert L.orr_set_task_noise(quiet.h, C.byref(envmod.task_noise_spec())) == 0 and L.orr_set_task_noise(quiet.h, None) == 0
    assert L.orr_set_task_noise(quiet.h, C.byref(envmod.task_noise_spec(0.0, 0.1))) == -1 and b"friction anchors" in L.orr_last_error()
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
