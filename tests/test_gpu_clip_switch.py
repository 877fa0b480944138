"""Mid-episode clip switching on the MI355X (orr_set_clip_switch; ImitationTask's clip_time_min / clip_time_max): the multi-clip variant
of the step kernel switches a robot to a newly drawn clip of its set whenever its motion time reaches the record's CLIP_CHANGE_TIME.
Every draw is keyed by the episode's Philox stream, so the host predicts each switch exactly from orc_uniform (env.clip_switch_draws,
env.clip_change_time); the CPU oracle never switches, so it checks everything downstream of a switch from the GPU's post-switch record."""
import json
import math
import os

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, motion, robots, state as statemod
from openroborl_amd.env import CLIP_CHANGE_DRAW, CLIP_DRAW, clip_change_time, clip_draw_index, clip_switch_draws
from tests import oracle_lib as ol
from tests.gpu_kit import make_env, stress

pytestmark = pytest.mark.gpu

WARMUP = 0.25     # run.py:58-64 warmup_time (orr_config::warmup_time)


def clamped_sidesteps(tmp_path):
    """laikago_sidesteps with "LoopMode": "Clamp" (every shipped clip wraps): a clip whose end is a MOTION_OVER termination."""
    with open(os.path.join(motion.DATA_DIR, "laikago_sidesteps.txt")) as f:
        clip = json.load(f)
    assert clip["LoopMode"] == "Wrap"
    clip["LoopMode"] = "Clamp"
    dst = os.path.join(str(tmp_path), "laikago_sidesteps_clamp.txt")
    with open(dst, "w") as f:
        json.dump(clip, f)
    return dst


def set4(tmp_path):
    return ["laikago_pace", "laikago_trot", "laikago_spin", clamped_sidesteps(tmp_path)]


def rec(env):
    """The record fields the prediction needs (host copies)."""
    fi = lambda k: env.field_int(k)[:, 0].cpu().numpy().astype(np.int64)
    ff = lambda k: env.field(k)[:, 0].cpu().numpy()
    return dict(clip=fi("CLIP_ID"), change=ff("CLIP_CHANGE_TIME"), ep_step=fi("EP_STEP"), ep=fi("EPISODE_IDX"), index=fi("ROBOT_INDEX"),
                offset=ff("TIME_OFFSET"), counter=fi("STATE_ACTION_COUNTER"), warm=fi("WARMUP"))


def motion_time(env, r, counter):
    return counter * 0.001 + r["offset"].astype(np.float64) - WARMUP * r["warm"]     # sim_dt 0.001: dec7 in the kernel, exact decimal


def test_switches_follow_the_host_prediction(tmp_path):
    """4096 robots, set {pace, trot, spin, clamped sidesteps}, 0.3 .. 0.8 s, 300 steps with auto-reset: CLIP_ID, CLIP_CHANGE_TIME and
    TIME_OFFSET after every step are what orc_uniform and the documented draw rule give - a switch exactly where t >= CLIP_CHANGE_TIME
    (old offset), a new episode's first change time at every reset."""
    L = ol.lib()
    env = make_env(4096, set4(tmp_path), clip_time_min=0.3, clip_time_max=0.8)
    assert env.clip_switch == {"laikago": (0.3, 0.8)}
    tmin, tmax = float(np.float32(0.3)), float(np.float32(0.8))
    ids = env.clip_sets["laikago"]
    durs = [np.float32(float(env.clips[i].frame_duration) * (env.clips[i].num_frames - 1)) for i in ids]
    seed = int(env.cfg.seed)
    u = lambda i, ep, d: L.orc_uniform(seed, int(i), int(ep), int(d))
    obs = env.reset()
    r = rec(env)
    t0 = motion_time(env, r, r["counter"])
    for i in range(env.num_robot):                       # the first change time of every episode: draw 29 of the reset
        assert r["change"][i] == clip_change_time(t0[i], tmin, tmax, u(r["index"][i], r["ep"][i], CLIP_CHANGE_DRAW)), i
    rng = np.random.RandomState(0)
    switches = same = warm = over = 0
    for k in range(300):
        pre = rec(env)
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        post = rec(env)
        dn = done.cpu().numpy().astype(bool)
        t = motion_time(env, pre, pre["counter"] + 33)   # the old offset's motion time of this step
        sw = t >= pre["change"].astype(np.float64)
        tie = np.abs(t - pre["change"]) < 1e-12             # a decision the last bit of the float64 time could flip: not judged
        sw &= ~tie
        reasons = env.field_int("DONE_REASON")[:, 0].cpu().numpy()
        for i in np.nonzero(sw)[0]:
            d0, d1, d2 = clip_switch_draws(pre["ep_step"][i])
            m = int(round(u(pre["index"][i], pre["ep"][i], d0) * (1 << 24)))
            new = ids[int(clip_draw_index(m, len(ids)))]
            switches += 1
            same += new == pre["clip"][i]
            warm += bool(pre["warm"][i])
            if dn[i]:
                over += bool(reasons[i] & _abi.DONE_MOTION_OVER) and new == 3
                continue                                   # the auto-reset overwrote the record: checked below as a reset
            assert post["clip"][i] == new, (k, i)
            assert post["change"][i] == clip_change_time(t[i], tmin, tmax, u(pre["index"][i], pre["ep"][i], d1)), (k, i)
            assert post["offset"][i] == np.float32(u(pre["index"][i], pre["ep"][i], d2)) * durs[new], (k, i)
        keep = ~sw & ~dn & ~tie
        np.testing.assert_array_equal(post["clip"][keep], pre["clip"][keep])
        np.testing.assert_array_equal(post["change"][keep], pre["change"][keep])
        np.testing.assert_array_equal(post["offset"][keep], pre["offset"][keep])
        t0 = motion_time(env, post, post["counter"])
        for i in np.nonzero(dn)[0]:
            m = int(round(u(post["index"][i], post["ep"][i], CLIP_DRAW) * (1 << 24)))
            assert post["clip"][i] == ids[int(clip_draw_index(m, len(ids)))], (k, i)
            assert post["change"][i] == clip_change_time(t0[i], tmin, tmax, u(post["index"][i], post["ep"][i], CLIP_CHANGE_DRAW)), (k, i)
    print("CLIP_SWITCH %d switches (%d to the same clip, %d in warm-up episodes, %d onto the clamped clip ending it at once)" %
          (switches, same, warm, over))
    assert switches > 10 * 4096 and same > 0 and warm > 0 and over > 0
    env.close()


def test_oracle_follows_from_the_post_switch_record(tmp_path):
    """256 robots: after a step in which robots switched, the GPU record goes into the oracle, and both step on until the next switch
    (the oracle has no switching: it runs the new clip at the new offset and origin the GPU set), three steps at most."""
    n = 256
    env = make_env(n, set4(tmp_path), clip_time_min=0.3, clip_time_max=0.8, auto_reset=False)
    rng = np.random.RandomState(2)
    obs = env.reset()
    checked = 0
    for k in range(60):
        pre = rec(env)
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        post = rec(env)
        switched = post["clip"] != pre["clip"]
        if switched.sum() < 8:
            continue
        orc = ol.OracleEnv(env.cfg, env.models, env.clips, n, robot_type=env.robot_type, clip_id=post["clip"], threads=8)
        orc.state[:] = statemod.to_float64(env.layout, env.state.detach().cpu().numpy())
        alive = switched.copy()
        for j in range(3):
            a = stress(env, obs, rng)
            r0 = rec(env)
            og, rg, dg, _ = env.step(a)
            oo, ro, do = orc.step(a.cpu().numpy().astype(np.float64))
            t = motion_time(env, r0, r0["counter"] + 33)
            alive &= ~(t >= r0["change"].astype(np.float64)) & ~dg.cpu().numpy().astype(bool) & ~do.astype(bool)
            if not alive.any():
                break
            g = statemod.to_float64(env.layout, env.state.detach().cpu().numpy())
            for name in ("CLIP_ID", "TIME_OFFSET", "ORIGIN_ROT"):
                np.testing.assert_array_equal(g[alive][:, env.layout.sl(name)], orc.state[alive][:, env.layout.sl(name)], err_msg=name)
            atol_obs = 5e-4 * (j + 1)
            np.testing.assert_allclose(og.cpu().numpy()[alive][:, 84:], oo[alive][:, 84:], atol=atol_obs, err_msg="target frames, step %d" % j)
            np.testing.assert_allclose(rg.cpu().numpy()[alive], ro[alive], atol=3e-3 * (j + 1), err_msg="reward, step %d" % j)
            np.testing.assert_allclose(g[alive][:, env.layout.sl("ORIGIN_POS")], orc.state[alive][:, env.layout.sl("ORIGIN_POS")], atol=2e-3 * (j + 1))
            checked += int(alive.sum())
        orc.close()
        if checked > 100:
            break
    assert checked > 100
    env.close()


def test_explicit_inf_is_bitwise_the_default(tmp_path):
    import torch
    files = set4(tmp_path)
    a = make_env(256, files, mode="train", enable_randomizer=True)
    b = make_env(256, files, mode="train", enable_randomizer=True, clip_time_min=math.inf, clip_time_max=math.inf)
    assert b.clip_switch == {"laikago": (math.inf, math.inf)}
    oa, ob = a.reset(), b.reset()
    rng = np.random.RandomState(4)
    for k in range(40):
        act = torch.from_numpy(rng.uniform(-0.3, 0.3, (256, 12)).astype(np.float32)).to(a.device)
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
    assert torch.equal(a.state.view(torch.int32), b.state.view(torch.int32))
    assert torch.isinf(a.field("CLIP_CHANGE_TIME")).all()
    a.close(); b.close()


def test_graph_rollout_equals_the_eager_steps_with_switching(tmp_path):
    import torch
    from openroborl_amd import ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = torch.device("cuda:0")
    n, T = 256, 16
    envs = [VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev,
                            motion_file=set4(tmp_path), clip_time_min=0.1, clip_time_max=0.3) for _ in range(2)]
    models = [ppo.ActorCritic(dev, seed=1).enable_fused() for _ in range(2)]
    collector = rollout.GraphRollout(envs[1], models[1], T)
    obs = [e.reset() for e in envs]
    gen = torch.Generator(device=dev).manual_seed(0)
    switched = 0
    for seg in range(4):
        before = envs[1].active_clip_ids()
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        a = rollout.collect_rollout(envs[0], models[0], T, obs=obs[0], noise=noise)
        b = collector.collect(obs[1], noise=noise)
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs"):
            assert torch.equal(a[k], b[k]), (seg, k)
        switched += int((envs[1].active_clip_ids() != before).sum())
        obs = [a["last_obs"], b["last_obs"]]
        assert torch.equal(envs[0].state.view(torch.int32), envs[1].state.view(torch.int32)), seg
    assert collector.graph is not None and switched > n
    for e in envs:
        e.close()


def test_abi_refusals(tmp_path):
    """orr_set_clip_switch refuses NaN, negative values, tmin > tmax, exactly one infinite bound and friction anchors; a refused call
    changes nothing (the type keeps its interval: the next steps are those of an untouched twin)."""
    import torch
    L = _lib.load()
    env = make_env(8, set4(tmp_path), clip_time_min=0.3, clip_time_max=0.8)
    twin = make_env(8, set4(tmp_path), clip_time_min=0.3, clip_time_max=0.8)
    t = robots.ROBOT_TYPE_ID["laikago"]
    inf, nan = float("inf"), float("nan")
    for lo, hi in ((nan, 1.0), (0.1, nan), (-0.1, 1.0), (0.5, 0.4), (0.3, inf), (inf, 0.3), (-inf, -inf)):
        assert L.orr_set_clip_switch(env.h, t, lo, hi) == -1, (lo, hi)
    assert L.orr_set_clip_switch(env.h, _abi.MAX_ROBOT_TYPES, 0.1, 0.2) == -1
    assert L.orr_set_clip_switch(env.h, -1, 0.1, 0.2) == -1
    assert L.orr_set_clip_switch(env.h, t, 0.0, 0.0) == 0 and L.orr_set_clip_switch(env.h, t, 0.3, 0.8) == 0   # accepted (tmin = tmax = 0 too)
    for e in (env, twin):
        e.reset()
    act = torch.zeros(8, 12, device=env.device)
    for k in range(40):
        env.step(act); twin.step(act)
    assert torch.equal(env.state.view(torch.int32), twin.state.view(torch.int32))
    env.close(); twin.close()
    # friction anchors: the setter refuses a finite interval, the env constructor reports it
    with pytest.raises(RuntimeError, match="friction anchors"):
        make_env(8, set4(tmp_path), clip_time_min=0.3, clip_time_max=0.8, model_overrides={"laikago": {"friction_anchor": 1}})
    # a one-clip set is accepted and never switches: bitwise the run without an interval
    one = make_env(8, "laikago_pace", clip_time_min=0.05, clip_time_max=0.1)
    ref = make_env(8, "laikago_pace")
    for e in (one, ref):
        e.reset()
    for k in range(30):
        one.step(act); ref.step(act)
    assert torch.equal(one.state.view(torch.int32), ref.state.view(torch.int32))
    one.close(); ref.close()


def test_switching_off_on_a_running_handle_stops_at_once(tmp_path):
    """orr_set_clip_switch(+inf, +inf) after some steps: the records keep finite change times, but no step switches any more."""
    import torch
    env = make_env(64, set4(tmp_path), clip_time_min=0.1, clip_time_max=0.2, auto_reset=False)
    obs = env.reset()
    rng = np.random.RandomState(6)
    for k in range(10):
        obs, _, _, _ = env.step(stress(env, obs, rng))
    assert _lib.load().orr_set_clip_switch(env.h, robots.ROBOT_TYPE_ID["laikago"], math.inf, math.inf) == 0
    before = rec(env)
    assert np.isfinite(before["change"]).all()
    for k in range(20):
        obs, _, _, _ = env.step(stress(env, obs, rng))
    after = rec(env)
    np.testing.assert_array_equal(after["clip"], before["clip"])
    np.testing.assert_array_equal(after["offset"], before["offset"])
    np.testing.assert_array_equal(after["change"], before["change"])
    del torch
    env.close()


GOLDEN = "task_laikago_clipswitch.npz"


def clamped_backwards_trot(tmp_path):
    """The fourth clip of the golden fixture (tests/golden/make_golden_clip_switch.py): backwards_trot with "LoopMode": "Clamp"."""
    with open(os.path.join(motion.DATA_DIR, "laikago_backwards_trot.txt")) as f:
        clip = json.load(f)
    clip["LoopMode"] = "Clamp"
    dst = os.path.join(str(tmp_path), "laikago_backwards_trot_clamp.txt")
    with open(dst, "w") as f:
        json.dump(clip, f)
    return dst


def test_hip_replay_reproduces_the_reference_switching(tmp_path):
    """tests/golden/task_laikago_clipswitch.npz - the reference's own WrapperEnv / ImitationTask with four clips and clip_time_min /
    clip_time_max, its draws taken from the device's Philox stream - replayed through orr_debug_replay_reset / _step (the multi-clip
    MODE 2 kernels): observations, reward and torques at test_gpu_golden_task.py's tolerances, and at every step the active clip, the
    switch steps, time offset, origin, PREV_PHASE, CLIP_CHANGE_TIME and the reference pose / velocity."""
    import torch
    from openroborl_amd.env import VecQuadrupedEnv
    g = np.load(os.path.join(ol.GOLDEN, GOLDEN))
    n = int(g["num_robot"])
    names = [str(x) for x in g["clip_names"]]
    files = names[:3] + [clamped_backwards_trot(tmp_path)]
    tmin, tmax = (float(x) for x in g["clip_time"])
    env = VecQuadrupedEnv(num_robot=n, robot=str(g["robot"]), motion_file=files, mode="train", enable_randomizer=bool(g["randomizer"]),
                          auto_reset=False, legacy_grid=True, seed=int(g["seed"]), clip_time_min=tmin, clip_time_max=tmax,
                          config_overrides=dict(ep_len_start=int(g["ep_start"]), ep_len_end=int(g["ep_end"]), curriculum_steps=int(g["curriculum_steps"])))
    dev = env.device
    m = env.models[int(env.robot_type[0])]
    jom = np.asarray(m["joint_of_motor"])
    mdir = np.asarray(m["motor_dir"])
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    F = lambda name: env.field(name).cpu().numpy()
    FI = lambda name: env.field_int(name)[:, 0].cpu().numpy()
    count, switches, worst = 0, 0, {"obs": 0.0, "tau": 0.0, "rew": 0.0}
    tau_out = torch.zeros((n, 33, 12), dtype=torch.float32, device=dev)
    for kind, idx in g["marks"]:
        idx = int(idx)
        if kind == 0.0:
            env.counters[_abi.CNT_TOTAL_STEP_COUNT] = count
            obs = env.replay_reset(f32(g["reset/uniforms"][idx])).cpu().numpy()
            R = lambda key: g["reset/" + key][idx]
            what = "reset %d " % idx
            np.testing.assert_array_equal(FI("CLIP_ID"), R("clip_id").astype(int), err_msg=what + "clip")
            np.testing.assert_allclose(obs, R("obs"), atol=2e-5, err_msg=what + "observation")
            np.testing.assert_array_equal(FI("WARMUP"), R("warmup").astype(int), err_msg=what + "warm-up flag")
            np.testing.assert_allclose(F("TIME_OFFSET")[:, 0], R("time_offset"), atol=1e-6, err_msg=what + "time offset")
            np.testing.assert_allclose(F("CLIP_CHANGE_TIME")[:, 0], R("clip_change_time"), atol=1e-6, err_msg=what + "change time")
            np.testing.assert_allclose(F("ORIGIN_POS"), R("origin_pos"), atol=2e-6, err_msg=what + "origin")
            np.testing.assert_allclose(F("ORIGIN_ROT"), R("origin_rot"), atol=2e-6, err_msg=what + "origin rotation")
            np.testing.assert_allclose(F("PREV_PHASE")[:, 0], R("prev_phase"), atol=1e-6, err_msg=what + "phase")
            np.testing.assert_allclose(F("REF_POSE"), R("ref_pose"), atol=5e-6, err_msg=what + "reference pose")
        else:
            S = lambda key: g["step/" + key][idx]
            change_pre = F("CLIP_CHANGE_TIME")[:, 0].copy()
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
            np.testing.assert_array_equal(FI("CLIP_ID"), S("clip_id").astype(int), err_msg=what + "clip")
            sw = S("switched").astype(bool)
            np.testing.assert_array_equal(F("CLIP_CHANGE_TIME")[:, 0] != change_pre, sw, err_msg=what + "switch steps")
            np.testing.assert_allclose(F("CLIP_CHANGE_TIME")[:, 0], S("clip_change_time"), atol=1e-6, err_msg=what + "change time")
            np.testing.assert_allclose(F("TIME_OFFSET")[:, 0], S("time_offset"), atol=1e-6, err_msg=what + "time offset")
            np.testing.assert_allclose(F("ORIGIN_ROT"), S("origin_rot"), atol=2e-6, err_msg=what + "origin rotation")
            np.testing.assert_allclose(F("ORIGIN_POS"), S("origin_pos"), atol=5e-6, err_msg=what + "origin")
            np.testing.assert_allclose(F("PREV_PHASE")[:, 0], S("prev_phase"), atol=1e-6, err_msg=what + "phase")
            np.testing.assert_allclose(F("REF_POSE"), S("ref_pose"), atol=1e-5, err_msg=what + "reference pose")
            np.testing.assert_allclose(F("REF_VEL"), S("ref_vel"), atol=1e-4, rtol=1e-5, err_msg=what + "reference velocity")
            switches += int(sw.sum())
            worst["tau"] = max(worst["tau"], float(np.abs(tau - ref_tau).max()))
            worst["obs"] = max(worst["obs"], float(np.abs(obs[:, 12:] - ro[:, 12:]).max()))
            worst["rew"] = max(worst["rew"], float(np.abs(rew - S("reward")).max()))
            if done.any():
                count += n     # wrapper_env.py:82-83
    print("GOLDEN_CLIPSWITCH %d switches, worst |d tau| %.2e  |d obs| %.2e  |d reward| %.2e" % (switches, worst["tau"], worst["obs"], worst["rew"]))
    assert switches >= 20
    env.close()
