"""Clip sets on the MI355X (orr_set_clip_set, the multi-clip variants of the step and reset kernels): every reset draws the episode's clip
from the robot type's set with draw 28 of the episode's Philox stream, k = (m n) >> 24.  The CPU oracle honours a per-robot CLIP_ID, so
every parity check presets it with the clip the prediction (orc_uniform + the same integer rule) says the device drew."""
import collections
import ctypes as C

import numpy as np
import pytest

from openroborl_amd import _abi, robots
from openroborl_amd.env import CLIP_DRAW, clip_draw_index
from tests import gpu_kit, oracle_lib as ol
from tests.gpu_kit import gpu_state64

pytestmark = pytest.mark.gpu

SET4 = ["laikago_pace", "laikago_trot", "laikago_spin", "laikago_sidesteps"]
TYPE_NAME = {v: k for k, v in robots.ROBOT_TYPE_ID.items()}


def make_env(n, motion_file, **kw):
    return gpu_kit.make_env(n, motion_file, **{"auto_reset": False, "seed": 3, **kw})


def predicted_clips(env):
    """The clip each robot's NEXT reset draws: episode = EPISODE_IDX + 1 of the record, key = (seed, ROBOT_INDEX)."""
    L = ol.lib()
    idx = env.field_int("ROBOT_INDEX")[:, 0].cpu().numpy()
    ep = env.field_int("EPISODE_IDX")[:, 0].cpu().numpy() + 1
    out = np.empty(env.num_robot, dtype=np.int32)
    for i in range(env.num_robot):
        s = env.clip_sets[TYPE_NAME[int(env.robot_type[i])]]
        m = int(round(L.orc_uniform(int(env.cfg.seed), int(idx[i]), int(ep[i]), CLIP_DRAW) * (1 << 24)))
        out[i] = s[int(clip_draw_index(m, len(s)))]
    return out


def oracle_for(env, clip_id):
    return ol.OracleEnv(env.cfg, env.models, env.clips, env.num_robot, robot_type=env.robot_type, clip_id=clip_id, threads=8)


def test_reset_draws_the_predicted_clip():
    """256 Laikago robots, set {pace, trot, spin, sidesteps}: the full reset and a masked reset of half of them."""
    import torch
    env = make_env(256, SET4)
    assert env.clip_sets == {"laikago": [0, 1, 2, 3]} and env.multi_clip
    pred = predicted_clips(env)
    env.reset()
    got = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got, pred)
    assert set(got.tolist()) == {0, 1, 2, 3}
    assert (env.field_int("EPISODE_IDX")[:, 0].cpu().numpy() == 1).all()
    mask = np.arange(256) % 2 == 0
    pred2 = predicted_clips(env)
    env.reset(torch.from_numpy(mask.astype(np.uint8)).to(env.device))
    got2 = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got2[mask], pred2[mask])
    np.testing.assert_array_equal(got2[~mask], got[~mask])
    assert (got2[mask] != got[mask]).any()                 # a new draw, not the old clip
    env.close()


def _reset_and_step_parity(env):
    import torch
    n = env.num_robot
    pred = predicted_clips(env)
    orc = oracle_for(env, pred)
    og = env.reset().cpu().numpy()
    oo = orc.reset()
    np.testing.assert_array_equal(env.active_clip_ids().cpu().numpy(), orc.field("CLIP_ID")[:, 0].astype(np.int32))
    np.testing.assert_allclose(og, oo, atol=2e-6)
    orc.state[:] = gpu_state64(env)
    a = np.random.RandomState(1).uniform(-0.2, 0.2, (n, 12)).astype(np.float32)
    og, rg, dg, _ = env.step(torch.from_numpy(a).to(env.device))
    oo, ro, do = orc.step(a.astype(np.float64))
    np.testing.assert_allclose(rg.cpu().numpy(), ro, atol=3e-3)
    np.testing.assert_allclose(og.cpu().numpy()[:, 84:], oo[:, 84:], atol=5e-4)
    orc.close()
    return pred


def test_reset_and_step_match_the_oracle():
    env = make_env(64, SET4)
    pred = _reset_and_step_parity(env)
    assert len(set(pred.tolist())) == 4
    env.close()


def test_mixed_batch_draws_from_each_types_own_set():
    """Laikago {pace, trot} + mini-cheetah {minicheetah_trot}, interleaved in every wavefront."""
    env = make_env(64, [["laikago_pace", "laikago_trot"], "minicheetah_trot"], robot=None, mixed_robots=["laikago", "mini_cheetah"])
    assert env.clip_sets == {"laikago": [0, 1], "mini_cheetah": [2]} and env.multi_clip
    pred = _reset_and_step_parity(env)
    lai = env.robot_type == robots.ROBOT_TYPE_ID["laikago"]
    assert set(pred[lai].tolist()) == {0, 1} and set(pred[~lai].tolist()) == {2}
    env.close()


def test_auto_reset_draws_the_next_clip_and_logs_the_ending_one():
    """Train mode, 20-step time limit: the reset inside the step launch draws the episode-2 clip, its fields match an oracle reset preset
    with that clip (the pattern of test_gpu_parity.test_auto_reset_inside_step_matches_oracle), and every episode-log row carries the clip
    of the episode that ENDED."""
    import torch
    n = 64
    env = make_env(n, SET4, mode="train", enable_randomizer=True, auto_reset=True, seed=17)
    orc = oracle_for(env, predicted_clips(env))
    env.reset(); orc.reset()
    np.testing.assert_array_equal(env.active_clip_ids().cpu().numpy(), orc.field("CLIP_ID")[:, 0].astype(np.int32))
    limit = int(env.field_int("MAX_EP_STEPS").max())
    assert limit == 20
    env.episode_log()                                   # empty
    rng = np.random.RandomState(1)
    clean = np.ones(n, dtype=bool)
    ended = []                                          # (return, length, clip) of every episode that ended, from the records
    checked = 0
    for k in range(limit + 1):
        g_pre = gpu_state64(env)
        clip_pre = env.active_clip_ids().cpu().numpy()
        pred_next = predicted_clips(env)
        a = rng.uniform(-0.05, 0.05, (n, 12)).astype(np.float32)
        og, rg, dg, _ = env.step(torch.from_numpy(a).to(env.device))
        dgn = dg.cpu().numpy().astype(bool)
        clip_post = env.active_clip_ids().cpu().numpy()
        np.testing.assert_array_equal(clip_post[dgn], pred_next[dgn])
        np.testing.assert_array_equal(clip_post[~dgn], clip_pre[~dgn])
        lr = env.field("LAST_EP_RETURN")[:, 0].cpu().numpy()
        ll = env.field_int("LAST_EP_LEN")[:, 0].cpu().numpy()
        ended += [(float(lr[i]), int(ll[i]), int(clip_pre[i])) for i in np.nonzero(dgn)[0]]
        if k == limit - 1:
            sel = clean & dgn
            assert sel.sum() > n // 2
            # the oracle resets the same robots from the same pre-step records, CLIP_ID preset with the predicted episode-2 clip: what a
            # reset produces depends only on the RNG stream and the clip, not on the physics of the step before it
            orc.state[:] = g_pre
            orc.field("CLIP_ID")[:, 0] = pred_next
            oo = orc.reset(mask=sel)
            g = gpu_state64(env)
            for name, tol in [(f, 0) for f in ("CLIP_ID", "EPISODE_IDX", "EP_STEP", "RING_LEN", "RING_HEAD", "STEP_COUNTER",
                                                "STATE_ACTION_COUNTER", "FILTER_VALID", "WARMUP", "MAX_EP_STEPS")] + \
                             [(f, 2e-5) for f in ("TIME_OFFSET", "LATENCY", "FOOT_MU", "KNEE_FRICTION", "MASS_RATIO", "INERTIA_RATIO",
                                                   "STRENGTH", "ORIGIN_POS", "ORIGIN_ROT", "REF_POSE", "REF_VEL", "POS", "QUAT", "Q", "QD",
                                                   "LINVEL", "ANGVEL")]:
                sl = env.layout.sl(name)
                np.testing.assert_allclose(g[sel][:, sl], orc.state[sel][:, sl], atol=tol, rtol=0, err_msg=name)
            np.testing.assert_allclose(og.cpu().numpy()[sel], oo[sel], atol=2e-4)
            assert len(set(pred_next[sel].tolist())) > 1
            checked = int(sel.sum())
        clean &= ~dgn
    assert checked > 0
    ret, length, clip = env.episode_log(with_clip=True)
    logged = sorted(zip(ret.cpu().numpy().tolist(), length.cpu().numpy().astype(int).tolist(), clip.cpu().numpy().tolist()))
    assert len(logged) == len(ended) >= checked
    assert logged == sorted(ended)
    env.close(); orc.close()


def test_variant_equals_the_default_kernel_bit_for_bit():
    """{pace, pace} (multi-clip variant: every reset draws one of two identical clips) against pace alone (the default kernel): 4096
    robots, train mode, randomiser on, 200 steps of the bench's stress actions with episodes ending and restarting inside the launches.
    Outputs and every state word but CLIP_ID must be identical: the variant adds the clip draw and nothing else."""
    import torch
    n, steps = 4096, 200
    kw = dict(mode="train", enable_randomizer=True, auto_reset=True, seed=5)
    envs = [make_env(n, ["laikago_pace", "laikago_pace"], **kw), make_env(n, "laikago_pace", **kw)]
    assert envs[0].multi_clip and not envs[1].multi_clip
    g = torch.Generator(device="cpu").manual_seed(0)
    obs = [e.reset() for e in envs]
    assert torch.equal(obs[0], obs[1])
    acts = [torch.empty(n, 12, device=e.device) for e in envs]
    n_done = 0
    for k in range(steps):
        noise = (torch.randn(n, 12, generator=g) * 0.125).to(envs[0].device)
        outs = []
        for e, o, a in zip(envs, obs, acts):
            e.stress_actions(o, noise, a)
            outs.append(e.step(a))
        assert torch.equal(outs[0][0], outs[1][0]), "observation, step %d" % k
        assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2]), "reward / done, step %d" % k
        n_done += int(outs[0][2].sum())
    assert n_done > n
    s0, s1 = envs[0].state.view(torch.int32).clone(), envs[1].state.view(torch.int32).clone()
    cid = envs[0].layout.sl("CLIP_ID")
    assert set(s0[:, cid].unique().tolist()) == {0, 1} and set(s1[:, cid].unique().tolist()) == {0}
    s0[:, cid] = 0
    assert torch.equal(s0, s1)
    for e in envs:
        e.close()


def test_clip_set_validation_and_anchor_refusal():
    import torch
    env = make_env(8, ["laikago_pace", "laikago_trot"])
    L, h = env.L, env.h

    def call(t, ids, n=None):
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        return L.orr_set_clip_set(h, t, arr, len(ids) if n is None else n), L.orr_last_error().decode()
    lai = robots.ROBOT_TYPE_ID["laikago"]
    for t, ids, n, word in ((-1, [0], None, "robot_type"), (_abi.MAX_ROBOT_TYPES, [0], None, "robot_type"), (lai, [0], 0, "clip set"),
                            (lai, [0] * 17, None, "clip set"), (lai, [0, 5], None, "not loaded"), (lai, [0, 16], None, "out of range"),
                            (lai, [-1], None, "out of range")):
        rc, msg = call(t, ids, n)
        assert rc != 0 and word in msg, (t, ids, n, msg)
    # nothing changed: the set is still {pace, trot} and the variant still runs
    pred = predicted_clips(env)
    env.reset()
    np.testing.assert_array_equal(env.active_clip_ids().cpu().numpy(), pred)
    with pytest.raises(ValueError):
        make_env(8, "laikago_pace").episode_log(with_clip=True)
    env.close()
    # friction anchors together with a clip set: refused with the message, nothing launched
    env = make_env(8, ["laikago_pace", "laikago_trot"], model_overrides={"laikago": {"friction_anchor": 1}})
    with pytest.raises(RuntimeError, match="friction anchors"):
        env.reset()
    with pytest.raises(RuntimeError, match="friction anchors"):
        env.step(torch.zeros(8, 12, device=env.device))
    torch.cuda.synchronize()
    assert float(env.obs.abs().max()) == 0.0
    env.close()


def test_graph_rollout_equals_the_eager_collector_with_a_clip_set():
    """rollout.GraphRollout against rollout.collect_rollout on twin clip-set envs: the replayed graph holds the multi-clip variant."""
    import torch
    from openroborl_amd import ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = torch.device("cuda:0")
    n, T = 256, 8
    envs = [VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev,
                            motion_file=SET4) for _ in range(2)]
    models = [ppo.ActorCritic(dev, seed=1).enable_fused() for _ in range(2)]
    collector = rollout.GraphRollout(envs[1], models[1], T)
    obs = [e.reset() for e in envs]
    gen = torch.Generator(device=dev).manual_seed(0)
    ended = 0
    for seg in range(4):
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        a = rollout.collect_rollout(envs[0], models[0], T, obs=obs[0], noise=noise)
        b = collector.collect(obs[1], noise=noise)
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs"):
            assert torch.equal(a[k], b[k]), (seg, k)
        ended += int(b["dones"].sum()) if seg >= 1 else 0
        obs = [a["last_obs"], b["last_obs"]]
    assert collector.graph is not None and ended >= n
    assert torch.equal(envs[0].state.view(torch.int32), envs[1].state.view(torch.int32))
    assert len(set(envs[1].active_clip_ids().tolist())) == 4
    for e in envs:
        e.close()


def test_two_shards_of_64_are_one_env_of_128_with_a_clip_set():
    """The pattern of test_gpu_shards.test_two_shards_of_64_are_one_env_of_128_bit_for_bit on a clip-set env: the clip draw is keyed by
    the GLOBAL robot index, so shards draw the clips the single env draws."""
    import torch
    from openroborl_amd.env import VecQuadrupedEnv
    from tests.test_gpu_shards import _run
    kw = dict(seed=11, robot="laikago", motion_file=SET4, mode="train", enable_randomizer=True, auto_reset=True)
    big = VecQuadrupedEnv(num_robot=128, **kw)
    a = VecQuadrupedEnv(num_robot=64, robot_index_offset=0, num_procs=2, **kw)
    b = VecQuadrupedEnv(num_robot=64, robot_index_offset=64, num_procs=2, **kw)
    f1, o1 = _run(torch, [big], [0], 128, 40)
    f2, o2 = _run(torch, [a, b], [0, 64], 128, 40)
    assert torch.equal(f1, f2)
    n_done = 0
    for k, ((ob1, r1, d1), (ob2, r2, d2)) in enumerate(zip(o1, o2)):
        assert torch.equal(ob1, ob2), "observation, step %d" % k
        assert torch.equal(r1, r2) and torch.equal(d1, d2), "reward / done, step %d" % k
        n_done += int(d1.sum())
    assert n_done >= 128
    assert torch.equal(big.state.view(torch.int32), torch.cat([a.state, b.state]).view(torch.int32))
    clips = collections.Counter(big.active_clip_ids().tolist())
    assert len(clips) == 4
    for e in (big, a, b):
        e.close()
