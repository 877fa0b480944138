"""Weighted and failure-adaptive clip sampling on the MI355X (orr_set_clip_weights, orr_set_clip_curriculum, orr_clip_curriculum_update):
the clip draws of resets and mid-episode switches go by 24-bit thresholds in device memory, and one kernel turns the episode log into
per-clip scores, running scores and new thresholds.  Every draw is keyed by the episode's Philox stream, so the host predicts each one
from orc_uniform and the thresholds (env_draws.clip_draw_weighted), as tests/test_gpu_multiclip.py does for the uniform rule."""
import ctypes as C

import numpy as np
import pytest

from openroborl_amd import _abi, env_draws as ed, robots
from openroborl_amd.env import CLIP_DRAW, clip_draw_index, clip_switch_draws
from tests import gpu_kit, oracle_lib as ol
from tests.test_gpu_clip_switch import motion_time, rec

pytestmark = pytest.mark.gpu

SET4 = ["laikago_pace", "laikago_trot", "laikago_spin", "laikago_sidesteps"]
TYPE_NAME = {v: k for k, v in robots.ROBOT_TYPE_ID.items()}
LAI, MINI = robots.ROBOT_TYPE_ID["laikago"], robots.ROBOT_TYPE_ID["mini_cheetah"]
ONE = 1 << 24
REF = [600.0, 300.0, 450.0, 200.0]       # the curriculum's per-clip refs of the update tests


def make_env(n, motion_file=SET4, **kw):
    return gpu_kit.make_env(n, motion_file, **{"auto_reset": False, "seed": 3, **kw})


def draw_int(env, index, episode, draw):
    return int(round(ol.lib().orc_uniform(int(env.cfg.seed), int(index), int(episode), int(draw)) * ONE))


def predicted_clips(env, thresholds=None):
    """The clip each robot's NEXT reset draws under `thresholds` ({robot name: cum}; None: the uniform rule (m n) >> 24)."""
    idx = env.field_int("ROBOT_INDEX")[:, 0].cpu().numpy()
    ep = env.field_int("EPISODE_IDX")[:, 0].cpu().numpy() + 1
    out = np.empty(env.num_robot, dtype=np.int32)
    for i in range(env.num_robot):
        name = TYPE_NAME[int(env.robot_type[i])]
        s = env.clip_sets[name]
        m = draw_int(env, idx[i], ep[i], CLIP_DRAW)
        out[i] = s[int(clip_draw_index(m, len(s)) if thresholds is None else ed.clip_draw_weighted(m, thresholds[name]))]
    return out


def test_weighted_reset_draws():
    """256 Laikago robots, {pace, trot, spin, sidesteps} weighted (1, 0, 2.5, 0.5): the thresholds on the device are the host's, a full and
    a masked reset draw by them, trot never appears, and None brings the uniform rule back - all without a new kernel variant."""
    import torch
    w = [1.0, 0.0, 2.5, 0.5]
    env = make_env(256, clip_weights=w)
    gen = env.launch_params_generation
    th = env.clip_thresholds()
    np.testing.assert_array_equal(th["laikago"], ed.clip_thresholds(w))
    np.testing.assert_allclose(env.clip_probabilities()["laikago"], np.array(w) / 4.0, atol=2.0 ** -24, rtol=0)
    pred = predicted_clips(env, th)
    env.reset()
    got = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got, pred)
    assert set(got.tolist()) == {0, 2, 3}
    assert (got != predicted_clips_at(env, 1)).any()           # not what the uniform rule would have drawn
    mask = np.arange(256) % 2 == 0
    pred2 = predicted_clips(env, th)
    env.reset(torch.from_numpy(mask.astype(np.uint8)).to(env.device))
    got2 = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got2[mask], pred2[mask])
    np.testing.assert_array_equal(got2[~mask], got[~mask])
    assert (got2[mask] != got[mask]).any() and 1 not in set(got2.tolist())
    env.set_clip_weights(None)
    np.testing.assert_array_equal(env.clip_thresholds()["laikago"], ed.clip_thresholds_uniform(4))
    pred3 = predicted_clips(env)
    env.reset()
    got3 = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got3, pred3)
    assert set(got3.tolist()) == {0, 1, 2, 3}
    assert env.launch_params_generation == gen                  # the kernels read the table: nothing to re-capture
    env.close()


def predicted_clips_at(env, episode):
    """The uniform rule's clip of every robot for the given episode index"""
    idx = env.field_int("ROBOT_INDEX")[:, 0].cpu().numpy()
    s = env.clip_sets["laikago"]
    return np.array([s[int(clip_draw_index(draw_int(env, i, episode, CLIP_DRAW), len(s)))] for i in idx], dtype=np.int32)


def test_mixed_batch_draws_by_each_types_own_thresholds():
    """Laikago {pace, trot} weighted (1, 3) + mini-cheetah {minicheetah_trot}, interleaved in every wavefront."""
    env = make_env(64, [["laikago_pace", "laikago_trot"], "minicheetah_trot"], robot=None, mixed_robots=["laikago", "mini_cheetah"],
                   clip_weights={"laikago": [1.0, 3.0]})
    th = env.clip_thresholds()
    np.testing.assert_array_equal(th["laikago"], [0, ONE // 4, ONE])
    np.testing.assert_array_equal(th["mini_cheetah"], [0, ONE])
    pred = predicted_clips(env, th)
    env.reset()
    got = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got, pred)
    lai = env.robot_type == LAI
    assert set(got[lai].tolist()) == {0, 1} and set(got[~lai].tolist()) == {2}
    assert (got[lai] == 1).sum() > (got[lai] == 0).sum()
    env.close()


def test_mid_episode_switches_draw_by_the_weights():
    """64 robots, a switch every 0.1 .. 0.2 s, 30 steps, weights (0, 1, 1, 2): every switch (draw 32 + 4 s) and every reset inside the
    launches (draw 28) picks the thresholds' entry; pace is never switched to."""
    w = [0.0, 1.0, 1.0, 2.0]
    env = gpu_kit.make_env(64, SET4, clip_time_min=0.1, clip_time_max=0.2, clip_weights=w)
    cum = env.clip_thresholds()["laikago"]
    np.testing.assert_array_equal(cum, ed.clip_thresholds(w))
    ids = env.clip_sets["laikago"]
    obs = env.reset()
    assert 0 not in set(env.active_clip_ids().tolist())
    rng = np.random.RandomState(0)
    switches, resets, picked = 0, 0, set()
    for k in range(30):
        pre = rec(env)
        obs, rew, done, _ = env.step(gpu_kit.stress(env, obs, rng))
        post = rec(env)
        dn = done.cpu().numpy().astype(bool)
        t = motion_time(env, pre, pre["counter"] + 33)
        sw = t >= pre["change"].astype(np.float64)
        tie = np.abs(t - pre["change"]) < 1e-12                 # a decision the last bit of the float64 time could flip: not judged
        sw &= ~tie
        for i in np.nonzero(sw & ~dn)[0]:
            d0, _, _ = clip_switch_draws(pre["ep_step"][i])
            new = ids[int(ed.clip_draw_weighted(draw_int(env, pre["index"][i], pre["ep"][i], d0), cum))]
            assert post["clip"][i] == new, (k, i)
            switches += 1
            picked.add(new)
        keep = ~sw & ~dn & ~tie
        np.testing.assert_array_equal(post["clip"][keep], pre["clip"][keep])
        for i in np.nonzero(dn)[0]:
            assert post["clip"][i] == ids[int(ed.clip_draw_weighted(draw_int(env, post["index"][i], post["ep"][i], CLIP_DRAW), cum))], (k, i)
            resets += 1
        assert 0 not in set(post["clip"].tolist())
    print("CLIP_WEIGHTS %d switches, %d resets inside the launches" % (switches, resets))
    assert switches > 64 and picked == {1, 2, 3}
    env.close()


def test_auto_reset_in_train_mode_draws_by_the_weights():
    """64 robots, train mode, the 20-step time limit, seed 17: the resets inside the step launches draw by the thresholds."""
    import torch
    n = 64
    env = make_env(n, mode="train", enable_randomizer=True, auto_reset=True, seed=17, clip_weights=[1.0, 0.0, 2.5, 0.5])
    th = env.clip_thresholds()
    env.reset()
    limit = int(env.field_int("MAX_EP_STEPS").max())
    assert limit == 20
    rng = np.random.RandomState(1)
    ended, seen = 0, set()
    for k in range(limit + 1):
        clip_pre = env.active_clip_ids().cpu().numpy()
        pred_next = predicted_clips(env, th)
        a = rng.uniform(-0.05, 0.05, (n, 12)).astype(np.float32)
        _, _, dg, _ = env.step(torch.from_numpy(a).to(env.device))
        dgn = dg.cpu().numpy().astype(bool)
        clip_post = env.active_clip_ids().cpu().numpy()
        np.testing.assert_array_equal(clip_post[dgn], pred_next[dgn])
        np.testing.assert_array_equal(clip_post[~dgn], clip_pre[~dgn])
        ended += int(dgn.sum())
        seen |= set(clip_post[dgn].tolist())
    assert ended >= n and seen == {0, 2, 3}
    env.close()


# ---- the update kernel on logs written by the test -----------------------------------------------------------------------------------
def write_log(env, ret, length, clip, count=None):
    import torch
    k = len(ret)
    assert k <= env.ep_log.shape[0]
    if k:
        env.ep_log[:k, 0] = torch.from_numpy(np.asarray(ret, dtype=np.float32)).to(env.device)
        env.ep_log[:k, 1] = torch.from_numpy(np.asarray(length, dtype=np.float32)).to(env.device)
        env.clip_log[:k] = torch.from_numpy(np.asarray(clip, dtype=np.int32)).to(env.device)
    env.counters[_abi.CNT_EPISODES] = k if count is None else count


def metric_values(metric, ret, length):
    """the float32 metric of each row, as the kernel forms it"""
    ret, length = np.asarray(ret, dtype=np.float32), np.asarray(length, dtype=np.float32)
    if metric == "length":
        return length
    if metric == "return":
        return ret
    return ret / np.maximum(length, np.float32(1.0))


def random_rows(rng, k):
    """returns, lengths and clip ids: clips 0, 1, 3 of the set (2 gets no row), 7 (a valid id outside the set), and ids outside [0, 16)"""
    length = rng.randint(0, 700, k).astype(np.float32)
    ret = (length * rng.uniform(-0.1, 1.1, k)).astype(np.float32)
    clip = rng.choice([0, 1, 3, 7, -1, 16, 100, -2 ** 31], size=k, p=[0.3, 0.3, 0.2, 0.05, 0.05, 0.05, 0.025, 0.025]).astype(np.int32)
    return ret, length, clip


def check_update(env, ref, metric, ema_before, ret, length, clip, alpha, eps):
    """One update on the log as written: n_c exact, S_c within n_c units of the float64 prediction, ema and thresholds against
    clip_curriculum_step on the device's own (n_c, S_c).  -> (stats, thresholds, largest |S_c - prediction|)"""
    stats = env.clip_curriculum_update().cpu().numpy().copy()
    th = env.clip_thresholds()["laikago"]
    x = metric_values(metric, ret, length)
    worst = 0
    for c in range(_abi.MAX_CLIPS):
        rows = np.asarray(clip) == c
        n_c = int(rows.sum())
        S_pred = int(ed.clip_episode_score(x[rows], ref[c]).sum()) if n_c else 0
        assert stats[c, 0] == n_c, (c, stats[c, 0], n_c)
        assert stats[c, 1] == int(stats[c, 1]) and abs(int(stats[c, 1]) - S_pred) <= n_c, (c, stats[c, 1], S_pred, n_c)
        worst = max(worst, abs(int(stats[c, 1]) - S_pred))
        mean = stats[c, 1] / (65536.0 * n_c) if n_c else 0.0
        assert stats[c, 2] == mean, c
    ema, want = ed.clip_curriculum_step(ema_before, stats[:, 0], stats[:, 1], env.clip_sets, alpha, eps)
    np.testing.assert_allclose(stats[:, 3], ema, atol=1e-12, rtol=0)
    np.testing.assert_allclose(th, want["laikago"], atol=1, rtol=0)
    assert th[0] == 0 and th[-1] == ONE and (np.diff(th) >= 0).all()
    return stats, th, worst


@pytest.mark.parametrize("metric", _abi.CLIP_METRICS)
def test_update_kernel_on_logs_written_by_the_test(metric):
    """Row counts around the kernel's strides (64 lanes a wave, 1024 threads, four rows a thread and trip) with clip ids outside the
    set, a clip without rows, two updates in a row, the same rows shuffled, and an empty log.  S_c may differ from the float64
    prediction by one unit per episode (a quotient that differs in its last bit); observed on the MI355X: 0 for every metric."""
    alpha, eps = 0.3, 0.2
    ref = REF if metric != "step_reward" else [1.0, 0.5, 0.75, 0.25]
    cur = {"alpha": alpha, "eps": eps, "metric": metric, "ref": ref}
    env = make_env(8, ep_log_capacity=8192)
    rng = np.random.RandomState(_abi.CLIP_METRICS.index(metric))
    refs = list(ref) + [1.0] * (_abi.MAX_CLIPS - 4)            # the validator's value for the ids outside every set
    worst = 0
    for k in (0, 1, 63, 64, 65, 257, 5000):
        env.set_clip_curriculum(cur)                             # zeroes the running scores
        ret, length, clip = random_rows(rng, k)
        write_log(env, ret, length, clip)
        before = env.clip_thresholds()["laikago"]
        s1, th1, w = check_update(env, refs, metric, np.zeros(_abi.MAX_CLIPS), ret, length, clip, alpha, eps)
        worst = max(worst, w)
        assert s1[2, 0] == 0 and s1[2, 3] == 0.0                 # clip 2: no rows, its score stays
        if k == 0:
            np.testing.assert_array_equal(s1, 0.0)
            np.testing.assert_array_equal(th1, before)           # an empty log changes nothing
            continue
        assert int(env.counters[_abi.CNT_EPISODES]) == k         # the update clears nothing
        # a second update in a row, on new rows: the running scores carry over
        ret2, length2, clip2 = random_rows(rng, k)
        write_log(env, ret2, length2, clip2)
        s2, th2, w = check_update(env, refs, metric, s1[:, 3], ret2, length2, clip2, alpha, eps)
        worst = max(worst, w)
        # the same two logs, each in another order, from zeroed scores: bit-identical stats and thresholds
        env.set_clip_curriculum(cur)
        for (r, l, c), s_want, th_want in (((ret, length, clip), s1, th1), ((ret2, length2, clip2), s2, th2)):
            p = rng.permutation(k)
            write_log(env, r[p], l[p], c[p])
            s = env.clip_curriculum_update().cpu().numpy()
            assert s.tobytes() == s_want.tobytes(), k
            np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th_want)
    # an empty log after all that: scores and thresholds stay
    s_last = env.clip_curriculum_update().cpu().numpy().copy()
    th_last = env.clip_thresholds()["laikago"]
    write_log(env, [], [], [])
    s = env.clip_curriculum_update().cpu().numpy()
    np.testing.assert_array_equal(s[:, :3], 0.0)
    np.testing.assert_array_equal(s[:, 3], s_last[:, 3])
    np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th_last)
    print("CLIP_CURRICULUM %s: largest |S_c - float64 prediction| = %d" % (metric, worst))
    env.close()


def test_update_reads_no_row_beyond_the_logs_capacity():
    """Capacity 64, the counter at 100 (36 episodes were dropped): the 64 rows count, nothing else."""
    env = make_env(8, ep_log_capacity=64)
    cur = {"alpha": 1.0, "eps": 0.0, "ref": REF}
    env.set_clip_curriculum(cur)
    rng = np.random.RandomState(5)
    length = rng.randint(1, 600, 64).astype(np.float32)
    clip = rng.randint(0, 4, 64).astype(np.int32)
    write_log(env, length, length, clip, count=100)
    s, th, _ = check_update(env, REF + [1.0] * 12, "length", np.zeros(_abi.MAX_CLIPS), length, length, clip, 1.0, 0.0)
    assert s[:, 0].sum() == 64
    env.close()


def test_draws_follow_the_thresholds_the_device_wrote():
    env = make_env(256)
    env.set_clip_curriculum({"alpha": 1.0, "eps": 0.1, "ref": 100.0})
    uniform = env.clip_thresholds()["laikago"]
    # pace mastered, trot half way, spin failing, sidesteps without episodes
    write_log(env, [0.0] * 6, [100.0, 100.0, 50.0, 50.0, 1.0, 1.0], [0, 0, 1, 1, 2, 2])
    stats = env.clip_curriculum_update().cpu().numpy()
    np.testing.assert_array_equal(stats[:3, 3], [1.0, 0.5, ed.clip_episode_score(1.0, 100.0) / 65536.0])
    th = env.clip_thresholds()
    assert (th["laikago"] != uniform).any() and (np.diff(th["laikago"]) > 0).all()
    p = env.clip_probabilities()["laikago"]
    assert abs(p.sum() - 1.0) < 1e-12 and p[0] < p[1] < p[2] < p[3]
    np.testing.assert_allclose(p[0], 0.025, atol=1e-6, rtol=0)               # f = 0: the uniform share eps / n alone
    pred = predicted_clips(env, th)
    env.reset()
    got = env.active_clip_ids().cpu().numpy()
    np.testing.assert_array_equal(got, pred)
    assert (got != predicted_clips_at(env, 1)).any()
    env.close()


def test_graph_rollout_with_the_curriculum_equals_the_eager_collector():
    """Twin envs of 256 robots, T = 8, four segments, the curriculum's update after each on both: the replayed graph draws by the
    thresholds the update wrote, without a new capture."""
    import torch
    from openroborl_amd import ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = torch.device("cuda:0")
    n, T = 256, 8
    envs = [VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev,
                            motion_file=SET4, clip_curriculum={"alpha": 0.5, "eps": 0.1, "ref": 20.0}) for _ in range(2)]
    models = [ppo.ActorCritic(dev, seed=1).enable_fused() for _ in range(2)]
    collector = rollout.GraphRollout(envs[1], models[1], T)
    obs = [e.reset() for e in envs]
    gen = torch.Generator(device=dev).manual_seed(0)
    uniform = ed.clip_thresholds_uniform(4)
    generation = envs[1].launch_params_generation
    graph, ended = None, 0
    for seg in range(4):
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        a = rollout.collect_rollout(envs[0], models[0], T, obs=obs[0], noise=noise)
        b = collector.collect(obs[1], noise=noise)
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs"):
            assert torch.equal(a[k], b[k]), (seg, k)
        ended += int(b["dones"].sum())
        obs = [a["last_obs"], b["last_obs"]]
        stats = [e.clip_curriculum_update().clone() for e in envs]
        assert torch.equal(stats[0], stats[1]), seg
        for e in envs:
            e.episode_log_device()                              # the clear between two updates
        if seg == 1:
            graph = collector.graph
            assert graph is not None
    assert collector.graph is graph and envs[1].launch_params_generation == generation
    assert ended >= n
    assert torch.equal(envs[0].state.view(torch.int32), envs[1].state.view(torch.int32))
    th = [e.clip_thresholds()["laikago"] for e in envs]
    np.testing.assert_array_equal(th[0], th[1])
    assert (th[1] != uniform).any()
    for e in envs:
        e.close()


def test_refused_calls_change_nothing():
    import torch
    env = make_env(8, clip_weights=[1.0, 2.0, 3.0, 4.0])
    L, h = env.L, env.h
    th0 = env.clip_thresholds()["laikago"]

    def weights(t, w, n=None):
        arr = (C.c_float * max(len(w), 1))(*w)
        return L.orr_set_clip_weights(h, t, arr, len(w) if n is None else n), L.orr_last_error().decode()
    for t, w, n, word in ((-1, [1] * 4, None, "robot_type"), (_abi.MAX_ROBOT_TYPES, [1] * 4, None, "robot_type"), (MINI, [1.0], None, "no clip set"),
                          (LAI, [1] * 3, None, "weights for"), (LAI, [1] * 5, None, "weights for"), (LAI, [1] * 4, 3, "weights for"),
                          (LAI, [1, -1, 1, 1], None, "finite"), (LAI, [1, float("nan"), 1, 1], None, "finite"),
                          (LAI, [1, float("inf"), 1, 1], None, "finite"), (LAI, [0, 0, 0, 0], None, "zero")):
        rc, msg = weights(t, w, n)
        assert rc < 0 and word in msg, (t, w, n, msg)
        np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th0)
    # the update without settings: nothing is launched, stats and thresholds stay
    stats = torch.full((_abi.MAX_CLIPS, 4), -7.0, dtype=torch.float64, device=env.device)
    write_log(env, [1.0] * 4, [100.0] * 4, [0, 1, 2, 3])
    assert L.orr_clip_curriculum_update(h, stats.data_ptr(), env._stream()) < 0 and "orr_set_clip_curriculum" in L.orr_last_error().decode()
    with pytest.raises(RuntimeError, match="orr_set_clip_curriculum"):
        env.clip_curriculum_update()
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all())
    np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th0)
    # settings: each refused argument leaves the settings and the running scores as they were
    env.set_clip_curriculum({"alpha": 0.5, "eps": 0.1, "ref": 100.0})
    write_log(env, [1.0] * 4, [100.0, 50.0, 25.0, 10.0], [0, 1, 2, 3])
    s0 = env.clip_curriculum_update().cpu().numpy().copy()
    th1 = env.clip_thresholds()["laikago"]
    assert (th1 != th0).any() and (s0[:4, 3] > 0).all()

    def curriculum(alpha=0.5, eps=0.1, metric=0, ref=None):
        c = _abi.OrrClipCurriculum(alpha=alpha, eps=eps, metric=metric)
        for i in range(_abi.MAX_CLIPS):
            c.ref[i] = 100.0 if ref is None or i not in ref else ref[i]
        return L.orr_set_clip_curriculum(h, C.byref(c)), L.orr_last_error().decode()
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(alpha=0.0), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=nan), "alpha"), (dict(alpha=-0.5), "alpha"),
                     (dict(eps=-0.1), "eps"), (dict(eps=1.1), "eps"), (dict(eps=nan), "eps"), (dict(metric=3), "metric"), (dict(metric=-1), "metric"),
                     (dict(ref={2: 0.0}), "ref[2]"), (dict(ref={0: -1.0}), "ref[0]"), (dict(ref={3: nan}), "ref[3]"), (dict(ref={1: inf}), "ref[1]")):
        rc, msg = curriculum(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert L.orr_set_clip_curriculum(h, None) < 0
    write_log(env, [], [], [])
    s1 = env.clip_curriculum_update().cpu().numpy()
    np.testing.assert_array_equal(s1[:, 3], s0[:, 3])            # the running scores were not zeroed
    np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th1)
    rc, msg = curriculum(ref={9: 0.0, 15: nan})                   # ids that occur in no set: not judged
    assert rc == 0, msg
    env.close()
    # no clip log (one clip): settings are accepted, the update is refused
    env = make_env(8, "laikago_pace")
    assert env.clip_log is None
    env.set_clip_curriculum({"alpha": 0.5, "eps": 0.1, "ref": 100.0})
    th0 = env.clip_thresholds()["laikago"]
    np.testing.assert_array_equal(th0, [0, ONE])
    with pytest.raises(RuntimeError, match="clip log"):
        env.clip_curriculum_update()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(env.clip_stats.cpu().numpy(), 0.0)
    np.testing.assert_array_equal(env.clip_thresholds()["laikago"], th0)
    env.close()
