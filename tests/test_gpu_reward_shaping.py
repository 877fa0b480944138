"""Reward shaping on the device (orr_set_reward_shaping, orr_bind_reward_shaping, orr_shaped_reward; env.set_reward_shaping) against the
float64 reference and the counted bounds of tests/shaping_refs.py:
  1. the edge grid, no env step: the entry point called directly on crafted records and buffers;
  2. a live run against a twin without shaping: the step itself is untouched, every step's rows are the reference's;
  3. zero weights and no floor: the reward is the imitation reward bit for bit;
  4. a GraphRollout follows a change of the weights without a new capture;
  5. refusals on a live handle;
  6. train.py --reward-shaping in a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from openroborl_amd import _abi, _lib
from tests import gpu_kit as kit
from tests import shaping_refs as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
SPEC = dict(zip(sr.NAMES, sr.WEIGHTS), floor=-0.5)
ATTRS = ("shaping_out", "episode_shaping", "shaping_totals", "_shaping_prev")


def _up(env, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _own_buffers(env, guard=4):
    """rebind the four shaping buffers to the first N rows of larger ones whose `guard` rows behind stay sentinels"""
    import torch
    n = env.num_robot
    big = [torch.full((n + guard, cols), SENTINEL, dtype=torch.float32, device=env.device) for cols in (8, 8, 8, 24)]
    env._bind_outputs(env.L.orr_bind_reward_shaping, ATTRS, tuple(b[:n] for b in big))
    return big


def _call(env, inp, in_place=False):
    """one orr_shaped_reward on the env's handle with the record's integers and every buffer taken from inp -> out, the reward tensor"""
    import torch
    n = env.num_robot
    for name, key in (("EP_STEP", "ep_step"), ("LAST_EP_LEN", "last_len"), ("DONE_REASON", "reason")):
        env.field_int(name)[:, 0] = _up(env, inp[key])
    if inp["act"] is not None:
        env.actuator_out.copy_(_up(env, inp["act"]))
    if inp["contact"] is not None:
        env.contact_out.copy_(_up(env, inp["contact"]).view(n, 16))
    env.shaping_out.fill_(SENTINEL)
    env.episode_shaping.copy_(_up(env, inp["ep"]))
    env.shaping_totals.copy_(_up(env, inp["tot"]))
    env._shaping_prev.copy_(_up(env, inp["prev"]))
    env.set_reward_shaping(dict(zip(sr.NAMES, [float(x) for x in inp["w"]]), floor=float(inp["floor"])))
    actions, r_in, done = _up(env, inp["actions"]), _up(env, inp["reward"]), _up(env, inp["done"])
    r_out = r_in if in_place else torch.full((n,), SENTINEL, dtype=torch.float32, device=env.device)
    _lib.check(env.L.orr_shaped_reward(env.h, actions.data_ptr(), r_in.data_ptr(), done.data_ptr(), r_out.data_ptr(), env._stream()), env.L)
    torch.cuda.synchronize()
    assert in_place or np.array_equal(r_in.cpu().numpy(), inp["reward"]) and np.array_equal(actions.cpu().numpy(), inp["actions"], equal_nan=True)
    return _read(env, r_out)


def _read(env, reward):
    return dict(row=env.shaping_out.cpu().numpy(), ep=env.episode_shaping.cpu().numpy(), tot=env.shaping_totals.cpu().numpy(),
                prev=env._shaping_prev.cpu().numpy(), reward=reward.cpu().numpy())


# ---- 1. the edge grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_edge_grid_against_float64(n):
    env = kit.make_env(n, actuator_outputs=True, contact_outputs=True, reward_shaping=SPEC)
    big = _own_buffers(env)
    generation = env.launch_params_generation
    worst = {}
    for rnd in range(sr.rounds(n)):
        inp = sr.edge_inputs(n, rnd, seed=23, action_repeat=env.cfg.action_repeat, sim_dt=env.cfg.sim_dt)
        out = _call(env, inp, in_place=rnd % 3 == 2)
        for k, v in sr.check(inp, out, what="n=%d call %d: " % (n, rnd)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("n=%d largest error / bound: %s" % (n, worst))
    assert env.launch_params_generation == generation                 # a change of weights moves nothing a captured graph holds by value
    for b in big:                                                     # the padding lane groups stored nothing
        assert bool((b[n:] == SENTINEL).all())
    env.close()


def test_edge_grid_with_unbound_outputs():
    """no actuator and no contact outputs bound: terms 0, 1 and 4 are zero whatever the step left elsewhere"""
    n = 7
    env = kit.make_env(n, reward_shaping={"action_rate": 0.01, "action_accel": 0.005, "failure": 0.7})
    assert env.actuator_out is None and env.contact_out is None
    for rnd in range(4):
        inp = sr.edge_inputs(n, rnd, seed=29, action_repeat=env.cfg.action_repeat, sim_dt=env.cfg.sim_dt, bound=(False, False))
        inp["w"] = np.array([0.0, 0.0, 0.01, 0.005, 0.0, 0.7], dtype=np.float32)
        inp["floor"] = np.float32(sr.reference(dict(inp, floor=np.float32(-np.inf)))["row"][0, 6] + (0.25 if rnd % 2 == 0 else -0.25))
        out = _call(env, inp)
        sr.check(inp, out, what="call %d: " % rnd)
        assert not out["row"][:, [0, 1, 4]].any()
    env.close()


# ---- 2. a live run against a twin --------------------------------------------------------------------------------------------------------
ACTION_SEED = 7          # with it the run below meets its three conditions (asserted at its end)


def test_live_run_against_a_twin_without_shaping():
    import torch
    n, steps = 67, 40
    plain = kit.mixed_env(n, config_overrides=kit.short_episodes())
    env = kit.mixed_env(n, config_overrides=kit.short_episodes(), reward_shaping=SPEC)
    assert env.actuator_out is not None and env.contact_out is not None and env.imitation_reward is not None       # bound by the switch
    rng = np.random.default_rng(ACTION_SEED)
    wild = torch.arange(n, device=env.device) % 3 == 0
    obs_p, obs = plain.reset(), env.reset()
    assert torch.equal(obs_p, obs)
    w, floor = np.array(list(env.reward_shaping.w), dtype=np.float32), np.float32(env.reward_shaping.floor)
    inv_nsub, inv_dt = sr.host_scales(env.cfg.action_repeat, env.cfg.sim_dt)
    ep64, ep_b, tot64, tot_b = (np.zeros((n, 8)) for _ in range(4))
    seen = dict(failure=0, time_limit=0, third_step=0)
    for k in range(steps):
        actions = kit.stress(plain, obs_p, rng)
        actions[wild] = torch.from_numpy(rng.uniform(-2 * np.pi, 2 * np.pi, (n, 12)).astype(np.float32)).to(env.device)[wild]
        before = {key: getattr(env, attr).cpu().numpy() for key, attr in (("ep", "episode_shaping"), ("tot", "shaping_totals"), ("prev", "_shaping_prev"))}
        obs_p, rew_p, done_p, _ = plain.step(actions)
        obs, rew, done, _ = env.step(actions)
        torch.cuda.synchronize()
        assert torch.equal(obs_p.view(torch.int32), obs.view(torch.int32)) and torch.equal(done_p, done), k
        assert torch.equal(plain.state.view(torch.int32), env.state.view(torch.int32)), k
        assert torch.equal(env.imitation_reward.view(torch.int32), rew_p.view(torch.int32)), k
        inp = dict(act=env.actuator_out.cpu().numpy(), contact=env.contact_out.cpu().numpy().reshape(n, 4, 4), actions=actions.cpu().numpy(),
                   reward=env.imitation_reward.cpu().numpy(), done=done.cpu().numpy(), ep_step=env.field_int("EP_STEP")[:, 0].cpu().numpy(),
                   last_len=env.field_int("LAST_EP_LEN")[:, 0].cpu().numpy(), reason=env.field_int("DONE_REASON")[:, 0].cpu().numpy(),
                   w=w, floor=floor, inv_nsub=inv_nsub, inv_dt=inv_dt, **before)
        ref = sr.reference(inp)
        sr.check(inp, _read(env, rew), ref=ref, what="step %d: " % k)
        # the host's own float64 sums of the reference rows, with the bounds of the device's float32 adds
        d = inp["done"] != 0
        n_step = np.where(d, inp["last_len"], inp["ep_step"])
        over = (n_step <= 1)[:, None]
        ep64 = np.where(over, ref["row"], ep64 + ref["row"])
        ep_b = np.where(over, ref["row_b"], ep_b + ref["row_b"] + sr.EPS * (np.abs(ep64) + ep_b + ref["row_b"]))
        tot64 = np.where(d[:, None], tot64 + ep64, tot64)
        tot_b = np.where(d[:, None], tot_b + ep_b + sr.EPS * (np.abs(tot64) + tot_b + ep_b), tot_b)
        seen["failure"] += int((d & ((inp["reason"] & sr.FAIL_BITS) != 0)).sum())
        seen["time_limit"] += int((d & ((inp["reason"] & sr.FAIL_BITS) == 0) & ((inp["reason"] & sr.TIME_LIMIT) != 0)).sum())
        seen["third_step"] += int((n_step >= 3).sum())
    print("live run:", seen)
    # the episode logs are the same multiset of rows (the slots of one launch go by arrival)
    k_log = int(env.counters[_abi.CNT_EPISODES].item())
    assert k_log == int(plain.counters[_abi.CNT_EPISODES].item()) and k_log > 0
    rows = [e.ep_log[:k_log].cpu().numpy() for e in (plain, env)]
    assert all(np.array_equal(r[np.lexsort(r.T[::-1])].view(np.int32), rows[0][np.lexsort(rows[0].T[::-1])].view(np.int32)) for r in rows)
    # the means per step over the finished episodes
    stats = env.reward_shaping_stats()
    assert set(stats) == set(sr.NAMES) | {"shaped_reward"}
    steps_done = tot64[:, 7].sum()
    assert steps_done > 0 and float(env.shaping_totals[:, 7].double().sum()) == steps_done
    for c, name in enumerate(_abi.SHAPING_COLUMNS[:-1]):
        want, bound = tot64[:, c].sum() / steps_done, tot_b[:, c].sum() / steps_done
        print("%s: %.9g, float64 %.9g, bound %.3g" % (name, stats[name], want, bound))
        assert abs(stats[name] - want) <= bound + 4 * np.finfo(np.float64).eps * abs(want), name
    env.clear_shaping_totals()
    assert env.reward_shaping_stats() == {}
    assert seen["failure"] > 0 and seen["time_limit"] > 0 and seen["third_step"] > 0, seen
    plain.close()
    env.close()


# ---- 3. zero weights ----------------------------------------------------------------------------------------------------------------------
def test_zero_weights_and_no_floor_pass_the_imitation_reward():
    import torch
    n = 13
    env = kit.mixed_env(n, config_overrides=kit.short_episodes(), reward_shaping={})
    assert env.actuator_out is None and env.contact_out is None       # no weight needs them
    rng = np.random.default_rng(2)
    obs = env.reset()
    for k in range(12):
        obs, rew, done, _ = env.step(kit.stress(env, obs, rng))
        assert torch.equal(rew.view(torch.int32), env.imitation_reward.view(torch.int32)), k
        assert torch.equal(env.shaping_out[:, 6].view(torch.int32), rew.view(torch.int32)) and not bool(env.shaping_out[:, [0, 1, 4]].any())
    assert bool(rew.any())
    env.close()


def test_switching_off_restores_the_single_launch():
    import torch
    n = 9
    env = kit.make_env(n, reward_shaping=SPEC)
    rng = np.random.default_rng(3)
    obs = env.reset()
    g0 = env.launch_params_generation
    env.set_reward_shaping(dict(SPEC, failure=2.0))
    assert env.launch_params_generation == g0
    obs, rew, _, _ = env.step(kit.stress(env, obs, rng))
    env.set_reward_shaping(None)
    assert env.launch_params_generation > g0 and env.reward_shaping is None and env.shaping_out is None and env.imitation_reward is None
    assert env.reward_shaping_stats() == {}
    env.reward.fill_(SENTINEL)
    obs, rew, _, _ = env.step(kit.stress(env, obs, rng))
    assert rew.data_ptr() == env.reward.data_ptr() and bool((rew >= 0).all())           # orr_step wrote the caller's buffer itself
    err = env.L.orr_shaped_reward(env.h, obs.data_ptr(), rew.data_ptr(), env.done.data_ptr(), rew.data_ptr(), env._stream())
    assert err < 0 and env.L.orr_last_error().decode().startswith("orr_shaped_reward: reward shaping is not set")
    torch.cuda.synchronize()
    env.close()


# ---- 4. a captured rollout follows the weights -----------------------------------------------------------------------------------------------
def test_graph_rollout_follows_new_weights_without_a_capture():
    import torch
    from openroborl_amd import ppo, rollout
    n, T = 64, 4
    env = kit.mixed_env(n, config_overrides=kit.short_episodes(), reward_shaping=SPEC)
    model = ppo.ActorCritic(env.device, seed=1).enable_fused()
    collector = rollout.GraphRollout(env, model, T)
    gen = torch.Generator(device=env.device).manual_seed(0)
    obs = env.reset()
    for _ in range(2):
        buf = collector.collect(obs, generator=gen)
        obs = buf["last_obs"]
    graph, generation = collector.graph, env.launch_params_generation
    assert graph is not None

    def shaped_from_rows():
        s = env.reward_shaping      # the struct the env holds
        w = np.array(list(s.w), dtype=np.float64)
        rows = env.shaping_out.double().cpu().numpy()
        r = env.imitation_reward.double().cpu().numpy()
        pen = (rows[:, :6] * w).sum(1)
        return np.maximum(r - pen, float(s.floor)), 7.0 * sr.EPS * (np.abs(rows[:, :6]) * w).sum(1) + sr.EPS * np.abs(r - pen), pen

    torch.cuda.synchronize()
    got = buf["rewards"][T - 1].double().cpu().numpy()
    want, bound, _ = shaped_from_rows()
    assert (np.abs(got - want) <= bound).all()
    doubled = {k: (2.0 * v if k != "floor" else v) for k, v in SPEC.items()}
    env.set_reward_shaping(doubled)
    buf = collector.collect(obs, generator=gen)
    torch.cuda.synchronize()
    assert collector.graph is graph and env.launch_params_generation == generation
    got = buf["rewards"][T - 1].double().cpu().numpy()
    want, bound, pen = shaped_from_rows()
    print("graph: largest error / bound %.3g" % float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
    assert (np.abs(got - want) <= bound).all()
    # and it is not what the old weights give: half the penalty
    old = np.maximum(env.imitation_reward.double().cpu().numpy() - 0.5 * pen, SPEC["floor"])
    moved = np.abs(got - old) > 4 * bound
    assert moved.sum() > n // 2, int(moved.sum())
    env.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import torch
    n = 6
    env = kit.make_env(n, actuator_outputs=True, contact_outputs=True, reward_shaping=SPEC)
    L, h, stream = env.L, env.h, env._stream()
    big = _own_buffers(env, guard=1)
    actions = torch.zeros((n + 1, 12), dtype=torch.float32, device=env.device)
    rew = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=env.device)
    done = torch.zeros(n, dtype=torch.uint8, device=env.device)
    a, r, d = actions.data_ptr(), rew.data_ptr(), done.data_ptr()
    bufs = [b.data_ptr() for b in big]
    S = _abi.OrrRewardShaping

    def spec(w=(0.0,) * 6, floor=-np.inf):
        return C.byref(S((C.c_float * 6)(*w), floor))

    def refused(entry, rc, text=""):
        msg = L.orr_last_error().decode()
        assert rc < 0 and msg.startswith(entry + ": ") and text in msg, (entry, rc, msg)

    refused("orr_shaped_reward", L.orr_shaped_reward(h, None, r, d, r, stream), "null")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, None, d, r, stream), "null")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, None, r, stream), "null")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, None, stream), "null")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a + 4, r, d, r, stream), "16-byte")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r + 2, d, r, stream), "4-byte")
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, r + 1, stream), "4-byte")
    for k in range(6):
        for bad in (-1e-3, float("nan"), float("inf")):
            refused("orr_set_reward_shaping", L.orr_set_reward_shaping(h, spec(w=[bad if j == k else 0.1 for j in range(6)]), stream), "w[%d]" % k)
    for bad in (float("nan"), float("inf")):
        refused("orr_set_reward_shaping", L.orr_set_reward_shaping(h, spec(floor=bad), stream), "floor")
    for miss in (1, 2, 3):
        refused("orr_bind_reward_shaping", L.orr_bind_reward_shaping(h, *[None if j == miss else p for j, p in enumerate(bufs)]), "needs")
    for off in range(4):
        refused("orr_bind_reward_shaping", L.orr_bind_reward_shaping(h, *[p + 4 if j == off else p for j, p in enumerate(bufs)]), "16-byte")
    # every refused setter and bind left the handle as it was: the call still runs with the old weights and buffers
    inp = sr.edge_inputs(n, 1, seed=31, action_repeat=env.cfg.action_repeat, sim_dt=env.cfg.sim_dt)
    sr.check(inp, _call(env, inp))
    # a weight whose buffer is not bound is refused at the launch, and nothing is written
    for b in big:
        b.fill_(SENTINEL)
    env.bind_actuator_outputs(False)
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, r, stream), "actuator outputs")
    env.bind_actuator_outputs(True)
    env.bind_contact_outputs(False)
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, r, stream), "contact outputs")
    env.bind_contact_outputs(True)
    # unbound shaping buffers, then shaping off
    _lib.check(L.orr_bind_reward_shaping(h, None, None, None, None), L)
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, r, stream), "not bound")
    _lib.check(L.orr_bind_reward_shaping(h, *bufs), L)
    _lib.check(L.orr_set_reward_shaping(h, None, stream), L)
    refused("orr_shaped_reward", L.orr_shaped_reward(h, a, r, d, r, stream), "not set")
    torch.cuda.synchronize()
    assert bool((rew == SENTINEL).all()) and all(bool((b == SENTINEL).all()) for b in big)
    # a handle without a bound state
    h2 = C.c_void_p()
    _lib.check(L.orr_create(C.byref(env.cfg), C.byref(h2)), L)
    refused("orr_set_reward_shaping", L.orr_set_reward_shaping(h2, spec(), stream), "not bound")
    refused("orr_bind_reward_shaping", L.orr_bind_reward_shaping(h2, *bufs), "not bound")
    refused("orr_shaped_reward", L.orr_shaped_reward(h2, a, r, d, r, stream), "not bound")
    L.orr_destroy(h2)
    env.close()


def test_the_python_side_refuses_what_the_c_side_would():
    env = kit.make_env(3)
    for bad in ({"torque": -1.0}, {"nope": 1.0}, {"floor": float("inf")}):
        with pytest.raises(ValueError):
            env.set_reward_shaping(bad)
    with pytest.raises(ValueError):
        env.set_reward_shaping(SPEC, scale=-0.5)
    assert env.reward_shaping is None and env.shaping_out is None
    env.close()


# ---- 6. train.py ----------------------------------------------------------------------------------------------------------------------------------
def test_train_with_reward_shaping_and_a_ramp(tmp_path):
    log_path = str(tmp_path / "log.json")
    # --init-std 1: exploration noise of a radian per joint, so that episodes end within the sixteen steps of the run
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--iters", "2", "--num-robot", "64", "--horizon", "8", "--init-std", "1.0",
           "--reward-shaping", "torque=1e-5,work=0.05,action_rate=0.01,action_accel=0.005,impact=0.002,failure=0.7,floor=-0.5",
           "--reward-shaping-ramp", "2", "--log", log_path]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    with open(log_path) as f:
        log = json.load(f)
    assert len(log) == 2
    for rec in log:
        assert set(rec["shaping"]) == set(sr.NAMES) | {"shaped_reward"}, rec
        assert all(np.isfinite(v) for v in rec["shaping"].values()), rec
        assert np.isfinite(rec["ep_ret_mean"]) and rec["episodes"] > 0
    # the ramp: iteration 0 runs with scale 0, so its shaped reward is the imitation reward of the same steps (a mean of non-negative numbers)
    assert log[0]["shaping"]["shaped_reward"] >= 0.0
