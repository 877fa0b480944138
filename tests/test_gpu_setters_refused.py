"""A setter of the C-ABI that refuses its argument leaves no trace (run with -m gpu on an MI355X): each call below goes to the library
directly (env.L, past the Python validators), is refused on the host before any copy - return code -1 and the message of
orr_last_error, letter for letter - and afterwards the env steps bit for bit like a twin that never received the calls.  Nothing here
launches with a bad pointer: the offset pointers and the lone first pointers never get past the checks, and every buffer has a spare
row behind it."""
import ctypes as C

import numpy as np
import pytest

from openroborl_amd import _abi, robots
from tests.gpu_kit import make_env, stress

pytestmark = pytest.mark.gpu
N = 8


def refused_calls(env):
    """[(what, return code, message)] of one refused call per setter on env's handle"""
    import torch
    L, h, t = env.L, env.h, robots.ROBOT_TYPE_ID["laikago"]

    def buf(*shape):        # a valid, 16-byte aligned device buffer with a spare leading row
        return torch.zeros((shape[0] + 1,) + shape[1:], dtype=torch.float32, device=env.device)
    rnd = _abi.OrrRandomizer()
    p = _abi.RAND_PARAM_NAMES.index("mass")
    rnd.enabled[p], rnd.lo[p], rnd.hi[p] = 1, 1.2, 0.8
    limits = (C.c_float * 12)(*([20.0] * 3 + [-1.0] + [20.0] * 8))
    terms, contact, contact_ep = buf(N, _abi.NUM_REWARD_TERMS), buf(N, _abi.CONTACT_OUT_DIM), buf(N, _abi.CONTACT_EP_DIM)
    act, act_ep = buf(N, _abi.NUM_MOTORS, _abi.ACTUATOR_OUT_DIM), buf(N, _abi.ACTUATOR_EP_DIM)
    push, rows = buf(N, _abi.PUSH_ROW), buf(N, _abi.RAND_ROW)
    for x in (terms, contact, contact_ep, act, act_ep, push, rows):
        assert x.data_ptr() % 16 == 0
    calls = (
        ("task noise, NaN deviation", lambda: L.orr_set_task_noise(h, C.byref(_abi.OrrTaskNoise(root_pos_std=float("nan"))))),
        ("sensor noise, negative deviation", lambda: L.orr_set_sensor_noise(h, C.byref(_abi.OrrSensorNoise(base_rpy_std=-0.1)))),
        ("randomiser, lo > hi", lambda: L.orr_set_randomizer(h, C.byref(rnd))),
        ("push, prob > 1", lambda: L.orr_set_push(h, C.byref(_abi.OrrPush(prob=1.5)))),
        ("clip switch, tmin > tmax", lambda: L.orr_set_clip_switch(h, t, 2.0, 1.0)),
        ("torque limits, negative limit", lambda: L.orr_set_torque_limits(h, t, limits)),
        ("reward terms, first pointer alone", lambda: L.orr_bind_reward_terms(h, terms.data_ptr(), None, None)),
        ("contact outputs, first pointer alone", lambda: L.orr_bind_contact_outputs(h, contact.data_ptr(), None, None)),
        ("actuator outputs, first pointer alone", lambda: L.orr_bind_actuator_outputs(h, act.data_ptr(), None, None)),
        ("contact outputs, misaligned", lambda: L.orr_bind_contact_outputs(h, contact.data_ptr() + 4, contact_ep.data_ptr(), None)),
        ("actuator outputs, misaligned", lambda: L.orr_bind_actuator_outputs(h, act.data_ptr() + 4, act_ep.data_ptr(), None)),
        ("push outputs, misaligned", lambda: L.orr_bind_push_outputs(h, push.data_ptr() + 4)),
        ("randomiser params, misaligned", lambda: L.orr_bind_randomizer_params(h, rows.data_ptr() + 4, 0)),
    )
    out = []
    for what, call in calls:
        rc = call()
        out.append((what, rc, L.orr_last_error().decode()))
    return out


# the messages as the C-ABI has always worded them (orr_kernels.hip before its setters shared their helpers)
MESSAGES = {
    "task noise, NaN deviation": "orr_set_task_noise: root_pos_std must be a finite standard deviation >= 0",
    "sensor noise, negative deviation": "orr_set_sensor_noise: base_rpy_std must be a finite standard deviation >= 0",
    "randomiser, lo > hi": "orr_set_randomizer: mass: lo > hi",
    "push, prob > 1": "orr_set_push: prob must be a probability in [0, 1]",
    "clip switch, tmin > tmax": "orr_set_clip_switch: tmin > tmax",
    "torque limits, negative limit": "orr_set_torque_limits: limits_host[3] must be a torque >= 0 or +inf (no limit)",
    "reward terms, first pointer alone": "orr_bind_reward_terms: terms_dev needs term_sums_dev (the running sums of the current episode)",
    "contact outputs, first pointer alone": "orr_bind_contact_outputs: contact_dev needs contact_ep_dev (the totals of the current episode)",
    "actuator outputs, first pointer alone": "orr_bind_actuator_outputs: act_dev needs act_ep_dev (the totals of the current episode)",
    "contact outputs, misaligned": "orr_bind_contact_outputs: the contact buffers must be 16-byte aligned (rows of 16 and 8 floats)",
    "actuator outputs, misaligned": "orr_bind_actuator_outputs: the actuator buffers (act_dev, act_ep_dev, act_log_dev) must be 16-byte aligned (rows of 4 floats)",
    "push outputs, misaligned": "orr_bind_push_outputs: push_dev must be 16-byte aligned (rows of ORR_PUSH_ROW floats)",
    "randomiser params, misaligned": "orr_bind_randomizer_params: params_dev must be 16-byte aligned (rows of ORR_RAND_ROW floats)",
}


def test_refused_setters_leave_no_trace():
    import torch
    env, twin = make_env(N), make_env(N)
    obs, obs_twin = env.reset(), twin.reset()
    generation = env.launch_params_generation
    results = refused_calls(env)
    assert [what for what, _, _ in results] == list(MESSAGES)
    for what, rc, message in results:
        assert rc == -1, (what, rc, message)
        assert message == MESSAGES[what], what
    assert env.launch_params_generation == generation
    rng, rng_twin = np.random.RandomState(17), np.random.RandomState(17)
    for _ in range(3):
        obs, reward, done, _ = env.step(stress(env, obs, rng))
        obs_twin, reward_twin, done_twin, _ = twin.step(stress(twin, obs_twin, rng_twin))
        torch.cuda.synchronize()
        assert torch.equal(obs.view(torch.int32), obs_twin.view(torch.int32))
        assert torch.equal(reward.view(torch.int32), reward_twin.view(torch.int32))
        assert torch.equal(done, done_twin)
        assert torch.equal(env.state.view(torch.int32), twin.state.view(torch.int32))
    assert bool(torch.isfinite(obs).all())
    env.close()
    twin.close()
