"""The step kernel's launch tally and inline auto-reset on the MI355X.

  * counters after EVERY launch (one-wave kernel, two-wave kernel, a batch whose last wave is partial, a batch of several
    dispatch rounds): slot 0 = start + the host sum of `done`, slot 3 = start + K N, the per-launch scratch slots 1 and 2 zero;
  * a host write to slot 0 between launches is the curriculum counter that the next launch's new episodes take their time limit from;
  * an inline auto-reset gives the same bits as a step without it followed by an explicit masked reset (obs, the whole record).
"""
import os

import numpy as np
import pytest

from openroborl_amd import _abi, motion

pytestmark = pytest.mark.gpu


def make_env(n, **kw):
    from openroborl_amd.env import VecQuadrupedEnv
    kw.setdefault("task_name", "imitation_learning_laikago")
    kw.setdefault("mode", "train")
    kw.setdefault("enable_randomizer", True)
    kw.setdefault("auto_reset", True)
    kw.setdefault("seed", 17)
    return VecQuadrupedEnv(num_robot=n, **kw)


def time_limit(cfg, total):
    """orr_task.h time_limit (wrapper_env.py:151-159)"""
    if not (cfg.flags & _abi.FLAG_CURRICULUM) or cfg.curriculum_steps <= 0:
        return cfg.ep_len_end
    t = min(max(float(total) / float(cfg.curriculum_steps), 0.0), 1.0)
    t = t * t * t
    return int((1.0 - t) * cfg.ep_len_start + t * cfg.ep_len_end)


# n: 4096 = one wave per SIMD; 8192 = the two-wave kernel; 4098 = two-wave kernel, last wave partial; 16386 = four dispatch rounds
# of the two-wave kernel plus a partial wave
SIZES = [4096, 4098, 8192, 16386]


@pytest.mark.parametrize("n", SIZES)
def test_counters_after_every_launch(n):
    import torch
    env = make_env(n)
    env.reset()
    start = env.counters.cpu().numpy().copy()
    assert start[_abi.CNT_DONE_ACCUM] == 0 and start[_abi.CNT_TICKET] == 0
    g = torch.Generator(device="cpu"); g.manual_seed(3)
    done_sum = 0
    for k in range(25):
        a = (torch.randn(n, 12, generator=g) * 0.125).to(env.device)
        _, _, done, _ = env.step(a)
        torch.cuda.synchronize()
        done_sum += int(done.sum().item())
        cnt = env.counters.cpu().numpy()
        assert cnt[_abi.CNT_TOTAL_STEP_COUNT] == start[_abi.CNT_TOTAL_STEP_COUNT] + done_sum, k
        assert cnt[_abi.CNT_TOTAL_TIMESTEPS] == start[_abi.CNT_TOTAL_TIMESTEPS] + (k + 1) * n, k
        assert cnt[_abi.CNT_DONE_ACCUM] == 0 and cnt[_abi.CNT_TICKET] == 0, k
    assert done_sum >= n          # 20-step episodes at the curriculum's start: every robot finished at least once
    env.close()


@pytest.mark.parametrize("n", [4096, 8192])
def test_host_write_sets_next_time_limit(n):
    import torch
    env = make_env(n)
    env.reset()
    g = torch.Generator(device="cpu"); g.manual_seed(4)
    value = env.cfg.curriculum_steps // 2
    want = time_limit(env.cfg, value)
    assert want != time_limit(env.cfg, 0)
    seen = 0
    for k in range(25):
        env.counters[_abi.CNT_TOTAL_STEP_COUNT] = value      # between launches: the next launch's snapshot
        a = (torch.randn(n, 12, generator=g) * 0.125).to(env.device)
        _, _, done, _ = env.step(a)
        torch.cuda.synchronize()
        d = done.bool()
        mx = env.field_int("MAX_EP_STEPS")[:, 0]
        assert (mx[d] == want).all(), k
        seen += int(d.sum().item())
    assert seen > 0
    env.close()


def run_pair(n, steps, **kw):
    """Env A: inline auto-reset.  Env B: no auto-reset, then reset(mask=done) with the curriculum counter set back to the value the
    launch started with (the inline reset uses the launch-start snapshot), then restored.  After every step both
    envs must hold the same bits."""
    import torch
    a_env = make_env(n, auto_reset=True, **kw)
    b_env = make_env(n, auto_reset=False, **kw)
    a_env.reset(); b_env.reset()
    torch.testing.assert_close(a_env.state, b_env.state, rtol=0, atol=0)
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    resets = 0
    for k in range(steps):
        act = (torch.randn(n, 12, generator=g) * 0.125).to(a_env.device)
        snap = int(b_env.counters[_abi.CNT_TOTAL_STEP_COUNT].item())
        _, ra, da, _ = a_env.step(act)
        _, rb, db, _ = b_env.step(act)
        torch.cuda.synchronize()
        assert torch.equal(da, db) and torch.equal(ra, rb), k
        mask = db.bool()
        if mask.any():
            after = int(b_env.counters[_abi.CNT_TOTAL_STEP_COUNT].item())
            b_env.counters[_abi.CNT_TOTAL_STEP_COUNT] = snap
            b_env.reset(mask=mask)
            b_env.counters[_abi.CNT_TOTAL_STEP_COUNT] = after
            torch.cuda.synchronize()
            resets += int(mask.sum().item())
        np.testing.assert_array_equal(a_env.obs.cpu().numpy().view(np.uint32), b_env.obs.cpu().numpy().view(np.uint32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(a_env.state.cpu().numpy().view(np.uint32), b_env.state.cpu().numpy().view(np.uint32), err_msg="record, step %d" % k)
        np.testing.assert_array_equal(a_env.counters.cpu().numpy(), b_env.counters.cpu().numpy(), err_msg="counters, step %d" % k)
    assert resets >= n
    a_env.close(); b_env.close()


@pytest.mark.parametrize("n", [4096, 8192])
def test_inline_reset_equals_explicit_reset(n):
    run_pair(n, 25)


def test_inline_reset_equals_explicit_reset_multiclip():
    files = [os.path.join(motion.DATA_DIR, f) for f in ("laikago_pace.txt", "laikago_trot.txt", "laikago_spin.txt", "laikago_sidesteps.txt")]
    run_pair(1024, 25, motion_file=files, clip_time_min=0.1, clip_time_max=0.3)
