"""The end of the step kernel on the MI355X: inline auto-reset, one observation per robot, every store and both atomics at the end.

The protocol is run_pair's of tests/test_gpu_launch_tally.py - an env with auto-reset against an env without it plus reset(mask=done),
compared bit for bit (observations, records, counters) after every step - on a batch built so that ONE launch holds every mix of
resetting and continuing robots a wave can have: 67 robots = 16 full waves and a padded one, and MAX_EP_STEPS written into both envs'
records so that at step 1 wave w resets exactly the robots in the bits of w (all 16 patterns; the padded wave resets nobody), and the
remaining robots reset at steps 2 and 3.  Once with the default kernels, once with reward terms, contact outputs and actuator outputs
bound, once with task noise (perturbed initial states with probability 0.5, target-heading sigma 0.1).

Episode log: its (return, length) rows are, as a multiset, what the host accumulates from reward_out / done_out; with the outputs
bound every slot's term, contact and actuator sums are the rows of the robot and episode of the (return, length) row in the same slot;
the cursor equals the number of dones; with a cap of 5 rows the drops are dones - 5 and nothing is written past the cap; with no log
bound the cursor still counts.
"""
import numpy as np
import pytest

from openroborl_amd import _abi
from tests.test_gpu_launch_tally import make_env

pytestmark = pytest.mark.gpu

N = 67                      # 16 full waves + one wave with three robots and a padding lane group
SENTINEL = -7.0


def limits():
    """MAX_EP_STEPS per robot: robot 4 w + b ends its first episode at step 1 where bit b of w is set (w < 16), the others at step 2 or 3"""
    r = np.arange(N)
    first = ((r // 4) < 16) & ((((r // 4) >> (r % 4)) & 1) == 1)
    return np.where(first, 1, 2 + (r % 2)).astype(np.int32), first


def set_limits(env):
    import torch
    lim, _ = limits()
    env.field_int("MAX_EP_STEPS")[:, 0] = torch.from_numpy(lim).to(env.device)


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32 if x.element_size() == 4 else np.uint8)


class HostEpisodes(object):
    """what the host accumulates from reward_out / done_out: float32 returns in the device's order of additions, lengths, finished episodes"""

    def __init__(self):
        self.ret = np.zeros(N, dtype=np.float32)
        self.len = np.zeros(N, dtype=np.int64)
        self.rows = []          # (return bits, length, side row bits) per finished episode

    def step(self, rew, done, side=None):
        self.ret = (self.ret + rew).astype(np.float32)
        self.len += 1
        for i in np.nonzero(done)[0]:
            self.rows.append((self.ret[i].tobytes(), int(self.len[i]), b"" if side is None else side[i].tobytes()))
        self.ret[done] = 0.0
        self.len[done] = 0


def side_rows(env):
    """[N, 5 + 8 + 4] the robots' current-episode rows of the three bound outputs (after a step that ended an episode: that episode's)"""
    return np.concatenate([env.episode_term_sums.cpu().numpy(), env.episode_contact.cpu().numpy(), env.episode_actuator.cpu().numpy()], axis=1)


def log_rows(env, k, with_side):
    log = env.ep_log[:k].cpu().numpy()
    side = np.concatenate([env.term_log[:k].cpu().numpy(), env.contact_log[:k].cpu().numpy(), env.actuator_log[:k].cpu().numpy()], axis=1) if with_side else None
    return sorted((log[j, 0].tobytes(), int(log[j, 1]), b"" if side is None else side[j].tobytes()) for j in range(k))


def run(with_side=False, **kw):
    import torch
    a_env = make_env(N, auto_reset=True, **kw)
    b_env = make_env(N, auto_reset=False, **kw)
    a_env.reset(); b_env.reset()
    set_limits(a_env); set_limits(b_env)
    assert np.array_equal(bits(a_env.state), bits(b_env.state))
    _, first = limits()
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    host = HostEpisodes()
    seen = np.zeros(N, dtype=bool)
    for k in range(3):
        act = (torch.randn(N, 12, generator=g) * 0.125).to(a_env.device)
        snap = int(b_env.counters[_abi.CNT_TOTAL_STEP_COUNT].item())
        _, ra, da, _ = a_env.step(act)
        _, rb, db, _ = b_env.step(act)
        torch.cuda.synchronize()
        assert torch.equal(da, db) and np.array_equal(bits(ra), bits(rb)), k
        mask = db.bool()
        done = mask.cpu().numpy()
        if k == 0:      # every reset pattern of a wave, in one launch
            waves = [int(sum(int(done[4 * w + b]) << b for b in range(4))) for w in range(16)]
            assert waves == list(range(16)) and not done[64:].any(), waves
            assert np.array_equal(done, first)
        host.step(ra.cpu().numpy(), done, side_rows(a_env) if with_side else None)
        if with_side:   # the outputs of both envs, before the explicit reset (it does not touch them)
            for x, y in ((a_env.reward_terms, b_env.reward_terms), (a_env.episode_term_sums, b_env.episode_term_sums), (a_env.contact_out, b_env.contact_out),
                         (a_env.episode_contact, b_env.episode_contact), (a_env.actuator_out, b_env.actuator_out), (a_env.episode_actuator, b_env.episode_actuator)):
                assert np.array_equal(bits(x), bits(y)), k
        if mask.any():
            after = int(b_env.counters[_abi.CNT_TOTAL_STEP_COUNT].item())
            b_env.counters[_abi.CNT_TOTAL_STEP_COUNT] = snap
            b_env.reset(mask=mask)
            b_env.counters[_abi.CNT_TOTAL_STEP_COUNT] = after
            torch.cuda.synchronize()
        seen |= done
        np.testing.assert_array_equal(bits(a_env.obs), bits(b_env.obs), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(bits(a_env.state), bits(b_env.state), err_msg="record, step %d" % k)
        np.testing.assert_array_equal(a_env.counters.cpu().numpy(), b_env.counters.cpu().numpy(), err_msg="counters, step %d" % k)
    assert seen.all()                         # the remaining robots reset in steps 2 and 3
    dones = len(host.rows)
    assert dones >= N
    for env in (a_env, b_env):
        cnt = env.counters.cpu().numpy()
        assert cnt[_abi.CNT_EPISODES] == dones and cnt[_abi.CNT_EPLOG_DROPPED] == 0       # the cursor = the number of dones: distinct slots 0 .. dones - 1
        assert log_rows(env, dones, with_side) == sorted(host.rows)
        assert not env.ep_log[dones:].any()
    if with_side:
        assert len({r[2] for r in host.rows}) == dones        # the side rows tell the episodes apart: a row in the wrong slot would show
    assert len({r[0] for r in host.rows}) == dones            # so do the returns
    a_env.close(); b_env.close()


def test_default_kernels():
    run()


def test_reward_terms_contact_and_actuator_outputs_bound():
    run(with_side=True, reward_terms=True, contact_outputs=True, actuator_outputs=True)


def test_task_noise():
    run(perturb_init_state_prob=0.5, tar_obs_noise=[0.1])


def steps_with_log(env, bind):
    """three steps of the auto-reset env with the log bound by `bind`; -> the number of dones"""
    import torch
    env.reset()
    set_limits(env)
    bind(env)
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    dones = 0
    for k in range(3):
        _, _, d, _ = env.step((torch.randn(N, 12, generator=g) * 0.125).to(env.device))
        dones += int(d.sum().item())
    torch.cuda.synchronize()
    assert dones >= N
    return dones


def test_a_log_of_five_rows_drops_the_rest_and_nothing_is_written_past_the_cap():
    import torch
    env = make_env(N)
    buf = torch.full((5 + 64, 2), SENTINEL, dtype=torch.float32, device=env.device)
    dones = steps_with_log(env, lambda e: _lib_check(e, e.L.orr_bind(e.h, e.state.data_ptr(), e.counters.data_ptr(), buf.data_ptr(), 5)))
    cnt = env.counters.cpu().numpy()
    assert cnt[_abi.CNT_EPISODES] == dones and cnt[_abi.CNT_EPLOG_DROPPED] == dones - 5
    rows = buf.cpu().numpy()
    assert (rows[5:] == SENTINEL).all() and (rows[:5] != SENTINEL).all()
    assert (rows[:5, 1] >= 1).all() and (rows[:5, 1] <= 3).all() and np.isfinite(rows[:5, 0]).all()
    env.close()


def test_without_a_log_the_cursor_still_counts():
    env = make_env(N)
    dones = steps_with_log(env, lambda e: _lib_check(e, e.L.orr_bind(e.h, e.state.data_ptr(), e.counters.data_ptr(), None, 0)))
    cnt = env.counters.cpu().numpy()
    assert cnt[_abi.CNT_EPISODES] == dones and cnt[_abi.CNT_EPLOG_DROPPED] == 0
    assert not env.ep_log.any()               # the env's own buffer, no longer bound
    env.close()


def _lib_check(env, rc):
    assert rc == 0, env.L.orr_last_error()
