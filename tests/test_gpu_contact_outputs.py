"""The foot contact outputs of the HIP path (orr_bind_contact_outputs; run with -m gpu on an MI355X): per leg the sums of a launch's
normal and friction impulses and its largest normal impulse (contact_out), stance steps and normal sums per episode (contact_ep) and the
episode log's contact rows -

  1. one sub-step of the debug physics: contact_out is the record's LAMBDA, bit for bit; LAMBDA against the oracle;
  2. accumulation: one launch of 8 sub-steps against 8 launches of one;
  3. the product path against the oracle's sub-step trace, bounded by the float32 parity oracle's own deviation (tests/contact_lib.py);
  4. bookkeeping with auto-reset: stance counts, normal sums, log rows, capacity, repeatability;
  5. the neighbours: unbinding, the reward terms alongside, large batches, clip sets + switching, task noise, a NaN action, friction
     anchors, captured graphs.

Measured figures: profiles/contact_outputs.txt."""
import ctypes as C

import numpy as np
import pytest

from openroborl_amd import _abi, robots
from tests import contact_lib as cl
from tests import oracle_lib as ol
from tests.gpu_kit import CLIP, EPS, SOFT_TOES, canonical_log, gpu_state64, log_rows_match, mixed_env, push_state, short_episodes, stress

pytestmark = pytest.mark.gpu


def rows(env):
    """contact_out as float32 [n, 4, 4] on the host"""
    return env.contact_out.cpu().numpy().reshape(env.num_robot, 4, 4)


def substep_env(robot, soft, n, **kw):
    from openroborl_amd.env import VecQuadrupedEnv
    return VecQuadrupedEnv(num_robot=n, seed=3, robot=robot, motion_file=CLIP[robot], mode="test", enable_randomizer=False, auto_reset=False,
                           model_overrides={robot: dict(SOFT_TOES)} if soft else None, **kw)


# ---- 1. one sub-step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,soft", [("laikago", False), ("mini_cheetah", False), ("laikago", True), ("mini_cheetah", True)])
def test_one_substep_of_the_debug_physics_writes_the_records_lambda(robot, soft):
    """The inputs of test_physics_substep_parity.  nsub = 1: contact_out[:, :, 0:3] is the record's LAMBDA bit for bit and column 3 is
    max(LAMBDA normal, 0) bit for bit - both after the one add to the +0 the sums start from, which is the identity on every value but
    -0 (the solver leaves -0 in friction words of open contacts; 0 + -0 = +0); LAMBDA against the oracle's after orc_physics_substep within that test's 5e-4; the record agrees
    with an unbound env's at that file's one-sub-step bounds (2e-6 positions, 1.5e-4 velocities, 5e-4 impulses)."""
    import torch
    from tests.parity_inputs import substep_parity_inputs
    n = 64
    env, plain = substep_env(robot, soft, n, contact_outputs=True), substep_env(robot, soft, n)
    orc = ol.OracleEnv(env.cfg, env.models, env.clips, n, robot_type=env.robot_type, clip_id=env.clip_id)
    env.reset(); plain.reset(); orc.reset()
    _, _, _, st, tau = substep_parity_inputs(robot, n)
    push_state(env, st); push_state(plain, st); orc.state[:] = st
    tg = torch.tensor(tau, dtype=torch.float32, device=env.device)
    env.contact_out.fill_(-7.0)
    env.debug_physics(tg, 1); plain.debug_physics(tg, 1)
    for i in range(n):
        orc.L.orc_physics_substep(orc.h, ol.P(orc.state[i]), ol.P(np.ascontiguousarray(tau[i])))
    out = rows(env)
    lam = env.field("LAMBDA").cpu().numpy().reshape(n, 4, 3)
    zero = np.float32(0)
    assert (out[:, :, 0:3] == lam).all() and out[:, :, 0:3].tobytes() == (zero + lam).tobytes()
    assert out[:, :, 3].tobytes() == (zero + np.maximum(lam[:, :, 0], zero)).tobytes()
    assert (lam[:, :, 0] > 0).sum() >= 8 and (lam[:, :, 0] == 0).sum() >= 8                 # touching and airborne legs
    assert not env.episode_contact.any()                                                    # env steps only
    g, p = gpu_state64(env), gpu_state64(plain)
    sl = env.layout.sl("LAMBDA")
    worst = np.abs(g[:, sl] - orc.state[:, sl]).max()
    print("CONTACT_OUTPUTS one sub-step %s%s: max |LAMBDA - oracle| %.3e (bound 5e-4), largest impulse %.3f" % (robot, " soft" if soft else "", worst, lam.max()))
    np.testing.assert_allclose(g[:, sl], orc.state[:, sl], atol=5e-4, err_msg="LAMBDA against the oracle")
    for names, tol in ((("POS", "QUAT", "Q"), 2e-6), (("LINVEL", "ANGVEL", "QD"), 1.5e-4), (("LAMBDA",), 5e-4)):
        for name in names:
            s = env.layout.sl(name)
            np.testing.assert_allclose(g[:, s], p[:, s], atol=tol, rtol=tol, err_msg="bound against unbound: " + name)
    env.close(); plain.close(); orc.close()


# ---- 2. accumulation ------------------------------------------------------------------------------------------------------------------
def test_eight_substeps_in_one_launch_sum_what_eight_launches_give():
    """From one record: one launch of nsub = 8 against eight launches of nsub = 1 after each of which the host adds LAMBDA in float32
    and takes the maximum.  Every value that crosses a sub-step boundary is a record word or a register copy of one, so the two final
    records are expected to be bit-identical (printed); then the sums and the maximum are equal bit for bit.  Otherwise both are
    compared with the float64 oracle's reduced trace by the floor rule of the product-path test."""
    import torch
    from tests.parity_inputs import substep_parity_inputs
    n, nsub = 64, 8
    one, many = substep_env("laikago", False, n, contact_outputs=True), substep_env("laikago", False, n, contact_outputs=True)
    one.reset(); many.reset()
    cfg, models, clips, st, tau = substep_parity_inputs("laikago", n)
    push_state(one, st); push_state(many, st)
    tg = torch.tensor(tau, dtype=torch.float32, device=one.device)
    one.debug_physics(tg, nsub)
    host = np.zeros((n, 4, 4), dtype=np.float32)
    for s in range(nsub):
        many.debug_physics(tg, 1)
        lam = many.field("LAMBDA").cpu().numpy().reshape(n, 4, 3)
        assert rows(many)[:, :, 0:3].tobytes() == (np.float32(0) + lam).tobytes()
        host[:, :, 0:3] = host[:, :, 0:3] + lam
        host[:, :, 3] = np.maximum(host[:, :, 3], lam[:, :, 0])
    same = torch.equal(one.state.view(torch.int32), many.state.view(torch.int32))
    print("CONTACT_OUTPUTS accumulation: records after 1 x %d and %d x 1 sub-steps bit-identical: %s" % (nsub, nsub, bool(same)))
    got = rows(one)
    assert (got[:, :, 0] > 0).sum() >= 8 and (got[:, :, 3] < got[:, :, 0]).any()         # sums of several sub-steps, not one
    if same:
        assert got.tobytes() == host.tobytes()
    else:
        tr = {}
        for f32 in (False, True):
            o = cl.TracedOracle(one.cfg, one.models, one.clips, n, one.robot_type, one.clip_id, f32=f32)
            o.orc.reset()
            o.orc.state[:] = st.astype(o.orc.dt)
            t = np.zeros((n, nsub, o.words), dtype=o.orc.dt)
            for i in range(n):
                ti = np.ascontiguousarray(tau[i], dtype=o.orc.dt)
                for s in range(nsub):
                    o.orc.L.orc_physics_substep(o.orc.h, o.orc.P(o.orc.state[i]), o.orc.P(ti))
                    t[i, s] = o.trace[i, 0]
            tr[f32] = cl.reduce_trace(t).astype(np.float64)
            o.close()
        for name, dev in (("one launch", got), ("eight launches", host)):
            r = cl.floor_rule(tr[False][None], tr[True][None], dev=dev[None])
            print("CONTACT_OUTPUTS accumulation, %s: %s" % (name, cl.describe(r)))
            assert r["f32_share"] <= cl.F32_SHARE and r["dev_share"] <= cl.DEVICE_SHARE
    one.close(); many.close()


# ---- 3. the product path against the oracle -------------------------------------------------------------------------------------------
def test_contact_rows_match_the_oracles_substep_trace_on_the_product_path():
    """N = 37 (ten waves, the last with one valid robot), Laikago and mini-cheetah mixed, train mode, randomiser on, no auto-reset, seed 3,
    40 steps of each robot's shipped policy on the device's observation + N(0, 0.05) from RandomState(11).  Every step the device's
    pre-step records and counters go into a float64 and a float32 parity oracle, both step with the trace on.  Floor rule
    (contact_lib.floor_rule): q = the 99th percentile of |f32 - f64| over the live cells, cell bound 4 q + 2^-22 max(1, |ref|); the
    float32 oracle leaves at most 0.5 % of the live leg-steps with a cell over it (else the inputs are at fault), the device at most
    2 %, dead leg-steps are exactly zero on the device unless within the same 2 %, at least 1000 leg-steps are live.  One missed
    sub-step is about 3 % of a sum of order 1 N s against a bound near 1.4e-4."""
    import torch
    n = cl.N
    env = mixed_env(n, auto_reset=False, contact_outputs=True)
    o64 = cl.TracedOracle(env.cfg, env.models, env.clips, n, env.robot_type, env.clip_id)
    o32 = cl.TracedOracle(env.cfg, env.models, env.clips, n, env.robot_type, env.clip_id, f32=True)
    rng = np.random.RandomState(cl.ACTION_SEED)
    obs = env.reset()
    ref, f32, dev, nan_steps = [], [], [], 0
    for k in range(cl.STEPS):
        act = cl.policy_actions(obs.cpu().numpy(), env.robot_type, rng)
        st64, counters = gpu_state64(env), env.counters.cpu().numpy()
        obs, rew, done, _ = env.step(torch.from_numpy(act).to(env.device))
        got = rows(env).astype(np.float64)
        r64, r32 = o64.step_from(st64, counters, act), o32.step_from(st64, counters, act)
        nan = (env.field_int("DONE_REASON")[:, 0].cpu().numpy() & _abi.DONE_NAN) != 0
        assert not got[nan].any()
        nan_steps += int(nan.sum())
        r64[nan], r32[nan] = 0.0, 0.0                       # a non-finite step is sixteen zeros by definition, not a comparison
        ref.append(r64); f32.append(r32); dev.append(got)
        stance = env.foot_contact().cpu().numpy()
        assert (stance == (got[:, :, 0] > 0)).all() and np.allclose(env.foot_forces().cpu().numpy(), got[:, :, 0:3] / (env.cfg.action_repeat * env.cfg.sim_dt), rtol=1e-6)
        assert np.allclose(env.foot_peak_force().cpu().numpy(), got[:, :, 3] / env.cfg.sim_dt, rtol=1e-6)
    r = cl.floor_rule(np.stack(ref), np.stack(f32), dev=np.stack(dev))
    print("CONTACT_OUTPUTS product path (%d robots x %d steps, %d non-finite robot-steps): %s" % (n, cl.STEPS, nan_steps, cl.describe(r)))
    env.close(); o64.close(); o32.close()
    assert r["live"] >= cl.MIN_LIVE
    assert r["f32_share"] <= cl.F32_SHARE, "the inputs are at fault"
    assert r["dev_share"] <= cl.DEVICE_SHARE


# ---- 4. bookkeeping -------------------------------------------------------------------------------------------------------------------
def bookkeeping_run(n=37, nsteps=80, seed=3, ep_log_capacity=65536, bind=None, **kw):
    """`nsteps` stress-action steps with auto-reset and short episodes.  The host accumulates contact_out per robot and episode and checks
    contact_ep after every step: stance counts exactly, normal sums within L x 2^-24 x the largest partial sum.  Returns the device's
    rows of every step (float32 bits), the host's per-episode records [(robot, length, the device's contact_ep row, return)] and the env."""
    kw.setdefault("config_overrides", short_episodes())
    kw.setdefault("auto_reset", True)
    env = mixed_env(n, seed=seed, ep_log_capacity=ep_log_capacity, contact_outputs=bind is None, **kw)
    if bind is not None:
        bind(env)
    rng = np.random.RandomState(7)
    obs = env.reset()
    count, acc, top, length = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4)), np.zeros(n, dtype=int)
    all_rows, all_ep, episodes = [], [], []
    for k in range(nsteps):
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        out, ep = rows(env), env.episode_contact.cpu().numpy().reshape(n, 4, 2)
        done = done.cpu().numpy().astype(bool)
        last_ret = env.field("LAST_EP_RETURN")[:, 0].cpu().numpy()
        assert np.isfinite(out).all() and (out[:, :, 0] >= 0).all() and (out[:, :, 3] <= out[:, :, 0]).all()
        normal = out[:, :, 0].astype(np.float64)
        count += normal > 0
        acc += normal
        top = np.maximum(top, acc)
        length += 1
        assert (ep[:, :, 0] == count).all(), "step %d: stance counts" % k
        assert (np.abs(ep[:, :, 1] - acc) <= length[:, None] * EPS * top).all(), "step %d: normal sums" % k
        for i in np.nonzero(done)[0]:
            episodes.append((int(i), int(length[i]), ep[i].copy(), float(last_ret[i])))
            if env.cfg.flags & _abi.FLAG_AUTO_RESET:
                count[i], acc[i], top[i], length[i] = 0.0, 0.0, 0.0, 0
        all_rows.append(out)
        all_ep.append(ep)
    return np.stack(all_rows), np.stack(all_ep), episodes, env


def check_log(env, episodes, logged=None):
    """The log's (return, length, contact row) triples are the host's per-episode ones (the device's own contact_ep row at the ending
    step) as a multiset; with a full log, `logged` of them."""
    k = len(episodes) if logged is None else logged
    assert int(env.counters[_abi.CNT_EPISODES].item()) == len(episodes)
    ep_log, contact_log = env.ep_log[:k].cpu().numpy(), env.contact_log[:k].cpu().numpy()
    assert (contact_log.reshape(k, 4, 2)[:, :, 0] <= ep_log[:, 1:2]).all()                 # stance steps <= length
    log_rows_match(ep_log, contact_log, [(r, l, row) for _, l, row, r in episodes], logged)


def test_stance_counts_normal_sums_and_log_rows_with_auto_reset():
    """N = 37, auto-reset, episodes of 8 .. 24 steps, 80 steps: the checks of bookkeeping_run, the log's rows, episode_gait and
    episode_log(with_contacts=True), and a second run giving identical bytes (the log up to the arrival order of one launch's slots)."""
    rows_a, ep_a, episodes, env = bookkeeping_run()
    assert len(episodes) >= 3 * 37 and len({l for _, l, _, _ in episodes}) >= 3
    assert any(row[:, 0].max() > 0 for _, _, row, _ in episodes) and any(0 < row[leg, 0] < l for _, l, row, _ in episodes for leg in range(4))
    check_log(env, episodes)
    gait = env.episode_gait()
    tot = float(sum(l for _, l, _, _ in episodes))
    want = np.sum([row.astype(np.float64) for _, _, row, _ in episodes], axis=0)
    assert sorted(gait) == ["duty", "normal_force"] and np.allclose(gait["duty"], want[:, 0] / tot, rtol=1e-12)
    assert np.allclose(gait["normal_force"], want[:, 1] / (tot * env.cfg.action_repeat * env.cfg.sim_dt), rtol=1e-6)
    assert env.episode_gait() == gait                                     # it does not clear the log
    ret, ln, cl_rows = env.episode_log(with_contacts=True)
    assert tuple(cl_rows.shape) == (len(episodes), 8) and ret.shape[0] == len(episodes)
    log_a = np.concatenate([ret.cpu().numpy()[:, None], ln.cpu().numpy()[:, None], cl_rows.cpu().numpy()], axis=1)
    assert env.episode_gait() == {}
    env.close()
    rows_b, ep_b, episodes_b, env = bookkeeping_run()
    assert rows_a.tobytes() == rows_b.tobytes() and ep_a.tobytes() == ep_b.tobytes()
    assert log_a[np.lexsort(log_a.T[::-1])].tobytes() == canonical_log(env, len(episodes_b), env.contact_log)
    env.close()


def test_a_full_log_drops_the_contact_rows_too():
    """ep_log_capacity = 4 and a contact_log of 8 rows whose last 4 hold a canary: rows 0..3 are written, the canary rows are untouched,
    ORR_CNT_EPLOG_DROPPED counts the episodes beyond 4."""
    bufs = {}

    def bind(env):
        t = env.torch
        bufs["out"], bufs["ep"] = t.zeros((env.num_robot, 16), device=env.device), t.zeros((env.num_robot, 8), device=env.device)
        bufs["log"] = t.full((8, 8), -7.0, device=env.device)
        assert env.ep_log.shape[0] == 4
        assert env.L.orr_bind_contact_outputs(env.h, bufs["out"].data_ptr(), bufs["ep"].data_ptr(), bufs["log"].data_ptr()) == 0
        env.contact_out, env.episode_contact, env.contact_log = bufs["out"], bufs["ep"], bufs["log"]
    _, _, episodes, env = bookkeeping_run(ep_log_capacity=4, bind=bind)
    assert len(episodes) > 4
    log = bufs["log"].cpu().numpy()
    assert (log[4:] == -7.0).all() and (log[:4] != -7.0).all()
    assert int(env.counters[_abi.CNT_EPLOG_DROPPED].item()) == len(episodes) - 4
    check_log(env, episodes, logged=4)
    env.close()


# ---- 5. neighbours --------------------------------------------------------------------------------------------------------------------
def test_without_the_binding_nothing_is_there_and_half_a_binding_is_refused():
    env = mixed_env(5)
    assert env.contact_out is None and env.episode_contact is None and env.contact_log is None
    with pytest.raises(ValueError, match="contact_outputs"):
        env.episode_log(with_contacts=True)
    for f in (env.episode_gait, env.foot_contact, env.foot_forces, env.foot_peak_force):
        with pytest.raises(ValueError, match="contact_outputs"):
            f()
    buf = env.torch.zeros((5, 16), device=env.device)
    assert env.L.orr_bind_contact_outputs(env.h, buf.data_ptr(), None, None) == -1 and b"contact_ep_dev" in env.L.orr_last_error()
    assert env.L.orr_bind_contact_outputs(env.h, buf.data_ptr() + 4, buf.data_ptr(), None) == -1 and b"16-byte aligned" in env.L.orr_last_error()
    env.reset(); env.step(env.torch.zeros(5, 12, device=env.device))               # nothing changed: the default kernels run
    env.torch.cuda.synchronize()
    assert not buf.any()
    env.close()


def test_after_unbinding_the_env_is_the_one_that_never_bound():
    """Bound, unbound again, then reset + 20 steps: observations, rewards, dones and records byte-identical to an env that never bound."""
    import torch
    a, b = mixed_env(37, auto_reset=True, contact_outputs=True, config_overrides=short_episodes()), mixed_env(37, auto_reset=True, config_overrides=short_episodes())
    gen = a.launch_params_generation
    a.bind_contact_outputs(False)
    assert a.contact_out is None and a.contact_log is None and a.launch_params_generation == gen + 1
    oa, ob = a.reset(), b.reset()
    rng = np.random.RandomState(4)
    for k in range(20):
        act = stress(b, ob, rng)
        (oa, ra, da, _), (ob, rb, db, _) = a.step(act), b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
    assert torch.equal(a.state.view(torch.int32), b.state.view(torch.int32)) and torch.equal(a.counters, b.counters)
    la, lb = a.ep_log.cpu().numpy(), b.ep_log.cpu().numpy()
    assert la[np.lexsort(la.T[::-1])].tobytes() == lb[np.lexsort(lb.T[::-1])].tobytes() and int(a.counters[_abi.CNT_EPISODES].item()) >= 37
    a.close(); b.close()


def test_together_with_the_reward_terms():
    """Both bindings on one handle: reward == w . terms holds (tests/test_gpu_reward_terms.py's bound) and, after one env step from one
    reset state, the contact rows and the record match a contacts-only env's at the one-sub-step bounds of tests/test_gpu_parity.py
    (5e-4 impulses, 2e-6 positions, 1.5e-4 velocities: another instantiation of the kernel, so closeness, not bit equality)."""
    import torch
    from tests import reward_terms_lib as rt
    n = 37
    a, b = mixed_env(n, auto_reset=False, contact_outputs=True, reward_terms=True), mixed_env(n, auto_reset=False, contact_outputs=True)
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    act = stress(a, oa, np.random.RandomState(2))
    (oa, ra, da, _), (ob, rb, db, _) = a.step(act), b.step(act)
    w = rt.weights(a.cfg)
    terms = a.reward_terms.cpu().numpy().astype(np.float64)
    assert (np.abs(ra.cpu().numpy().astype(np.float64) - terms @ w) <= 16.0 * EPS * np.abs(w).sum()).all() and (terms > 0).any()
    ca, cb = rows(a), rows(b)
    print("CONTACT_OUTPUTS with and without the reward terms: contact rows bit-identical: %s, max |d| %.3e" % (ca.tobytes() == cb.tobytes(), np.abs(ca - cb).max()))
    assert (cb[:, :, 0] > 0).any()
    np.testing.assert_allclose(ca, cb, atol=5e-4, rtol=5e-4)
    np.testing.assert_allclose(a.episode_contact.cpu().numpy().reshape(n, 4, 2)[:, :, 0], cb[:, :, 0] > 0)
    sa, sb = gpu_state64(a), gpu_state64(b)
    for names, tol in ((("POS", "QUAT", "Q"), 2e-6), (("LINVEL", "ANGVEL", "QD"), 1.5e-4)):
        for name in names:
            np.testing.assert_allclose(sa[:, a.layout.sl(name)], sb[:, a.layout.sl(name)], atol=tol, rtol=tol, err_msg=name)
    np.testing.assert_allclose(ra.cpu().numpy(), rb.cpu().numpy(), atol=5e-6)
    a.close(); b.close()


def test_more_waves_than_simds_stay_on_the_contact_kernel():
    """N = 4100: one step leaves no canary in any row (a fall-back to the two-wave kernel would write nothing)."""
    n = 4100
    env = mixed_env(n, auto_reset=True, contact_outputs=True)
    obs = env.reset()
    env.contact_out.fill_(-7.0); env.episode_contact.fill_(-7.0)
    env.step(stress(env, obs, np.random.RandomState(0)))
    out, ep = rows(env), env.episode_contact.cpu().numpy().reshape(n, 4, 2)
    assert np.isfinite(out).all() and (out != -7.0).all() and (out[:, :, 0] >= 0).all() and (out[:, :, 0] > 0).any()
    assert (ep[:, :, 0] == (out[:, :, 0] > 0)).all() and (ep[:, :, 1] == out[:, :, 0]).all()      # the first step of the episode overwrites the row
    env.close()


def test_with_clip_sets_and_switching(tmp_path):
    """A four-clip set with a switch interval, no auto-reset (a robot's CLIP_ID after its ending step is the clip the episode played):
    the (clip, return, contact row) triples of the log's slots are the host's, i.e. the rows of one slot belong to one episode."""
    from tests.test_gpu_clip_switch import set4
    from openroborl_amd.env import VecQuadrupedEnv
    env = VecQuadrupedEnv(num_robot=37, robot="laikago", motion_file=set4(tmp_path), mode="train", enable_randomizer=True, auto_reset=False, seed=5,
                          clip_time_min=0.1, clip_time_max=0.3, contact_outputs=True, config_overrides=short_episodes())
    assert env.clip_log is not None
    rng = np.random.RandomState(3)
    obs = env.reset()
    triples, clips_seen = [], set()
    for k in range(40):
        obs, rew, done, _ = env.step(stress(env, obs, rng))
        d = done.cpu().numpy().astype(bool)
        cid, ret, ep = env.field_int("CLIP_ID")[:, 0].cpu().numpy(), env.field("LAST_EP_RETURN")[:, 0].cpu().numpy(), env.episode_contact.cpu().numpy()
        clips_seen |= set(cid.tolist())
        triples += [(int(cid[i]), ret[i].tobytes(), ep[i].tobytes()) for i in np.nonzero(d)[0]]
    k = int(env.counters[_abi.CNT_EPISODES].item())
    assert k == len(triples) >= 37 and len(clips_seen) >= 3
    ep_log, contact_log, clip_log = env.ep_log[:k].cpu().numpy(), env.contact_log[:k].cpu().numpy(), env.clip_log[:k].cpu().numpy()
    assert sorted((int(clip_log[j]), ep_log[j, 0].tobytes(), contact_log[j].tobytes()) for j in range(k)) == sorted(triples)
    ret, ln, cid, crow = env.episode_log(with_clip=True, with_contacts=True)
    assert tuple(cid.shape) == (k,) and tuple(crow.shape) == (k, 8)
    env.close()


def test_with_task_noise():
    """Perturbed initial states and target-heading noise on: counts, sums and log rows hold as without."""
    _, _, episodes, env = bookkeeping_run(nsteps=40, perturb_init_state_prob=0.5, tar_obs_noise=[0.1])
    assert len(episodes) >= 37
    check_log(env, episodes)
    env.close()


def test_a_nan_action_gives_sixteen_zeros_and_done_nan():
    import torch
    n = 9
    env = mixed_env(n, auto_reset=False, contact_outputs=True)
    obs = env.reset()
    rng = np.random.RandomState(1)
    env.step(stress(env, obs, rng))
    before = env.episode_contact.cpu().numpy().copy()
    act = stress(env, env.obs, rng)
    act[4, 7] = float("nan")
    env.contact_out.fill_(-7.0)
    env.step(act)
    out, reason = rows(env), env.field_int("DONE_REASON")[:, 0].cpu().numpy()
    assert reason[4] & _abi.DONE_NAN and not out[4].any() and out[4].tobytes() == np.zeros(16, dtype=np.float32).tobytes()
    assert not (np.delete(reason, 4) & _abi.DONE_NAN).any() and (np.delete(out, 4, axis=0)[:, :, 0] > 0).any() and (out != -7.0).all()
    assert (env.episode_contact.cpu().numpy()[4] == before[4]).all()                # a step of sixteen zeros adds nothing
    env.close()


def test_friction_anchors_are_refused_at_bind_and_at_launch():
    import torch
    from openroborl_amd.env import VecQuadrupedEnv
    kw = dict(num_robot=8, robot="laikago", motion_file="laikago_pace", mode="test", enable_randomizer=False, seed=5)
    with pytest.raises(RuntimeError, match="orr_bind_contact_outputs: friction anchors"):
        VecQuadrupedEnv(contact_outputs=True, model_overrides={"laikago": {"friction_anchor": 1}}, **kw)
    anchored = VecQuadrupedEnv(model_overrides={"laikago": {"friction_anchor": 1}}, **kw)
    assert anchored.L.orr_bind_contact_outputs(anchored.h, None, None, None) == 0             # unbinding an anchor handle is fine
    with pytest.raises(RuntimeError, match="friction anchors"):
        anchored.bind_contact_outputs(True)
    assert anchored.contact_out is None
    anchored.reset(); anchored.step(torch.zeros(8, 12, device=anchored.device))               # nothing changed: the anchor kernels run
    anchored.close()
    # an anchor model set on a handle with the outputs bound: every launch is refused and nothing runs
    env = VecQuadrupedEnv(contact_outputs=True, **kw)
    env.reset()
    act = torch.zeros(8, 12, device=env.device)
    env.step(act)
    t = robots.ROBOT_TYPE_ID["laikago"]
    m = dict(env.models[t])
    m["friction_anchor"] = 1
    assert env.L.orr_set_model(env.h, t, C.byref(robots.to_struct(m))) == 0
    torch.cuda.synchronize()
    before = env.state.clone(), env.contact_out.clone(), env.episode_contact.clone()
    with pytest.raises(RuntimeError, match=r"orr_reset: friction anchors \(orr_model::friction_anchor\) and contact outputs \(orr_bind_contact_outputs\) cannot be combined"):
        env.reset()
    with pytest.raises(RuntimeError, match=r"orr_step: friction anchors .* contact outputs"):
        env.step(act)
    with pytest.raises(RuntimeError, match=r"orr_debug_physics: friction anchors .* contact outputs"):
        env.debug_physics(act, 1)
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), before[0].view(torch.int32)) and torch.equal(env.contact_out, before[1]) and torch.equal(env.episode_contact, before[2])
    env.close()


def test_graph_rollout_recaptures_after_the_binding():
    """A GraphRollout that captured its segment on the unbound env captures again after bind_contact_outputs (launch_params_generation
    moved): the replayed segment runs the contact kernel and writes the rows."""
    import torch
    from openroborl_amd import ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = torch.device("cuda:0")
    n, T = 64, 4
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev)
    model = ppo.ActorCritic(dev, seed=1).enable_fused()
    collector = rollout.GraphRollout(env, model, T)
    obs = env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for seg in range(2):                                         # eager, then captured
        obs = collector.collect(obs, noise=torch.randn(T, n, 12, device=dev, generator=gen))["last_obs"]
    first, captured_for = collector.graph, collector._captured_for
    assert first is not None
    env.bind_contact_outputs(True)
    obs = env.step(torch.zeros(n, 12, device=dev))[0]           # the variant's first launch loads its code object: not inside a capture
    env.contact_out.fill_(-7.0)
    collector.collect(obs, noise=torch.randn(T, n, 12, device=dev, generator=gen))
    torch.cuda.synchronize()
    assert collector.graph is not first and collector._captured_for != captured_for
    out = rows(env)
    assert (out != -7.0).all() and (out[:, :, 0] > 0).any()
    env.close()
