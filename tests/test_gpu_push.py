"""External pushes of the HIP path (orr_set_push, orr_bind_push_outputs; run with -m gpu on an MI355X): a velocity kick of the base
twist at the start of an env step, drawn on the episode's Philox stream -

  5. the rows of the outputs buffer against the float64 predictor (env.push_kick on the oracle's stream): kicked flag and count exact,
     unkicked rows exactly zero, the components within their derived bounds, padding rows untouched;
  6. the kick is physics: from the device's pre-step records the float64 and the float32 parity oracle, with the predictor's kick added,
     bound the device's post-step rigid state by the floor rule; the unkicked float64 step lies far outside;
  7. nothing else moves: prob 0, a grace period longer than the run, every other feature on with and without push, and a handle that had
     pushes and dropped them are bit for bit the env without push;
  8. push alone selects the variant: identical to the default env up to a robot's first kick, never-kicked robots throughout;
  9. stream independence: a robot's rows do not depend on the batch it is in; the seed decides them;
  10. refusals on a live handle, the generation counter, the LegacyListEnv pass-through.

Bounds of (5), with u = m / 2^24 the stream's uniforms and the float32 settings on both sides.  Horizontal components m cos / m sin,
per unit of m: the sine / cosine polynomial < 1e-7 (measured, profiles/device_primitives.txt), the angle's rounding half an ulp of an
argument <= pi / 4 (6e-8 at most), the product one rounding (6e-8), m = fmaf(u, hi - lo, lo) one rounding of hi - lo and one of the
result (<= 1.2e-7 relative to lin_hi) - about 2.5e-7 lin_hi, bound 2^-21 lin_hi = 4.8e-7 lin_hi (a margin of two).  dv_z and dw_k are
one fmaf of exact operands each: half an ulp of a result below the bound b in magnitude, at most 2^-24 * 2 b = 2^-23 b.

Measured figures: profiles/push.txt."""
import ctypes as C

import numpy as np
import pytest

from openroborl_amd import _abi, robots
from openroborl_amd import env as envmod
from tests import actuator_lib as al
from tests import contact_lib as cl
from tests import drift
from tests import oracle_lib as ol
from tests import push_lib as pl
from tests.gpu_kit import canonical_log, gpu_state64, mixed_env, short_episodes, stress

pytestmark = pytest.mark.gpu
SENTINEL = pl.SENTINEL


def own_rows(env, n, pad=pl.PAD):
    """The test's own outputs buffer: n + pad rows filled with a sentinel, bound through the C-ABI"""
    buf = env.torch.full((n + pad, _abi.PUSH_ROW), SENTINEL, device=env.device)
    assert env.L.orr_bind_push_outputs(env.h, buf.data_ptr()) == 0
    env.push_out = buf[:n]
    return buf


def bits(x):
    import torch
    return x.view(torch.int32) if x.dtype == torch.float32 else x


# ---- 5. / 6. the run of the physics comparison -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product_run():
    """push_lib's inputs on the device: N = 37 mixed, train mode, randomiser on, auto-reset, env seed push_lib.SEED, 40 steps of each
    robot's shipped policy on the device's observation + N(0, 0.05) from RandomState(11), prob 0.25, lin_vel (0.2, 0.6), lin_vel_z 0.2,
    ang_vel 0.5.  Every step the device's pre-step records and counters go into push_lib.ThreeOracles with the predictor's kick."""
    import torch
    n = pl.N
    assert n % 4 != 0
    env = mixed_env(n, seed=pl.SEED, auto_reset=True, push=pl.PUSH)
    buf = own_rows(env, n)
    T = pl.ThreeOracles(env.cfg, env.models, env.clips, n, env.robot_type, env.clip_id)
    L = ol.lib()
    rng = np.random.RandomState(pl.ACTION_SEED)
    obs = env.reset()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                      # no reset touches the buffer
    R = {k: [] for k in ("rows", "pad", "kicked", "dv", "dw", "s", "ref", "f32", "free", "dev", "nan", "obs_dev", "obs_ref", "obs_f32", "rew_dev", "rew_ref",
                         "rew_f32", "done_dev", "done_ref")}
    for k in range(pl.STEPS):
        act = cl.policy_actions(obs.cpu().numpy(), env.robot_type, rng)
        st64, counters = gpu_state64(env), env.counters.cpu().numpy()
        kicked, dv, dw = pl.kicks(L, env.push, pl.SEED, st64, env.layout)
        buf[:, :7].fill_(SENTINEL)                             # (word 7 is the step's own input: the episode's count so far)
        obs, rew, done, _ = env.step(torch.from_numpy(act).to(env.device))
        rows = buf.cpu().numpy().copy()
        R["rows"].append(rows[:n]); R["pad"].append(rows[n:])
        R["kicked"].append(kicked); R["dv"].append(dv); R["dw"].append(dw); R["s"].append(pl.stream_words(env.layout, st64)[2])
        R["dev"].append(al.rigid_of(env.layout, gpu_state64(env)))
        R["nan"].append((env.field_int("DONE_REASON")[:, 0].cpu().numpy() & _abi.DONE_NAN) != 0)
        R["obs_dev"].append(obs.cpu().numpy().astype(np.float64)); R["rew_dev"].append(rew.cpu().numpy().astype(np.float64))
        R["done_dev"].append(done.cpu().numpy().astype(bool))
        r = T.step_from(st64, counters, act, dv, dw)
        for name in ("ref", "f32", "free"):
            R[name].append(r[name])
        R["obs_ref"].append(r["obs"]); R["obs_f32"].append(r["obs32"]); R["rew_ref"].append(r["reward"]); R["rew_f32"].append(r["reward32"])
        R["done_ref"].append(r["done"])
    R = {k: np.stack(v) for k, v in R.items()}
    R["spec"] = env.push
    env.close(); T.close()
    return R


def test_kick_rows_match_the_predictor(product_run):
    """(5).  Measured on an MI355X: profiles/push.txt."""
    R = product_run
    spec, rows, kicked = R["spec"], R["rows"].astype(np.float64), R["kicked"]
    assert np.isfinite(rows).all() and bool((R["pad"] == SENTINEL).all())
    assert np.array_equal(rows[..., 6], kicked.astype(np.float64))                      # word 6
    count = np.zeros(rows.shape[1])
    for k in range(rows.shape[0]):                                                    # word 7 restarts where EP_STEP before the step is 0
        count = np.where(R["s"][k] == 0, 0.0, count) + kicked[k]
        assert np.array_equal(rows[k, :, 7], count), k
    assert (R["s"][1:] == 0).sum() > 0 and rows[..., 7].max() >= 3
    assert not rows[~kicked][:, :7].any()                                             # not kicked: exactly zero
    lin_hi, lin_z, ang = float(spec.lin_hi), float(spec.lin_z), float(spec.ang)
    e_xy = np.abs(rows[kicked][:, 0:2] - R["dv"][kicked][:, 0:2]).max()
    e_z = np.abs(rows[kicked][:, 2] - R["dv"][kicked][:, 2]).max()
    e_w = np.abs(rows[kicked][:, 3:6] - R["dw"][kicked]).max()
    print("PUSH rows: %d kicks in %d robot-steps; worst |dv_xy - predictor| %.3e (bound %.3e), |dv_z| %.3e (bound %.3e), |dw| %.3e (bound %.3e)" % (
        int(kicked.sum()), kicked.size, e_xy, 2.0 ** -21 * lin_hi, e_z, 2.0 ** -23 * lin_z, e_w, 2.0 ** -23 * ang))
    assert kicked.sum() > 300
    assert e_xy <= 2.0 ** -21 * lin_hi and e_z <= 2.0 ** -23 * lin_z and e_w <= 2.0 ** -23 * ang
    mag = np.hypot(rows[kicked][:, 0], rows[kicked][:, 1])
    assert (mag >= spec.lin_lo - 2.0 ** -21 * lin_hi).all() and (mag <= spec.lin_hi + 2.0 ** -21 * lin_hi).all()


def test_the_kick_is_physics(product_run):
    """(6).  Floor rule per rigid field over [steps, n] cells: the float32 oracle at most 0.5 % over the bound (else the inputs are at
    fault), the device at most 2 %; the unkicked float64 step outside the bound in more than 10 % of all cells, so a device that
    reported kicks without applying them fails.  Observation, reward and done of the same steps as tests/test_gpu_parity.py's step
    parity bounds them: within the float32 oracle's own error (drift.assert_within_float32_floor), done flags agree in > 97 %."""
    R = product_run
    ok = ~R["nan"]
    per, outside = pl.shares(R["ref"], R["f32"], R["free"], dev=R["dev"], ok=ok)
    print("PUSH physics: %d kicks in %d robot-steps, %d non-finite; the unkicked float64 step outside the bound in %.1f %% of all cells" % (
        int(R["kicked"].sum()), R["kicked"].size, int(R["nan"].sum()), 100 * outside))
    for name, r in per.items():
        print("PUSH physics %s: %s | unkicked outside %.1f %%" % (name, al.describe(r), 100 * r["free_share"]))
    for name, r in per.items():
        assert r["f32_share"] <= al.F32_SHARE, "the inputs are at fault: " + name
        assert r["dev_share"] <= al.DEVICE_SHARE, name
    assert outside > 0.10
    drift.assert_within_float32_floor(np.abs(R["rew_dev"] - R["rew_ref"])[ok], np.abs(R["rew_f32"] - R["rew_ref"])[ok], "push step reward")
    for what, sl in drift.OBS_GROUPS:
        drift.assert_within_float32_floor(np.abs(R["obs_dev"][..., sl] - R["obs_ref"][..., sl]).max(axis=-1)[ok],
                                          np.abs(R["obs_f32"][..., sl] - R["obs_ref"][..., sl]).max(axis=-1)[ok], "push step " + what)
    assert (R["done_dev"] == R["done_ref"]).mean() > 0.97 and R["done_ref"].sum() > pl.N


# ---- 7. nothing else moves -------------------------------------------------------------------------------------------------------------
def run_side_by_side(envs, steps=40, extra=(), seed=4):
    """envs: {name: env}, "none" the reference.  Stress actions from the reference's observation; observations, rewards and dones of
    every env equal the reference's bit for bit at every step, `extra` buffers likewise against the env named "base"; at the end the
    records, the counters and the episode log."""
    import torch
    ref = envs["none"]
    obs = {k: e.reset() for k, e in envs.items()}
    rng = np.random.RandomState(seed)
    for k in range(steps):
        a = stress(ref, obs["none"], rng)
        out = {name: e.step(a) for name, e in envs.items()}
        obs = {name: o[0] for name, o in out.items()}
        for name in envs:
            assert all(torch.equal(bits(out[name][j]), bits(out["none"][j])) for j in range(3)), (k, name)
        for x in extra:
            for name in envs:
                if name not in ("none", "base") and getattr(envs[name], x) is not None:
                    assert torch.equal(bits(getattr(envs[name], x)), bits(getattr(envs["base"], x))), (k, name, x)
    episodes = int(ref.counters[_abi.CNT_EPISODES].item())
    assert episodes >= len(ref.robot_type)
    for name, e in envs.items():
        assert torch.equal(bits(e.state), bits(ref.state)) and torch.equal(e.counters, ref.counters), name
        la, lb = e.ep_log.cpu().numpy(), ref.ep_log.cpu().numpy()
        assert la[np.lexsort(la.T[::-1])].tobytes() == lb[np.lexsort(lb.T[::-1])].tobytes(), name
    return episodes


def test_a_push_that_never_kicks_is_the_env_without_push():
    """37 robots x 40 stress-action steps with auto-reset, short episodes and the randomiser on: prob 0 with the outputs bound, and
    prob 1 behind a grace period of 1000 steps, are bit for bit the env without push (observations, rewards, dones, records, counters,
    episode log); their rows are zero and the padding rows keep the sentinel."""
    kw = dict(auto_reset=True, config_overrides=short_episodes())
    envs = {"none": mixed_env(37, **kw), "zero": mixed_env(37, push=dict(prob=0.0, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), **kw),
            "grace": mixed_env(37, push=dict(prob=1.0, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5, grace_steps=1000), **kw)}
    assert not envmod.push_on(envs["zero"].push) and envs["zero"].push_out is None
    bufs = {name: own_rows(envs[name], 37) for name in ("zero", "grace")}
    run_side_by_side(envs)
    for name, b in bufs.items():
        rows = b.cpu().numpy()
        assert not rows[:37].any() and (rows[37:] == SENTINEL).all(), name
    for e in envs.values():
        e.close()


def test_with_every_other_feature_on_a_push_of_probability_zero_changes_no_buffer():
    """Reward terms, contact outputs, actuator outputs and limits, sensor noise, a randomiser table and the params buffer on two envs,
    one of them with push at prob 0 and the outputs bound (the push variant against the randomiser variant): the same bits in
    observations, rewards, dones, records, counters, the episode log and every one of those buffers and side logs."""
    cfg = {"mass": [0.8, 1.2], "base mass": [0.9, 1.1], "motor strength": [0.8, 1.2], "latency": [0.0, 0.04], "leg weaken": [0.5, 1.0]}
    kw = dict(auto_reset=True, config_overrides=short_episodes(), reward_terms=True, contact_outputs=True, actuator_outputs=True,
              torque_limits=al.mixed_limits(), observation_noise_stdev=[0.01, 0.0, 0.0, 0.02, 0.1], randomizer_config=cfg, randomizer_params=True)
    envs = {"none": mixed_env(37, **kw), "base": mixed_env(37, **kw),
            "push": mixed_env(37, push=dict(prob=0.0, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True, **kw)}
    assert envs["push"].push_out is not None and envs["base"].push_out is None
    extra = ("reward_terms", "episode_term_sums", "contact_out", "episode_contact", "actuator_out", "episode_actuator", "randomizer_rows")
    episodes = run_side_by_side(envs, extra=extra)
    A, B = envs["push"], envs["base"]
    for log in ("term_log", "contact_log", "actuator_log"):
        assert canonical_log(A, episodes, getattr(A, log)) == canonical_log(B, episodes, getattr(B, log)), log
    assert not A.push_out.any()
    for e in envs.values():
        e.close()


def test_after_dropping_the_pushes_the_env_is_the_one_that_never_had_them():
    """Pushes on and outputs bound, stepped (kicks land), then set_push(None) and bind_push_outputs(False): reset + 20 steps give
    observations, rewards, dones, records and the log bit-identical to an env that never had them, and the old buffer, filled with a
    sentinel, stays untouched.  Both setters bump launch_params_generation."""
    import torch
    kw = dict(auto_reset=True, config_overrides=short_episodes())
    a = mixed_env(37, push=dict(pl.PUSH, prob=1.0), push_outputs=True, **kw)
    b = mixed_env(37, **kw)
    oa = a.reset()
    a.step(stress(a, oa, np.random.RandomState(1)))
    assert (a.push_out[:, 6] == 1).all() and (a.push_out[:, 7] == 1).all()
    old = a.push_out
    gen = a.launch_params_generation
    a.set_push(None)
    assert a.launch_params_generation == gen + 1 and not envmod.push_on(a.push)
    a.bind_push_outputs(False)
    assert a.push_out is None and a.launch_params_generation == gen + 2
    old.fill_(SENTINEL)
    a.counters.zero_(); a.ep_log.zero_()
    a.state.copy_(b.state)                                   # the records as they were before the first reset
    oa, ob = a.reset(), b.reset()
    rng = np.random.RandomState(4)
    for k in range(20):
        act = stress(b, ob, rng)
        (oa, ra, da, _), (ob, rb, db, _) = a.step(act), b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
    assert torch.equal(bits(a.state), bits(b.state)) and torch.equal(a.counters, b.counters)
    la, lb = a.ep_log.cpu().numpy(), b.ep_log.cpu().numpy()
    assert la[np.lexsort(la.T[::-1])].tobytes() == lb[np.lexsort(lb.T[::-1])].tobytes() and int(a.counters[_abi.CNT_EPISODES].item()) >= 37
    assert bool((old == SENTINEL).all())
    a.close(); b.close()


# ---- 8. push alone selects the variant -------------------------------------------------------------------------------------------------
def test_push_alone_selects_the_variant():
    """An env with only push= set (prob 0.02: a robot sees no kick in 40 steps with probability 0.45) against the default env, the same
    actions: a robot's record is bit for bit the default env's up to its first kicked step and differs after that step; robots that are
    never kicked stay bit-identical through the whole run, auto-resets included.  The episode length is fixed (ep_len_start =
    ep_len_end), so that no robot's time limit depends on when OTHER robots' episodes end."""
    import torch
    over = dict(short_episodes(), ep_len_start=12, ep_len_end=12)
    kw = dict(seed=pl.SEED, auto_reset=True, config_overrides=over)
    push = dict(prob=0.02, lin_vel=(0.3, 0.6), lin_vel_z=0.2, ang_vel=0.5)
    a, b = mixed_env(37, push=push, **kw), mixed_env(37, **kw)
    assert a.push_out is None
    L = ol.lib()
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    rng = np.random.RandomState(4)
    clean = np.ones(37, dtype=bool)                         # not kicked so far
    first = 0
    for k in range(40):
        kicked, _, _ = pl.kicks(L, a.push, pl.SEED, gpu_state64(a), a.layout)
        act = stress(b, ob.clone(), rng)
        a.step(act); b.step(act)
        same = (bits(a.state) == bits(b.state)).all(dim=1).cpu().numpy()
        now = clean & kicked
        assert same[clean & ~kicked].all(), k
        assert not same[now].any(), k                       # the first kick moves the record
        first += int(now.sum())
        clean &= ~kicked
    assert first >= 8 and clean.sum() >= 8, (first, int(clean.sum()))
    assert int(b.counters[_abi.CNT_EPISODES].item()) >= 37 * 3
    a.close(); b.close()


# ---- 9. stream independence ------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_and_follow_the_seed():
    import torch
    push = dict(pl.PUSH, prob=0.5)

    def run(n, seed, steps):
        env = mixed_env(n, seed=seed, auto_reset=True, push=push, push_outputs=True)
        env.reset()
        act = torch.zeros(n, 12, device=env.device)
        rows = []
        for _ in range(steps):
            env.step(act)
            rows.append(env.push_out.cpu().numpy().copy())
        env.close()
        return np.stack(rows)
    small, big, twin, other = run(5, 3, 1), run(37, 3, 10), run(37, 3, 10), run(37, 9, 10)
    assert small[0, :, 6].sum() >= 1 and np.array_equal(small[0].view(np.uint32), big[0, :5].view(np.uint32))
    assert np.array_equal(big.view(np.uint32), twin.view(np.uint32))
    assert not np.array_equal(big[..., 6], other[..., 6]) and not np.array_equal(big[..., :6], other[..., :6])


# ---- 10. refusals on a live handle -----------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import torch
    from openroborl_amd.env import VecQuadrupedEnv
    env = mixed_env(5)
    L, h = env.L, env.h
    good = dict(prob=0.25, lin_lo=0.2, lin_hi=0.6, lin_z=0.2, ang=0.5, grace_steps=0)
    for field, bad, needle in (("prob", float("nan"), b"prob"), ("prob", 1.5, b"prob"), ("prob", -0.1, b"prob"), ("lin_lo", -0.2, b"lin_lo"),
                               ("lin_lo", 0.7, b"lin_lo > lin_hi"), ("lin_hi", float("inf"), b"lin_hi"), ("lin_hi", 100.5, b"lin_hi"),
                               ("lin_z", float("nan"), b"lin_z"), ("lin_z", -1.0, b"lin_z"), ("lin_z", 101.0, b"lin_z"), ("ang", -0.5, b"ang"),
                               ("ang", 1e3, b"ang"), ("grace_steps", -1, b"grace_steps")):
        s = _abi.OrrPush(**dict(good, **{field: bad}))
        assert L.orr_set_push(h, C.byref(s)) == -1 and needle in L.orr_last_error() and b"orr_set_push" in L.orr_last_error(), (field, bad)
    buf = torch.full((5, _abi.PUSH_ROW), SENTINEL, device=env.device)
    assert L.orr_bind_push_outputs(h, buf.data_ptr() + 4) == -1 and b"16-byte aligned" in L.orr_last_error()
    env.reset(); env.step(torch.zeros(5, 12, device=env.device))               # nothing changed: the default kernels run
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert L.orr_set_push(h, C.byref(_abi.OrrPush(**good))) == 0 and L.orr_set_push(h, None) == 0 and L.orr_bind_push_outputs(h, None) == 0
    env.close()
    # friction anchors before
    kw = dict(num_robot=8, robot="laikago", motion_file="laikago_pace", mode="test", enable_randomizer=False, seed=5)
    anchors = {"laikago": {"friction_anchor": 1}}
    with pytest.raises(RuntimeError, match="orr_set_push: friction anchors"):
        VecQuadrupedEnv(push=dict(prob=0.1, lin_vel=(0.1, 0.2)), model_overrides=anchors, **kw)
    with pytest.raises(RuntimeError, match="orr_bind_push_outputs: friction anchors"):
        VecQuadrupedEnv(push_outputs=True, model_overrides=anchors, **kw)
    anchored = VecQuadrupedEnv(model_overrides=anchors, **kw)
    assert anchored.L.orr_set_push(anchored.h, None) == 0 and anchored.L.orr_bind_push_outputs(anchored.h, None) == 0      # turning off is fine
    anchored.set_push(dict(prob=0.0, lin_vel=(0.1, 0.2)))                      # and so is a push that is off
    with pytest.raises(RuntimeError, match="friction anchors"):
        anchored.set_push(dict(prob=0.1, lin_vel=(0.1, 0.2)))
    with pytest.raises(RuntimeError, match="friction anchors"):
        anchored.bind_push_outputs(True)
    assert anchored.push_out is None and not envmod.push_on(anchored.push)
    anchored.reset(); anchored.step(torch.zeros(8, 12, device=anchored.device))               # nothing changed: the anchor kernels run
    anchored.close()
    # friction anchors after: every launch is refused and nothing runs
    env = VecQuadrupedEnv(push=dict(prob=1.0, lin_vel=(0.1, 0.2)), push_outputs=True, **kw)
    env.reset()
    act = torch.zeros(8, 12, device=env.device)
    env.step(act)
    assert (env.push_out[:, 6] == 1).all()
    t = robots.ROBOT_TYPE_ID["laikago"]
    m = dict(env.models[t])
    m["friction_anchor"] = 1
    assert env.L.orr_set_model(env.h, t, C.byref(robots.to_struct(m))) == 0
    torch.cuda.synchronize()
    before = env.state.clone(), env.push_out.clone()
    with pytest.raises(RuntimeError, match=r"orr_reset: friction anchors \(orr_model::friction_anchor\) and pushes"):
        env.reset()
    with pytest.raises(RuntimeError, match=r"orr_step: friction anchors .* pushes"):
        env.step(act)
    torch.cuda.synchronize()
    assert torch.equal(bits(env.state), bits(before[0])) and torch.equal(env.push_out, before[1])
    env.close()


def test_the_generation_counter_and_the_legacy_list_env():
    from openroborl_amd.env import LegacyListEnv
    env = mixed_env(5, auto_reset=False)
    gen = env.launch_params_generation
    env.set_push(dict(prob=0.5, lin_vel=(0.1, 0.2)))
    env.bind_push_outputs(True)
    assert env.launch_params_generation == gen + 2
    env.set_push(None); env.bind_push_outputs(False)
    assert env.launch_params_generation == gen + 4 and env.push_out is None
    leg = LegacyListEnv(env, push=dict(prob=1.0, lin_vel=(0.3, 0.3), grace_steps=1), push_outputs=True)
    assert env.push_out is not None and envmod.push_on(env.push) and env.push.grace_steps == 1
    leg.reset()
    leg.step([np.zeros(12) for _ in range(5)])
    assert not leg.push_out.any()                                                 # the grace period: EP_STEP 0
    leg.step([np.zeros(12) for _ in range(5)])
    rows = leg.push_out.cpu().numpy()
    assert (rows[:, 6] == 1).all() and np.allclose(np.hypot(rows[:, 0], rows[:, 1]), 0.3, atol=1e-6) and not rows[:, 2:6].any()
    with pytest.raises(ValueError, match="prob"):
        LegacyListEnv(env, push=dict(prob=2.0))
    with pytest.raises(ValueError, match="push_outputs"):
        LegacyListEnv(env, push_outputs=1)
    env.close()
