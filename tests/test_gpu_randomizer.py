"""The table-driven, controllable randomiser on the MI355X (orr_set_randomizer, orr_bind_randomizer_params;
ControllableEnvRandomizerFromConfig): the randomiser variants of the kernels (csrc/orr_kernels_randomizer.hip) apply up to ten parameters
per episode, each with its own range, and write or - suspended - apply the episode's normalised samples per robot.  Every draw is keyed
by the episode's Philox stream, so the host predicts each record word from the oracle's stream (tests/randomizer_kit.stream_rows,
env.randomizer_apply); the reference's own class, driven with the same samples, is the fixture tests/golden/randomizer_laikago.npz.

Bound of a randomised word against the float64 prediction: the device computes fmaf(u, hi - lo, lo) from the float32 bounds that the
prediction uses too and a u that float32 holds exactly - two float32 roundings, one of hi - lo (at most 2^-24 max(|lo|, |hi|) times u < 1:
|hi - lo| <= max(|lo|, |hi|) for bounds >= 0) and one of the result (at most 2^-24 max(|lo|, |hi|)): 2^-23 max(|lo|, |hi|) of the parameter
that wrote the word.

66 robots: 17 waves, the last one with two padding lane groups."""
import ctypes as C
import os

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, robots
from openroborl_amd import env as envmod
from tests import oracle_lib as ol, randomizer_kit as kit
from tests.gpu_kit import make_env

pytestmark = pytest.mark.gpu

N, SEED = 66, 5
FIELDS = ("STRENGTH", "MASS_RATIO", "INERTIA_RATIO", "KNEE_FRICTION", "LATENCY", "FOOT_MU")
P = {n: i for i, n in enumerate(_abi.RAND_PARAM_NAMES)}


def cases():
    return kit.load_cases(np.load(os.path.join(ol.GOLDEN, "randomizer_laikago.npz")))


def rand_env(n=N, **kw):
    kw.setdefault("mode", "train")
    kw.setdefault("enable_randomizer", True)
    kw.setdefault("seed", SEED)
    return make_env(n, **kw)


def words(env):
    """the randomised record words, as float32 arrays on the host"""
    return {f: env.field(f).cpu().numpy().copy() for f in FIELDS}


def stream(env):
    I = lambda k: env.field_int(k)[:, 0].cpu().numpy().astype(np.int64)
    return I("ROBOT_INDEX"), I("EPISODE_IDX")


def bounds(spec):
    """2^-23 max(|lo|, |hi|) of the parameter that writes each word last (module docstring), per field [k]"""
    b = lambda name: 2.0 ** -23 * max(abs(float(spec.lo[P[name]])), abs(float(spec.hi[P[name]])))
    last = lambda *names: next((b(n) for n in reversed(names) if spec.enabled[P[n]]), 0.0)
    return {"STRENGTH": np.full(12, last("global motor strength", "leg weaken", "motor strength", "single leg weaken")),
            "MASS_RATIO": np.array([last("base mass", "mass"), last("mass")]), "INERTIA_RATIO": np.full(2, last("inertia")),
            "KNEE_FRICTION": np.full(4, last("joint friction")), "LATENCY": np.full(1, last("latency")), "FOOT_MU": np.full(1, last("lateral friction"))}


def check(spec, rows, before, after, sel, what):
    """The robots `sel` of `after` hold randomizer_apply(spec, rows) within the derived bound; the words that no enabled parameter
    writes are bit for bit those of `before`; with a weakening parameter as the last writer the other legs are exactly 1.0.
    -> (words compared with a prediction, words bit-identical to before)"""
    pred = envmod.randomizer_apply(spec, rows)
    bd = bounds(spec)
    hit = kept = 0
    for f in FIELDS:
        got, bef, w = after[f][sel], before[f][sel], ~np.isnan(pred[f])
        err = np.abs(got.astype(np.float64) - pred[f])
        assert (err[w] <= np.broadcast_to(bd[f], err.shape)[w]).all(), "%s %s: error %.3g above the bound %.3g" % (what, f, err[w].max(), bd[f].max())
        assert (got.view(np.uint32)[~w] == bef.view(np.uint32)[~w]).all(), "%s %s: a word of a disabled parameter changed" % (what, f)
        hit += int(w.sum())
        kept += int((~w).sum())
    weaken = "single leg weaken" if spec.enabled[P["single leg weaken"]] else ("leg weaken" if spec.enabled[P["leg weaken"]] and not spec.enabled[P["motor strength"]] else None)
    if weaken:
        leg = np.zeros(len(rows)) if weaken == "single leg weaken" else rows[:, envmod.RAND_LEG_WORD]
        other = (np.arange(12) // 3) != leg[:, None]
        assert (after["STRENGTH"][sel][other] == np.float32(1.0)).all(), what + ": an unweakened leg is not exactly 1.0"
        assert (pred["STRENGTH"][other] == 1.0).all()
    return hit, kept


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_reset_matches_the_host_prediction():
    """orr_reset under each of the fixture's five dictionaries (set_randomizer on one env, so that a case's disabled words hold the case
    before's values): every randomised word is randomizer_apply of the stream's draws within 2^-23 max(|lo|, |hi|), disabled words keep
    their bits, unweakened legs are exactly 1.0, and the weakened leg is the integer rule's - all four legs occur."""
    import torch
    L = ol.lib()
    env = rand_env(auto_reset=False)
    for name, (cfg, _, _, _) in cases().items():
        env.set_randomizer(cfg)
        spec = envmod.randomizer_spec(cfg)
        before = words(env)
        env.reset()
        torch.cuda.synchronize()
        idx, ep = stream(env)
        rows = kit.stream_rows(L, SEED, idx, ep)
        if "leg weaken" in cfg:
            assert set(rows[:, envmod.RAND_LEG_WORD]) == {0.0, 1.0, 2.0, 3.0}, "the seed must weaken every leg somewhere"
        hit, kept = check(spec, rows, before, words(env), slice(None), "case " + name)
        assert hit == N * {"six": 22, "base_global": 13, "leg_weaken": 12, "single_leg_weaken": 12, "all_ten": 22}[name] and hit + kept == N * 22
    env.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_auto_reset_matches_the_host_prediction():
    """The inline auto-reset of orr_step: episodes of 3 steps, 7 steps; after every step the robots whose done is set hold the NEW
    episode's prediction (base mass, latency and leg weaken enabled: the seven other parameters' words keep their bits)."""
    import torch
    L = ol.lib()
    c = cases()["all_ten"][0]
    cfg = {k: c[k] for k in ("base mass", "latency", "leg weaken")}
    spec = envmod.randomizer_spec(cfg)
    env = rand_env(randomizer_config=cfg, config_overrides=dict(ep_len_start=3, ep_len_end=3))
    env.reset()
    act = torch.zeros(N, 12, device=env.device)
    checked = 0
    for s in range(7):
        before = words(env)
        _, _, done, _ = env.step(act)
        torch.cuda.synchronize()
        sel = done.cpu().numpy().astype(bool)
        after = words(env)
        for f in FIELDS:        # a robot that goes on keeps every word
            assert (after[f][~sel].view(np.uint32) == before[f][~sel].view(np.uint32)).all()
        if sel.any():
            idx, ep = stream(env)
            check(spec, kit.stream_rows(L, SEED, idx[sel], ep[sel]), before, after, sel, "step %d" % s)
            checked += int(sel.sum())
    assert checked >= 2 * N         # an episode lasts 3 steps at the most: every robot began at least two new ones
    env.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_builtin_ranges_default_kernels_against_randomizer_variants():
    """The built-in six ranges by the default kernels and, as the table "all_params", by the randomiser variants: both resets meet the
    host prediction; then, from one common state, 5 steps give bit-identical obs, reward, done and state - and again with sensor noise,
    reward terms, contact and actuator outputs on both (sensor variants against randomiser variants), those outputs included."""
    import torch
    L = ol.lib()
    spec = envmod.randomizer_spec("all_params")
    envs = [rand_env(auto_reset=False), rand_env(auto_reset=False, randomizer_config="all_params")]
    got = []
    for e in envs:
        before = words(e)
        e.reset()
        torch.cuda.synchronize()
        idx, ep = stream(e)
        check(spec, kit.stream_rows(L, SEED, idx, ep), before, words(e), slice(None), "built-in ranges")
        got.append(words(e))
    same = sum(int((got[0][f].view(np.uint32) == got[1][f].view(np.uint32)).sum()) for f in FIELDS)
    print("built-in ranges: %d of %d randomised words bit-identical between the default reset and the randomiser reset" % (same, N * 22))
    rng = np.random.RandomState(1)
    acts = [torch.from_numpy(rng.uniform(-0.3, 0.3, (N, 12)).astype(np.float32)).to(envs[0].device) for _ in range(5)]
    bits = lambda x: x.detach().cpu().numpy().view(np.uint32 if x.element_size() == 4 else np.uint8)

    def run(extra):
        start = envs[0].state_dict()
        for e in envs:
            e.load_state_dict(start)
        for k, a in enumerate(acts):
            outs = []
            for e in envs:
                o, r, d, _ = e.step(a)
                torch.cuda.synchronize()
                outs.append([bits(o).copy(), bits(r).copy(), bits(d).copy(), bits(e.state).copy()] + [bits(getattr(e, x)).copy() for x in extra])
            for name, x, y in zip(["obs", "reward", "done", "state"] + list(extra), outs[0], outs[1]):
                assert (x == y).all(), "step %d: %s differs between the two paths" % (k, name)
    run(())
    for e in envs:
        e.set_sensor_noise([0.01, 0.0, 0.0, 0.02, 0.1])
        e.bind_reward_terms(True)
        e.bind_contact_outputs(True)
        e.bind_actuator_outputs(True)
    run(("reward_terms", "episode_term_sums", "contact_out", "episode_contact", "actuator_out", "episode_actuator"))
    for e in envs:
        e.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_params_buffer_and_suspension():
    """The params buffer: a reset's rows are the draws exactly and get_randomization_parameters is -1 + 2 u; suspended, a reset and an
    auto-reset apply the rows that set_randomization_parameters wrote, within the bound of test 1, and leave them untouched; unbinding
    returns to drawing."""
    import torch
    L = ol.lib()
    cfg = cases()["all_ten"][0]
    spec = envmod.randomizer_spec(cfg)
    env = rand_env(randomizer_config=cfg, randomizer_params=True, config_overrides=dict(ep_len_start=3, ep_len_end=3))
    env.reset()
    torch.cuda.synchronize()
    idx, ep = stream(env)
    rows = kit.stream_rows(L, SEED, idx, ep)
    np.testing.assert_array_equal(env.randomizer_rows.cpu().numpy().astype(np.float64), rows)
    par = env.get_randomization_parameters()
    assert sorted(par) == sorted(cfg)
    for name, v in par.items():
        want = -1.0 + 2.0 * rows[:, envmod.RAND_ROW_WORDS[name]]
        if name == "leg weaken":
            want[:, 0] = rows[:, envmod.RAND_LEG_WORD]
        np.testing.assert_array_equal(v.cpu().numpy().astype(np.float64), want, err_msg=name)
    # an auto-reset writes the new episode's rows too
    act = torch.zeros(N, 12, device=env.device)
    ep0 = stream(env)[1]
    for _ in range(3):
        env.step(act)
    torch.cuda.synchronize()
    idx, ep = stream(env)
    assert (ep > ep0).all()         # an episode lasts 3 steps at the most
    np.testing.assert_array_equal(env.randomizer_rows.cpu().numpy().astype(np.float64), kit.stream_rows(L, SEED, idx, ep))
    # suspended: the rows are the caller's
    env.bind_randomizer_params(True, suspend=True)
    rng = np.random.RandomState(2)

    def write_rows():
        env.set_randomization_parameters({n: (np.column_stack([rng.randint(0, 4, N), rng.uniform(-1, 1, N)]) if n == "leg weaken" else
                                              rng.uniform(-1, 1, (N, sl.stop - sl.start))) for n, sl in envmod.RAND_ROW_WORDS.items()})
        torch.cuda.synchronize()
        return env.randomizer_rows.cpu().numpy().copy()
    mine = write_rows()
    assert set(mine[:, envmod.RAND_LEG_WORD]) == {0.0, 1.0, 2.0, 3.0} and ((mine[:, :28] >= 0) & (mine[:, :28] <= 1)).all()
    before = words(env)
    env.reset()
    torch.cuda.synchronize()
    check(spec, mine.astype(np.float64), before, words(env), slice(None), "suspended reset")
    assert (env.randomizer_rows.cpu().numpy().view(np.uint32) == mine.view(np.uint32)).all(), "a suspended reset wrote the rows"
    mine2 = write_rows()
    assert (mine2 != mine).any()
    before = words(env)
    ep0 = stream(env)[1]
    for _ in range(3):
        env.step(act)
    torch.cuda.synchronize()
    assert (stream(env)[1] > ep0).all()
    check(spec, mine2.astype(np.float64), before, words(env), slice(None), "suspended auto-reset")
    assert (env.randomizer_rows.cpu().numpy().view(np.uint32) == mine2.view(np.uint32)).all(), "a suspended auto-reset wrote the rows"
    # unbound: drawing again
    env.bind_randomizer_params(False)
    assert env.randomizer_rows is None
    before = words(env)
    env.reset()
    torch.cuda.synchronize()
    idx, ep = stream(env)
    check(spec, kit.stream_rows(L, SEED, idx, ep), before, words(env), slice(None), "reset after unbinding")
    env.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_replay_reset_reproduces_the_reference():
    """orr_debug_replay_reset on a handle with each of the fixture's dictionaries, draws 0..25 from the fixture's rows (the two newer
    blocks come from the Philox stream: the fixture's seed and episode): the values the reference's randomiser left on its robots, at
    tests/test_gpu_golden_task.py's bounds for the same quantities; unwritten words keep their bits."""
    import torch
    g = np.load(os.path.join(ol.GOLDEN, "randomizer_laikago.npz"))
    atol = {"LATENCY": 1e-8, "STRENGTH": 1e-6, "MASS_RATIO": 1e-6, "INERTIA_RATIO": 1e-6, "FOOT_MU": 1e-6, "KNEE_FRICTION": 1e-7}
    all_cases = cases()
    n = len(all_cases["six"][1])
    env = rand_env(n, auto_reset=False, seed=int(g["seed"]))
    for name, (cfg, rows, _, after) in all_cases.items():
        env.set_randomizer(cfg)
        env.field_int("EPISODE_IDX")[:] = int(g["episode"]) - 1
        uni = np.full((n, 28), 0.5)
        uni[:, :26] = rows[:, :26]
        before = words(env)
        env.replay_reset(torch.tensor(uni, dtype=torch.float32, device=env.device))
        torch.cuda.synchronize()
        got = words(env)
        w = {f: ~np.isnan(v) for f, v in envmod.randomizer_apply(envmod.randomizer_spec(cfg), rows).items()}
        for f in FIELDS:
            np.testing.assert_allclose(got[f][w[f]], after[f][w[f]], rtol=0, atol=atol[f], err_msg="case %s: %s" % (name, f))
            assert (got[f].view(np.uint32)[~w[f]] == before[f].view(np.uint32)[~w[f]]).all(), "case %s: %s: an unwritten word changed" % (name, f)
    env.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_change_nothing():
    """Every refused orr_set_randomizer / orr_bind_randomizer_params call returns -1 with a message that names the parameter and leaves
    the handle as it was: the same reset from the same state gives the same bits before and after them.  Friction anchors: refused by
    both calls, and by a launch when the anchors come afterwards."""
    import torch
    cfg = cases()["all_ten"][0]
    env = rand_env(randomizer_config=cfg, randomizer_params=True, auto_reset=False)
    Lh = env.L
    start = env.state_dict()
    env.reset()
    torch.cuda.synchronize()
    first, first_rows = env.state.clone(), env.randomizer_rows.clone()

    def table(**over):
        s = envmod.randomizer_spec(cfg)
        for name, (lo, hi) in over.items():
            s.lo[P[name.replace("_", " ")]], s.hi[P[name.replace("_", " ")]] = lo, hi
        return s
    nan, inf = float("nan"), float("inf")
    refused = [(dict(inertia=(nan, 1.0)), b"inertia"), (dict(mass=(0.5, inf)), b"mass"), (dict(motor_strength=(1.2, 0.8)), b"motor strength"),
               (dict(base_mass=(0.0, 1.0)), b"base mass"), (dict(mass=(-0.5, 1.0)), b"mass"), (dict(inertia=(0.0, 1.0)), b"inertia"),
               (dict(joint_friction=(-0.01, 0.05)), b"joint friction"), (dict(latency=(-0.001, 0.01)), b"latency"),
               (dict(lateral_friction=(-0.5, 1.0)), b"lateral friction"), (dict(leg_weaken=(-0.1, 0.5)), b"leg weaken"),
               (dict(single_leg_weaken=(-0.1, 0.5)), b"single leg weaken"), (dict(global_motor_strength=(-0.1, 0.5)), b"global motor strength"),
               (dict(motor_strength=(-0.1, 0.5)), b"motor strength"), (dict(latency=(0.0, 0.0421)), b"latency")]
    for over, needle in refused:
        assert Lh.orr_set_randomizer(env.h, C.byref(table(**over))) == -1, over
        assert needle in Lh.orr_last_error() and b"orr_set_randomizer" in Lh.orr_last_error(), (over, Lh.orr_last_error())
    assert Lh.orr_set_randomizer(None, C.byref(table())) == -1 and b"null handle" in Lh.orr_last_error()
    assert Lh.orr_bind_randomizer_params(None, env.randomizer_rows.data_ptr(), 0) == -1 and b"null handle" in Lh.orr_last_error()
    assert Lh.orr_bind_randomizer_params(env.h, env.randomizer_rows.data_ptr() + 4, 1) == -1 and b"16-byte aligned" in Lh.orr_last_error()
    env.load_state_dict(start)
    env.randomizer_rows.zero_()
    env.reset()
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), first.view(torch.int32)) and torch.equal(env.randomizer_rows.view(torch.int32), first_rows.view(torch.int32))
    # friction anchors
    m = dict(env.models[int(env.robot_type[0])], friction_anchor=1)
    _lib.check(Lh.orr_set_model(env.h, int(env.robot_type[0]), C.byref(robots.to_struct(m))), Lh)
    with pytest.raises(RuntimeError, match="friction anchors"):
        env.reset()
    env.close()
    anchored = rand_env(auto_reset=False, model_overrides={"laikago": {"friction_anchor": 1}})
    assert Lh.orr_set_randomizer(anchored.h, C.byref(table())) == -1 and b"friction anchors" in Lh.orr_last_error()
    rows = torch.zeros(N, _abi.RAND_ROW, device=anchored.device)
    assert Lh.orr_bind_randomizer_params(anchored.h, rows.data_ptr(), 0) == -1 and b"friction anchors" in Lh.orr_last_error()
    anchored.reset()             # still the anchor kernels
    torch.cuda.synchronize()
    anchored.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_rollout_recaptures_after_set_randomizer():
    """A GraphRollout that captured its segment before set_randomizer captures again after it (launch_params_generation moved)."""
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
    first, captured_for, generation = collector.graph, collector._captured_for, env.launch_params_generation
    assert first is not None
    env.set_randomizer({"global motor strength": [0.5, 0.5], "latency": [0.0, 0.0]})
    env.bind_randomizer_params(True)
    assert env.launch_params_generation == generation + 2
    obs = env.step(torch.zeros(n, 12, device=dev))[0]           # the variant's first launch loads its code object: not inside a capture
    env.randomizer_rows.fill_(-7.0)
    for seg in range(6):                                         # 24 steps: past the curriculum's first time limit of 20
        obs = collector.collect(obs, noise=torch.randn(T, n, 12, device=dev, generator=gen))["last_obs"]
    torch.cuda.synchronize()
    assert collector.graph is not first and collector._captured_for != captured_for
    rows = env.randomizer_rows.cpu().numpy()
    assert (rows != -7.0).all(), "the replayed segments ran no randomiser reset"
    strength = env.field("STRENGTH").cpu().numpy()
    assert (strength == np.float32(0.5)).all()
    env.close()
