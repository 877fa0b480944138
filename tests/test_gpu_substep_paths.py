"""GPU tests of the paths through one physics sub-step that depend on what the robots of ONE wave (four robots) do together: the union
mask of the wave's contact legs (a leg that no robot of the wave has down is skipped, a leg that some robot has down is worked for
all four), the joint-limit bank (bank B: taken by the whole wave when one robot has a joint inside limit_activation) with the limit rows
of the velocity update, and the second half of the velocity update's packed pair (DOFs 16 and 17, lanes 0 and 1 of a robot).

Seven robots = one full wave and one partly filled wave.  The debug physics entry (fixed torques) runs 1 and 3 sub-steps in one launch
(the second and third sub-step of a launch take the path that skips the joint-limit row setup) against the float64 oracle, at the
tolerances tests/test_gpu_parity.py uses for ONE sub-step: 2e-6 on positions, 1.5e-4 on velocities, 5e-4 on the stored impulses.

The states are built by tests/gpu_kit.py's robot_state (on tests/phys_ref.py's kinematics, the way tests/parity_inputs.py's shank_contact_inputs does it)
and not drawn with substep_parity_inputs: the cases need an exact contact pattern per robot and joints a millimetre-radian from a
bound, and each test checks that its inputs are that.  A joint-limit row only shows in the result when its impulse is non-zero, i.e.
when the joint would cross the bound within the sub-step (rate * dt > gap): the limited joints sit 0.001 rad inside the bound at
2 rad/s towards it, and every such case asserts that the oracle's velocity of that joint differs, by far more than the tolerance, from
a second oracle that makes no joint-limit rows (limit_activation below the gap).
"""
import numpy as np
import pytest

from openroborl_amd import state as statemod
from tests import oracle_lib as ol
from tests.gpu_kit import HIP, KNEE, THIGH, robot_state
from tests.test_gpu_parity import CLIP, compare_fields, gpu_state64, push_state

pytestmark = pytest.mark.gpu

N = 7                       # robots 0..3: a full wave; robots 4..6: a wave with one empty slot
PTOL, VTOL, LTOL = 2e-6, 1.5e-4, 5e-4      # test_physics_substep_parity, nsub = 1
GAP, RATE = 0.001, 2.0      # a limited joint: GAP inside its bound, moving into it at RATE (it would cross in half a sub-step of 1 ms)


def make_env(iters=None):
    from openroborl_amd.env import VecQuadrupedEnv
    over = {} if iters is None else dict(config_overrides=dict(solver_iters=iters))
    env = VecQuadrupedEnv(num_robot=N, seed=3, robot="laikago", motion_file=CLIP["laikago"], mode="test", enable_randomizer=False,
                          auto_reset=False, **over)
    orc = ol.OracleEnv(env.cfg, env.models, env.clips, N, robot_type=env.robot_type, clip_id=env.clip_id, threads=4)
    cfg0 = type(env.cfg).from_buffer_copy(env.cfg)
    cfg0.limit_activation = 0.1 * GAP                    # the same oracle without joint-limit rows for joints GAP inside a bound
    free = ol.OracleEnv(cfg0, env.models, env.clips, N, robot_type=env.robot_type, clip_id=env.clip_id, threads=4)
    env.reset(); orc.reset(); free.reset()
    return env, orc, free


@pytest.fixture(scope="module")
def pair():
    env, orc, free = make_env()
    yield env, orc, free
    env.close(); orc.close(); free.close()


def build(env, orc, specs, seed):
    """specs: one dict of robot_state's keywords per robot -> (state64 [N, stride], torques [N, 12], down [N, 4], limited [N, 12])"""
    rng = np.random.RandomState(seed)
    rows, down, lim = zip(*[robot_state(env, orc.state[i], rng, **s) for i, s in enumerate(specs)])
    st = statemod.to_float64(env.layout, statemod.from_float64(env.layout, np.array(rows)))
    tau = rng.uniform(-5, 5, (N, 12)).astype(np.float32).astype(np.float64)
    return st, tau, np.array(down), np.array(lim)


def step_oracle(orc, st, tau, nsub):
    orc.state[:] = st
    for i in range(N):
        for _ in range(nsub):
            orc.L.orc_physics_substep(orc.h, ol.P(orc.state[i]), ol.P(np.ascontiguousarray(tau[i])))


def assert_limit_rows_act(env, orc, free, st, tau, lim, what):
    """The joint-limit rows of the inputs push: after the first sub-step the oracle has every limited joint's velocity far (> 0.1
    rad/s: 600 x the tolerance) from where the oracle without joint-limit rows has it.  (One sub-step: in the second one the joint of
    that oracle is past its bound, which is inside any activation distance.)  Overwrites both oracles' states."""
    step_oracle(orc, st, tau, 1); step_oracle(free, st, tau, 1)
    sl = env.layout.sl("QD")
    d = np.abs(orc.state[:, sl] - free.state[:, sl])[lim]
    print("%s: the limit rows move their joints' velocities by %s rad/s in the first sub-step" % (what, np.round(d, 3).tolist()))
    assert lim.any() and (d > 0.1).all(), d


def run_and_compare(env, orc, st, tau, nsub, what):
    import torch
    push_state(env, st)
    env.debug_physics(torch.tensor(tau, dtype=torch.float32, device=env.device), nsub)
    step_oracle(orc, st, tau, nsub)
    g = gpu_state64(env)
    for names in (["POS", "QUAT", "Q"], ["LINVEL", "ANGVEL", "QD"], ["LAMBDA"]):
        print("%s nsub=%d %s: largest difference %.3g" % (what, nsub, "/".join(names), max(
            np.abs(g[:, env.layout.sl(f)] - orc.state[:, env.layout.sl(f)]).max() for f in names)))
    compare_fields(env, orc, ["POS", "QUAT", "Q"], atol=PTOL, rtol=PTOL, what="%s nsub=%d" % (what, nsub))
    compare_fields(env, orc, ["LINVEL", "ANGVEL", "QD"], atol=VTOL, rtol=VTOL, what="%s nsub=%d" % (what, nsub))
    compare_fields(env, orc, ["LAMBDA"], atol=LTOL, what="%s nsub=%d" % (what, nsub))


def union(down, wave):
    return down[4 * wave:4 * wave + 4].any(axis=0)


# every case: (specs of the seven robots, check(down, limited) of what the case is there for)
def case_all_feet_down():
    return [dict()] * N, lambda down, lim: down.all() and not lim.any()


def case_no_foot_down():
    return [dict(height=0.3)] * N, lambda down, lim: not down.any() and not lim.any()


def case_wave_misses_a_leg():
    # leg 1 up in all four robots of the full wave (the union misses it), down in the other wave
    return [dict(lifted=(1,))] * 4 + [dict()] * 3, lambda down, lim: (
        list(union(down, 0)) == [True, False, True, True] and union(down, 1).all())


def case_different_stance_legs():
    # every robot of the full wave lifts another leg: the union is full, and each robot is worked through a leg whose rows are inactive
    # for it; the partly filled wave lifts two legs in two robots
    specs = [dict(lifted=(i,)) for i in range(4)] + [dict(lifted=(0, 1)), dict(lifted=(2,)), dict(lifted=(3, 0))]
    return specs, lambda down, lim: union(down, 0).all() and union(down, 1).all() and (down.sum(axis=1) < 4).all()


def case_one_robot_at_a_joint_limit():
    # robot 2 only: the hip of leg 1 at its upper bound and moving into it (bank B for the whole wave; the other wave has none)
    specs = [dict() for _ in range(N)]
    specs[2] = dict(limits=((1, HIP, 1, GAP, RATE),))
    return specs, lambda down, lim: lim[2, 3 * 1 + HIP] and lim.sum() == 1 and down[[0, 1, 3]].all()


def case_two_legs_at_joint_limits():
    # robot 2: the hip of leg 0 at its upper bound and the thigh of leg 2 at its lower bound.  Leg 3's thigh and knee are joints 10 and
    # 11 = DOFs 16 and 17, the second half of the velocity update's pair: robot 1 has that thigh at its lower bound, robots 5 and 6 (the
    # other wave, neither its first robot) the knee at its lower bound and the thigh at its upper bound
    specs = [dict() for _ in range(N)]
    specs[2] = dict(limits=((0, HIP, 1, GAP, RATE), (2, THIGH, 0, GAP, RATE)))
    specs[1] = dict(limits=((3, THIGH, 0, GAP, RATE),))
    specs[5] = dict(limits=((3, KNEE, 0, GAP, RATE),))
    specs[6] = dict(limits=((3, THIGH, 1, GAP, RATE),))
    return specs, lambda down, lim: (lim[2, 0 + HIP] and lim[2, 6 + THIGH] and lim[1, 9 + THIGH] and lim[5, 9 + KNEE] and lim[6, 9 + THIGH]
                                     and lim.sum() == 5)


def case_dofs_16_and_17():
    # joints 10 and 11 (DOFs 16 and 17: the second half of the velocity update's pair, lanes 0 and 1) moving, every other joint at rest,
    # in robots that are not the first of their wave; leg 3 stands, so its contact impulses change exactly these two velocities
    qd = [0.0] * 10 + [3.0, -4.0]
    specs = [dict() for _ in range(N)]
    specs[1] = dict(qd=qd); specs[3] = dict(qd=[-x for x in qd]); specs[6] = dict(qd=qd)
    return specs, lambda down, lim: down.all()


CASES = {"all_feet_down": case_all_feet_down, "no_foot_down": case_no_foot_down, "wave_misses_a_leg": case_wave_misses_a_leg,
         "different_stance_legs": case_different_stance_legs, "one_robot_at_a_joint_limit": case_one_robot_at_a_joint_limit,
         "two_legs_at_joint_limits": case_two_legs_at_joint_limits, "dofs_16_and_17": case_dofs_16_and_17}


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_substep_paths_match_the_oracle(pair, case, nsub):
    env, orc, free = pair
    specs, check = CASES[case]()
    st, tau, down, lim = build(env, orc, specs, seed=sorted(CASES).index(case))
    assert check(down, lim), (down, lim)                                  # the inputs are what the case is about
    run_and_compare(env, orc, st, tau, nsub, case)
    lay = env.layout
    if "joint_limit" in case:
        assert_limit_rows_act(env, orc, free, st, tau, lim, case)
    if case == "no_foot_down":
        assert (orc.state[:, lay.sl("LAMBDA")] == 0.0).all()
    if case == "dofs_16_and_17":                                          # both went in non-zero and come out non-zero
        assert (st[:, lay.sl("QD")][[1, 3, 6], 10:] != 0.0).all() and (np.abs(orc.state[:, lay.sl("QD")][[1, 3, 6], 10:]) > 0.1).all()


@pytest.mark.parametrize("iters", [1, 2, 3, 4, 9, 10])
def test_substep_paths_with_other_sweep_counts(iters):
    """Both sweep loops (with and without the joint-limit bank) at iteration counts that enter and leave the three-sweeps-per-pass loop
    differently: the full wave sweeps bank B (robot 2 is at two joint limits, one of them DOF 16), the partly filled one does not."""
    env, orc, free = make_env(iters)
    try:
        assert env.cfg.solver_iters == iters
        specs = case_different_stance_legs()[0]
        specs[2] = dict(lifted=(2,), limits=((1, HIP, 1, GAP, RATE), (3, THIGH, 0, GAP, RATE)))
        st, tau, down, lim = build(env, orc, specs, seed=20 + iters)
        assert lim[2].sum() == 2 and lim.sum() == 2 and union(down, 1).all()
        for nsub in (1, 3):
            run_and_compare(env, orc, st, tau, nsub, "iters=%d" % iters)
        assert_limit_rows_act(env, orc, free, st, tau, lim, "iters=%d" % iters)
    finally:
        env.close(); orc.close(); free.close()


@pytest.mark.parametrize("which", ["contacts", "lifted_leg_and_joint_limits"])
def test_a_robots_sub_steps_do_not_depend_on_its_place_in_the_wave(pair, which):
    """The same record in all seven places (each of the four positions of the full wave, three of the other): after three sub-steps
    the seven records are the same bit for bit."""
    import torch
    env, orc, free = pair
    spec = dict() if which == "contacts" else dict(lifted=(0,), limits=((1, HIP, 1, GAP, RATE), (3, KNEE, 1, GAP, RATE)), qd=[0.4] * 10 + [3.0, -4.0])
    st, tau, down, lim = build(env, orc, [spec] * N, seed=40)
    st[:] = st[0]; tau[:] = tau[0]
    if which == "contacts":
        assert down.all() and not lim.any()
    else:     # legs 0 and 1 clear of the ground (the hip at its bound swings leg 1 up), legs 2 and 3 down, two pushing limit rows
        assert [list(r) for r in down] == [[False, False, True, True]] * N and list(np.flatnonzero(lim[0])) == [3 + HIP, 9 + KNEE]
        assert_limit_rows_act(env, orc, free, st, tau, lim, which)
    push_state(env, st)
    before = env.state.detach().cpu().numpy().view(np.int32).copy()
    assert (before == before[0]).all()
    env.debug_physics(torch.tensor(tau, dtype=torch.float32, device=env.device), 3)
    after = env.state.detach().cpu().numpy().view(np.int32)
    assert (after[0] != before[0]).any()
    for i in range(1, N):
        np.testing.assert_array_equal(after[i], after[0], err_msg="robot %d against robot 0" % i)
