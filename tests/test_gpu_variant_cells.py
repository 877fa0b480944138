"""Every cell of the C-ABI's variant tables launches (orr_kernels.hip: step_launcher, reset_launcher, physics_launcher,
replay_step_launcher).  Which variant a handle gets is the pure rule of csrc/orr_variants.h, walked without a GPU in
tests/test_variant_rule_cpu.py; what a CPU cannot see is that the launcher behind each answer exists and runs.  One small env per
variant of the env step, six robots (two waves, the second one partial), through all five entry points."""
import numpy as np
import pytest

from tests import gpu_kit

pytestmark = pytest.mark.gpu

N = 6
ANCHOR = {"laikago": {"friction_anchor": 1}}
PUSH = dict(prob=0.5, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5)

# name -> (constructor keywords, attributes of the per-step outputs that the feature owns).  The two-clip row has a switch interval
# too: that is what selects the clip-set cells of the two replays.
ROWS = {
    "default": ({}, ()),
    "two_wave": ({}, ()),
    "anchor": (dict(model_overrides=ANCHOR), ()),
    "clips": (dict(files=["laikago_pace", "laikago_trot"], clip_time_min=0.3, clip_time_max=0.8), ()),
    "noise": (dict(perturb_init_state_prob=1.0, tar_obs_noise=[0.1]), ()),
    "terms": (dict(reward_terms=True), ("reward_terms",)),
    "contacts": (dict(contact_outputs=True), ("contact_out",)),
    "contacts_terms": (dict(contact_outputs=True, reward_terms=True), ("contact_out", "reward_terms")),
    "actuator": (dict(actuator_outputs=True), ("actuator_out",)),
    "sensor": (dict(observation_noise_stdev=[0.02, 0.0, 0.0, 0.03, 0.1]), ()),
    "randomizer": (dict(mode="train", enable_randomizer=True, randomizer_config="all_params", randomizer_params=True), ()),
    "push": (dict(push=PUSH, push_outputs=True), ("push_out",)),
}


def finite(t):
    return bool(t.isfinite().all())


def written_part(env, name):
    """The words of an output that every step writes afresh: all of them, but for the last word of a push row, the episode's kick count,
    which the step carries on from the row itself"""
    t = getattr(env, name)
    return t[:, :7] if name == "push_out" else t


@pytest.mark.parametrize("row", list(ROWS))
def test_every_entry_point_launches(row, monkeypatch):
    import torch
    if row == "two_wave":
        monkeypatch.setenv("ORR_STEP_WAVES_PER_EU", "2")            # read when the handle is created
    kw, owned = ROWS[row]
    kw = dict(kw)
    files = kw.pop("files", "laikago_pace")
    env, twin = gpu_kit.make_env(N, files, **kw), gpu_kit.make_env(N, files, auto_reset=False, **kw)
    dev = env.device
    rng = np.random.RandomState(4)

    # reset, two steps, the debug physics
    if env.randomizer_rows is not None:
        env.randomizer_rows.fill_(float("nan"))
    obs = env.reset()
    torch.cuda.synchronize(dev)
    assert finite(obs)
    if env.randomizer_rows is not None:                              # every reset writes the new episode's row
        rows = env.randomizer_rows[:, :31]
        assert finite(rows) and bool(((rows >= 0.0) & (rows < 4.0)).all())
    if env.multi_clip:
        assert set(env.active_clip_ids().cpu().tolist()) <= {0, 1}
    for _ in range(2):
        for name in owned:
            written_part(env, name).fill_(float("nan"))
        obs, reward, done, _ = env.step(gpu_kit.stress(env, obs, rng))
        torch.cuda.synchronize(dev)
        assert finite(obs) and finite(reward) and bool((done <= 1).all())
        for name in owned:
            assert finite(written_part(env, name)), name
    if env.contact_out is not None:
        env.contact_out.fill_(float("nan"))
    fall = env.debug_physics(torch.zeros((N, 12), dtype=torch.float32, device=dev), 1)
    torch.cuda.synchronize(dev)
    assert bool((fall <= 1).all()) and finite(env.state[:, 0:37])
    if env.contact_out is not None:                                  # the debug physics sums the sub-step's impulses too
        assert finite(env.contact_out)

    # the parity replays, on the twin without auto-reset: the reset with given draws, one step that holds the robots where they are
    uni = rng.uniform(0.0, 1.0, (N, 28)).astype(np.float32)
    uni[:, 26] = 0.0                                                 # reference state initialisation for every robot
    obs = twin.replay_reset(torch.from_numpy(uni).to(dev))
    torch.cuda.synchronize(dev)
    assert finite(obs)
    traj = twin.state[:, None, 0:37].repeat(1, twin.cfg.action_repeat, 1).contiguous()
    eff = torch.zeros((N, 2, 8, 3), dtype=torch.float32, device=dev)
    fall = torch.zeros(N, dtype=torch.uint8, device=dev)
    tau = torch.full((N, twin.cfg.action_repeat, 12), float("nan"), dtype=torch.float32, device=dev)
    replay_owned = [name for name in owned if name in ("reward_terms", "actuator_out")]      # the replays have no impulses and no pushes
    for name in replay_owned:
        getattr(twin, name).fill_(float("nan"))
    obs, reward, done = twin.replay_step(torch.zeros((N, 12), dtype=torch.float32, device=dev), traj, eff, fall, tau)
    torch.cuda.synchronize(dev)
    assert finite(obs) and finite(reward) and finite(tau) and bool((done <= 1).all())
    for name in replay_owned:
        assert finite(getattr(twin, name)), name
    env.close()
    twin.close()
