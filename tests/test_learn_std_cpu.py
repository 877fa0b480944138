"""The learned action std's host side without a GPU: ppo.ActorCritic(learn_std=True) and model/pi/logstd:0, the per-dimension log-probability
and sampler on the torch path, ppo.PPO's entropy bonus, diagnostics and clamp, the zip round trip, and the refusals of the two entry points
(include/openroborl_learner.h: orr_ppo_head_logstd, orr_gauss_prepare)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from openroborl_amd import _abi, _lib, policy as pol, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "model/pi/logstd:0"


def _uneven_log_std():
    return (math.log(0.125) + torch.linspace(-0.7, 0.7, 12)).reshape(1, 12)


def _batch(model, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, 160, generator=g)
    noise = torch.randn(n, 12, generator=g)
    return obs, noise, torch.randn(n, generator=g)


@pytest.mark.parametrize("seed", [0, 7])
def test_the_parameter_is_filled_not_drawn(seed):
    plain, learn = ppo.ActorCritic("cpu", seed=seed), ppo.ActorCritic("cpu", seed=seed, learn_std=True, std=0.2)
    assert KEY not in plain.p and not plain.learn_std and plain.std == pol.PI_STD
    assert learn.learn_std and sorted(set(learn.p) - set(plain.p)) == [KEY]
    for k in plain.p:
        assert torch.equal(plain.p[k], learn.p[k]), k
    want = torch.full((1, 12), math.log(0.2), dtype=torch.float32)
    assert tuple(learn.p[KEY].shape) == (1, 12) and torch.equal(learn.p[KEY].detach(), want) and learn.p[KEY].requires_grad
    assert learn.log_std is learn.p[KEY]
    std = learn.std                                      # the host's view, for logging
    assert isinstance(std, np.ndarray) and std.shape == (12,) and np.allclose(std, 0.2, rtol=1e-6)
    with pytest.raises(AttributeError, match="mark_updated"):
        learn.std = 0.3
    with pytest.raises(AttributeError):
        plain.log_std
    plain.std = 0.3                                      # a fixed std stays a plain number
    assert plain.std == 0.3
    # with params the presence of the key decides, whatever the argument says
    again = ppo.ActorCritic("cpu", params=learn.state_dict(), learn_std=False)
    assert again.learn_std and torch.equal(again.p[KEY].detach(), want) and KEY not in again.extra
    assert not ppo.ActorCritic("cpu", params=plain.state_dict(), learn_std=True).learn_std


def test_log_prob_and_act_use_the_per_dimension_std():
    model = ppo.ActorCritic("cpu", seed=2, learn_std=True)
    with torch.no_grad():
        model.p[KEY].copy_(_uneven_log_std())
    obs, noise, _ = _batch(model, 257)
    clipped, raw, value = model.act(obs, noise=noise)
    with torch.no_grad():
        mu = model.mean(obs)
        assert torch.equal(raw, mu + model.p[KEY].exp() * noise)
        assert torch.equal(clipped, raw.clamp(-2.0 * math.pi, 2.0 * math.pi)) and torch.equal(value, model.value(obs))
        assert torch.equal(model.act(obs, deterministic=True)[1], mu)
        ls = model.p[KEY].double()
        z = (raw.double() - mu.double()) * torch.exp(-ls)
        want = -0.5 * (z * z).sum(dim=1) - ls.sum() - 6.0 * math.log(2.0 * math.pi)
        got = model.log_prob(obs, raw)
    assert (got.double() - want).abs().max().item() < 1e-5
    # ... which is what the sampler's noise says: a - mean = exp(log_std) * noise
    assert (want - (-0.5 * (noise.double() ** 2).sum(dim=1) - ls.sum() - 6.0 * math.log(2.0 * math.pi))).abs().max().item() < 1e-4


def test_the_entropy_bonus_alone_moves_log_std_up_by_lr():
    # Adam's first step is lr * g / (|g| + eps): lr * sign up to eps / |g|.  |g| = ent_coef = 0.01, so the learner's default eps = 1e-5 would
    # sit exactly on the 1e-3 lr bound; eps = 1e-8 (torch's default) leaves 1e-6 lr, and lr = 1e-2 keeps the bound (1e-5) well above the
    # float32 spacing of log 0.125 (2.4e-7)
    lr = 1e-2
    model = ppo.ActorCritic("cpu", seed=5, learn_std=True)
    obs, noise, ret = _batch(model, 128, seed=1)
    _, raw, _ = model.act(obs, noise=noise)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    learner = ppo.PPO(model, lr=lr, adam_eps=1e-8, minibatch=128, ent_coef=0.01)
    stats = learner.update(obs, raw, torch.zeros(128), ret, epochs=1)
    # zero advantages: the surrogate is constant, the loss's only pull on log_std is - ent_coef dH / d log_std = - ent_coef
    moved = (model.p[KEY].detach() - before[KEY]).reshape(-1)
    assert (moved - lr).abs().max().item() < 1e-3 * lr, moved
    for k in before:
        if k.startswith("model/pi") and k != KEY:
            assert torch.equal(model.p[k].detach(), before[k]), k
            assert model.p[k].grad is not None and bool((model.p[k].grad == 0).all()), k
    assert not torch.equal(model.p["model/vf/b:0"].detach(), before["model/vf/b:0"])     # the critic did learn
    assert stats.shape == (5,) and np.isfinite(stats).all() and len(ppo.STAT_NAMES) == 5
    assert abs(stats[2] - (float(before[KEY].double().sum()) + 6.0 * math.log(2.0 * math.pi * math.e))) < 1e-5
    assert stats[0] == 0.0 and abs(stats[3]) < 1e-6 and stats[4] == 0.0      # old policy = this policy: ratio 1, nothing clipped


def test_log_std_is_clamped_after_the_step():
    lo, hi = math.log(0.1), math.log(0.13)
    for ent_coef in (1.0, -1.0):                         # pushed up into hi, pushed down into lo
        model = ppo.ActorCritic("cpu", seed=5, learn_std=True)
        obs, noise, ret = _batch(model, 64, seed=2)
        _, raw, _ = model.act(obs, noise=noise)
        ppo.PPO(model, lr=0.5, minibatch=64, ent_coef=ent_coef, log_std_bounds=(lo, hi)).update(obs, raw, torch.zeros(64), ret)
        ls = model.p[KEY].detach()
        assert bool((ls >= lo).all()) and bool((ls <= hi).all())
        assert torch.equal(ls, torch.full_like(ls, hi if ent_coef > 0 else lo))


def test_zip_round_trip(tmp_path):
    import json
    import zipfile
    model = ppo.ActorCritic("cpu", seed=1, learn_std=True)
    with torch.no_grad():
        model.p[KEY].copy_(_uneven_log_std())
    path = str(tmp_path / "learn_std.zip")
    pol.save_parameters_zip(path, model.state_dict())
    with zipfile.ZipFile(path) as z:
        names = json.loads(z.read("parameter_list"))
    assert names[:14] == [n for n, _ in pol.SB_PARAMETER_LIST] and names[14:] == [KEY]      # behind the reference's fourteen
    loaded = ppo.ActorCritic("cpu", params=pol.load_parameters(path))
    assert loaded.learn_std and set(loaded.p) == set(model.p)
    for k in model.p:
        assert torch.equal(loaded.p[k].detach(), model.p[k].detach()), k
    # the inference policy samples with it
    mlp = pol.MLPPolicy.from_file(path, "cpu")
    assert mlp.learn_std and torch.equal(mlp.log_std, model.p[KEY].detach())
    obs = torch.randn(33, 160, generator=torch.Generator().manual_seed(3))
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    with torch.no_grad():
        _, raw, _ = mlp.act(obs, generator=g1)
        assert torch.equal(raw, mlp.mean(obs) + model.p[KEY].exp() * torch.randn(33, 12, generator=g2))
        assert (mlp.log_prob(obs, raw) - model.log_prob(obs, raw)).abs().max().item() < 1e-5
    # a zip without the key is a fixed-std model, as ever
    plain_path = str(tmp_path / "plain.zip")
    pol.save_parameters_zip(plain_path, ppo.ActorCritic("cpu", seed=1).state_dict())
    with zipfile.ZipFile(plain_path) as z:
        assert json.loads(z.read("parameter_list")) == [n for n, _ in pol.SB_PARAMETER_LIST]
    plain = ppo.ActorCritic("cpu", params=pol.load_parameters(plain_path))
    assert not plain.learn_std and KEY not in plain.p and pol.MLPPolicy.from_file(plain_path, "cpu").log_std is None
    with pytest.raises(ValueError):
        pol.save_parameters_zip(path, dict(model.state_dict(), **{KEY: np.zeros(12, dtype=np.float32)}))


def test_a_student_of_a_learn_std_teacher_keeps_the_fixed_std(tmp_path):
    """train.py's history_student: the teacher's variables go into a model built without learn_std; the log-std is carried, not trained."""
    teacher = ppo.ActorCritic("cpu", seed=1, priv_dim=48, actor_priv_dim=48, learn_std=True, std=0.3)
    path = str(tmp_path / "teacher.zip")
    pol.save_parameters_zip(path, teacher.state_dict())
    params = pol.load_parameters(path)
    assert KEY in params
    student = ppo.ActorCritic("cpu", seed=0, priv_dim=48, actor_priv_dim=48, history=ppo.HISTORY_STEPS)
    with torch.no_grad():
        for k, v in params.items():
            if k in student.p:
                student.p[k].copy_(torch.as_tensor(v))
            else:
                student.extra[k] = np.asarray(v, dtype=np.float32).copy()
    assert not student.learn_std and KEY not in student.p and KEY in student.extra and student.std == pol.PI_STD
    # ... and its zip is a fixed-std policy's: reloaded, it samples with the std it was rolled out with, not with the teacher's
    assert KEY not in student.state_dict()
    spath = str(tmp_path / "student.zip")
    pol.save_parameters_zip(spath, student.state_dict())
    again = ppo.ActorCritic("cpu", params=pol.load_parameters(spath))
    assert not again.learn_std and again.history == ppo.HISTORY_STEPS and not pol.MLPPolicy.from_file(spath, "cpu").learn_std
    # the distillation learners leave a log-std alone: it has no optimiser state and does not move
    model = ppo.ActorCritic("cpu", seed=2, learn_std=True)
    learner = ppo.Distill(model, lr=1e-2, minibatch=32)
    assert all(p is not model.p[KEY] for group in learner.opt.param_groups for p in group["params"])
    before = model.p[KEY].detach().clone()
    learner.update(torch.randn(32, 160), torch.randn(32, 12))
    assert torch.equal(model.p[KEY].detach(), before)
    # a teacher loaded from such a zip labels with its means
    loaded = ppo.ActorCritic("cpu", params=params)
    obs, priv = torch.randn(8, 160), torch.randn(8, 48)
    with torch.no_grad():
        assert torch.equal(loaded.mean(obs, priv), teacher.mean(obs, priv))


def test_refusals_and_declarations():
    hdr = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    assert re.search(r"int32_t orr_ppo_head_logstd\(const float\* mean, const float\* value, const float\* batch, const float\* log_std, int32_t m,", hdr)
    assert re.search(r"int32_t orr_gauss_prepare\(const float\* noise, const float\* log_std, float\* scaled, float\* logp, int32_t n, void\* stream\);", hdr)
    assert "orr_ppo_head_logstd" in _lib.EXPORTS and "orr_gauss_prepare" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(_abi.PPO_HEAD_LOGSTD_ARGS) == 16 and len(_abi.GAUSS_PREPARE_ARGS) == 6
    L = _lib.load()
    assert L.orr_ppo_head_logstd.argtypes == _abi.PPO_HEAD_LOGSTD_ARGS and L.orr_gauss_prepare.argtypes == _abi.GAUSS_PREPARE_ARGS
    # host-side refusals (no launch happens on these paths)
    assert L.orr_ppo_head_logstd(None, None, None, None, 16, 0.2, 0.5, 0.01, None, None, None, None, None, None, None, None) == -1
    assert b"orr_ppo_head_logstd" in L.orr_last_error()
    assert L.orr_ppo_head_logstd(16, 16, 16, 16, 0, 0.2, 0.5, 0.01, 16, 16, 16, 16, 16, 16, 16, None) == -1 and b"orr_ppo_head_logstd" in L.orr_last_error()
    assert L.orr_ppo_head_logstd(16, 16, 20, 16, 4, 0.2, 0.5, 0.01, 16, 16, 16, 16, 16, 16, 16, None) == -1
    assert b"orr_ppo_head_logstd" in L.orr_last_error() and b"16-byte aligned" in L.orr_last_error()
    assert L.orr_gauss_prepare(None, None, None, None, 4, None) == -1 and b"orr_gauss_prepare" in L.orr_last_error()
    assert L.orr_gauss_prepare(16, 16, 32, None, 0, None) == -1 and b"orr_gauss_prepare" in L.orr_last_error()
    assert L.orr_gauss_prepare(16, 16, 36, None, 4, None) == -1 and b"16-byte aligned" in L.orr_last_error()
    assert L.orr_gauss_prepare(4096, 16, 4096 + 48, None, 4, None) == -1 and b"overlap" in L.orr_last_error()      # rows 1.. of noise
    # an entropy bonus on a fixed std would have no gradient
    fixed = ppo.ActorCritic("cpu", seed=0)
    with pytest.raises(ValueError):
        ppo.PPO(fixed, ent_coef=0.01)
    assert ppo.PPO(fixed).update(torch.randn(16, 160), torch.randn(16, 12), torch.randn(16), torch.randn(16)).shape == (2,)
    with pytest.raises(ValueError):
        ppo.PPO(ppo.ActorCritic("cpu", seed=0, learn_std=True), log_std_bounds=(0.0, -1.0))
