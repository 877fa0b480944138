"""The privileged critic's host side without a GPU: the ABI constants and tables (include/openroborl_hip.h, openroborl_policy.h,
_abi.py, _lib.py), ppo.ActorCritic(priv_dim=48) and one ppo.PPO.update with `priv` on the CPU against float64."""
import math
import os
import re

import numpy as np
import torch

from openroborl_amd import _abi, _lib, env as envmod, policy as pol, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_header_and_abi_constants_agree():
    hip, policy = _header("openroborl_hip.h"), _header("openroborl_policy.h")
    assert int(re.search(r"#define ORR_PRIV_DIM (\d+)", hip).group(1)) == _abi.PRIV_DIM == envmod.PRIV_DIM == 48
    assert int(re.search(r"#define ORR_POLICY_PRIV_DIM (\d+)", policy).group(1)) == _abi.POLICY_PRIV_DIM == pol.PRIV_DIM == _abi.PRIV_DIM
    assert re.search(r"int32_t orr_privileged_obs\(orr_handle\* h, const uint8_t\* done_dev, float\* priv_dev, void\* stream\);", hip)
    assert re.search(r"int32_t orr_policy_forward_priv\(const orr_policy_net\* net, const float\* obs, const float\* priv, int32_t n,", policy)
    # the name -> slice table covers the row once, in order, and the header documents every boundary of it
    cuts = sorted((s.start, s.stop) for s in envmod.PRIV_FIELDS.values())
    assert cuts[0][0] == 0 and cuts[-1][1] == envmod.PRIV_DIM and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    doc = hip[hip.index("Privileged observation"):hip.index("#define ORR_PRIV_DIM")]
    for a, b in cuts:
        if b - a > 1 and (a, b) not in ((28, 30), (30, 32)):      # MASS_RATIO and INERTIA_RATIO share the header's line 28..31
            assert re.search(r"\b%d\.\.%d\b" % (a, b - 1), doc), (a, b)
    assert re.search(r"\b28\.\.31\b", doc)


def test_both_names_are_exported():
    assert "orr_privileged_obs" in _lib.EXPORTS and "orr_policy_forward_priv" in _lib.EXPORTS
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def test_priv_units_is_one_row_behind_push_units_and_the_older_tables_are_unchanged():
    assert _lib.PRIV_UNITS == [("priv", _lib.SRC_PRIV, _lib.HIPCC_FLAGS_PLAIN, False)]
    assert os.path.basename(_lib.SRC_PRIV) == "orr_kernels_priv.hip" and os.path.isfile(_lib.SRC_PRIV) and _lib.SRC_PRIV in _lib.DEPS
    names = lambda table: [u[0] for u in table]   # noqa: E731
    assert names(_lib.UNITS) == ["env", "w2", "anchor", "multiclip", "policy", "learner"] and _lib.ENV_UNITS == _lib.UNITS[:4]
    assert names(_lib.ALL_UNITS) == names(_lib.UNITS) + ["noise"] and names(_lib.ALL_ENV_UNITS) == ["env", "w2", "anchor", "multiclip", "noise"]
    older = (_lib.NOISE_UNITS, _lib.TERMS_UNITS, _lib.CONTACT_UNITS, _lib.ACTUATOR_UNITS, _lib.SENSOR_UNITS, _lib.RANDOMIZER_UNITS, _lib.PUSH_UNITS)
    assert [names(t) for t in older] == [["noise"], ["terms"], ["contacts"], ["actuator"], ["sensor"], ["randomizer"], ["push"]]
    for t in older:
        assert t[0][2] == _lib.HIPCC_FLAGS and t[0][3] is False
    # build() compiles the tables in this order: the new unit last
    src = open(os.path.join(ROOT, "openroborl_amd", "_lib.py")).read()
    assert "RANDOMIZER_UNITS + PUSH_UNITS + PRIV_UNITS:" in src
    # its device code: one kernel, the launcher declared in the env kernels' header and called from the unit that holds the handle
    assert "launch_privileged_obs(" in open(os.path.join(_lib.CSRC, "orr_env_kernels.h")).read()
    assert "launch_privileged_obs(" in open(_lib.SRC).read() and "__global__" in open(_lib.SRC_PRIV).read()


def _mlp64(p, net, x):
    h = torch.relu(x @ p["model/%s_fc0/w:0" % net] + p["model/%s_fc0/b:0" % net])
    h = torch.relu(h @ p["model/%s_fc1/w:0" % net] + p["model/%s_fc1/b:0" % net])
    return h @ p["model/%s/w:0" % net] + p["model/%s/b:0" % net]


def test_actor_critic_with_a_privileged_critic_on_the_cpu(tmp_path):
    m = ppo.ActorCritic("cpu", seed=3, priv_dim=48)
    assert m.priv_dim == 48
    shapes = {k: tuple(v.shape) for k, v in m.p.items()}
    assert shapes["model/vf_fc0/w:0"] == (208, 512) and shapes["model/pi_fc0/w:0"] == (160, 512)
    assert shapes["model/vf_fc1/w:0"] == shapes["model/pi_fc1/w:0"] == (512, 256) and shapes["model/vf/w:0"] == (256, 1)
    # the same rule: N(0, 1) * sqrt(2) / sqrt(fan_in) with the new fan_in
    assert abs(float(m.p["model/vf_fc0/w:0"].detach().std()) * math.sqrt(208.0 / 2.0) - 1.0) < 0.02
    g = torch.Generator().manual_seed(0)
    obs, priv = torch.randn(37, 160, generator=g), torch.randn(37, 48, generator=g)
    with torch.no_grad():
        for k, v in m.p.items():
            if k.endswith("/b:0"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        v32 = m.value(obs, priv)
        a, raw, v_act = m.act(obs, priv, deterministic=True)
    p64 = {k: v.detach().double() for k, v in m.p.items()}
    v64 = _mlp64(p64, "vf", torch.cat((obs, priv), dim=1).double())[:, 0]
    assert float((v32.double() - v64).abs().max()) < 2e-5 * max(1.0, float(v64.abs().max()))
    assert torch.equal(v_act, v32) and torch.equal(raw, m.mean(obs).detach())
    # the vector is required by a privileged critic and refused by a plain one
    for call in (lambda: m.value(obs), lambda: m.act(obs), lambda: ppo.ActorCritic("cpu").value(obs, priv)):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("no ValueError")
    # a zip round trip infers the width; the reference's 160-row parameters keep loading as a plain critic
    path = str(tmp_path / "priv.zip")
    pol.save_parameters_zip(path, m.state_dict())
    back = ppo.ActorCritic("cpu", params=pol.load_parameters(path))
    assert back.priv_dim == 48
    for k in m.p:
        assert torch.equal(back.p[k].detach(), m.p[k].detach()), k
    from tests import oracle_lib as ol
    shipped = ppo.ActorCritic("cpu", params=pol.load_parameters(os.path.join(ol.GOLDEN, "policy_laikago_pace.npz")))
    assert shipped.priv_dim == 0 and tuple(shipped.p["model/vf_fc0/w:0"].shape) == (160, 512)


def test_priv_dim_zero_gives_todays_parameters():
    """The draws of the initialisation, restated: six layers in the order pi_fc0, pi_fc1, pi, vf_fc0, vf_fc1, vf from one generator."""
    m = ppo.ActorCritic("cpu", seed=7, priv_dim=0)
    d = ppo.ActorCritic("cpu", seed=7)
    g = torch.Generator().manual_seed(7)
    for net, out in (("pi", 12), ("vf", 1)):
        for name, fi, fo, gain in (("model/%s_fc0" % net, 160, 512, math.sqrt(2.0)), ("model/%s_fc1" % net, 512, 256, math.sqrt(2.0)),
                                   ("model/%s" % net, 256, out, 0.01 if net == "pi" else 1.0)):
            w = torch.randn(fi, fo, generator=g) * (gain / math.sqrt(fi))
            assert torch.equal(m.p[name + "/w:0"].detach(), w) and torch.equal(d.p[name + "/w:0"].detach(), w), name
            assert not bool(m.p[name + "/b:0"].detach().any())
    # and the actor of a privileged model is the plain model's actor for the same seed (it is initialised first)
    p = ppo.ActorCritic("cpu", seed=7, priv_dim=48)
    for k in m.p:
        if "/pi" in k:
            assert torch.equal(p.p[k].detach(), m.p[k].detach()), k


def test_one_ppo_update_with_priv_matches_float64_on_the_cpu():
    """tests/test_gpu_learner.py::test_one_ppo_update_matches_float64_cpu with a privileged critic, on the CPU, at its tolerances."""
    B = 4096                                    # engages the split weight-gradient path (ppo._wgrad) with the 208-row input
    g = torch.Generator().manual_seed(1)
    obs, priv = torch.randn(B, 160, generator=g), torch.randn(B, 48, generator=g)
    model = ppo.ActorCritic("cpu", seed=4, priv_dim=48)
    with torch.no_grad():
        mu = model.mean(obs)
        # the premise of comparing gradients across precisions: no hidden unit sits within float32 rounding of the ReLU's kink (one that
        # does has derivative 0 in one precision and 1 in the other: a whole column of a weight gradient then differs by one sample's
        # share).  Of the 6 M pre-activations here none does; the data seed was picked for that, and this assertion holds it
        for net, x in (("pi", obs), ("vf", torch.cat((obs, priv), dim=1))):
            h32, h64 = x, x.double()
            for layer in ("_fc0", "_fc1"):
                w, b = model.p["model/%s%s/w:0" % (net, layer)], model.p["model/%s%s/b:0" % (net, layer)]
                z32, z64 = h32 @ w + b, h64 @ w.double() + b.double()
                assert bool(((z32 > 0) == (z64 > 0)).all()), (net, layer)
                h32, h64 = torch.relu(z32), torch.relu(z64)
    act = mu + 0.125 * torch.randn(B, 12, generator=g)
    old_logp = (-0.5 * ((act - (mu + 0.04 * torch.randn(B, 12, generator=g))) ** 2) / 0.125 ** 2
                - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    adv, ret = torch.randn(B, generator=g), torch.randn(B, generator=g)

    p64 = {k: v.detach().double().requires_grad_(True) for k, v in model.p.items()}
    var = 0.125 ** 2
    logp64 = (-0.5 * ((act.double() - _mlp64(p64, "pi", obs.double())) ** 2) / var - 0.5 * math.log(2.0 * math.pi * var)).sum(dim=1)
    ratio64 = torch.exp(logp64 - old_logp.double())
    surr64 = -torch.min(ratio64 * adv.double(), torch.clamp(ratio64, 0.8, 1.2) * adv.double()).mean()
    vf64 = ((_mlp64(p64, "vf", torch.cat((obs, priv), dim=1).double())[:, 0] - ret.double()) ** 2).mean()
    (surr64 + vf64).backward()

    ratio = torch.exp(model.log_prob(obs, act) - old_logp)
    surr = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
    vf = ((model.value(obs, priv) - ret) ** 2).mean()
    (surr + vf).backward()
    clipped = ((ratio < 0.8) | (ratio > 1.2)).float().mean().item()
    assert 0.02 < clipped < 0.9, clipped
    assert abs(surr.item() - surr64.item()) < 2e-4 * max(1.0, abs(surr64.item()))
    assert abs(vf.item() - vf64.item()) < 2e-4 * max(1.0, abs(vf64.item()))
    for k in sorted(model.p):
        g32, g64 = model.p[k].grad.detach().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        assert cs.item() > 0.99999, (k, cs.item())
    assert float(p64["model/vf_fc0/w:0"].grad[160:].abs().max()) > 0.0          # the privileged rows are trained

    before = {k: v.detach().clone() for k, v in model.p.items()}
    for v in model.p.values():
        v.grad = None
    learner = ppo.PPO(model, lr=1e-4, adam_eps=1e-5, minibatch=B)
    learner.update(obs, act, adv, ret, old_logp=old_logp, epochs=1, generator=torch.Generator().manual_seed(1), priv=priv)
    for k in sorted(model.p):
        g64 = p64[k].grad
        step64 = -1e-4 * g64 / (g64.abs() + 1e-5)              # m_hat = g, v_hat = g^2 at t = 1
        step = (model.p[k].detach() - before[k]).double()
        big = g64.abs() > 1e-3
        assert big.any()
        assert (step - step64)[big].abs().max().item() < 2e-6, k
        assert step.abs().max().item() <= 1e-4 * (1 + 1e-3)
    # the learner asks for the vector exactly when the critic is privileged
    for lrn, kw in ((learner, {}), (ppo.PPO(ppo.ActorCritic("cpu", seed=4), minibatch=B), {"priv": priv})):
        try:
            lrn.update(obs, act, adv, ret, old_logp=old_logp, **kw)
        except ValueError:
            continue
        raise AssertionError("no ValueError")
