"""ActorCritic, the trainable twin of policy.MLPPolicy that every learner trains, and the GEMM-with-epilogue layers it is made of.  ppo
re-exports every name."""
import math

import numpy as np

from . import policy as pol
from .history import ENC_HIDDEN, HISTORY_DIM, HISTORY_STEPS
from .obs_norm import RunningNorm, _norm_state

_LINEAR = {}

LOGSTD = pol.LOGSTD                # the learned log-std [1, 12] of ActorCritic(learn_std=True); the reference declares it and freezes it (imitation_policies.py:48)
ENTROPY_CONST = 6.0 * math.log(2.0 * math.pi * math.e)     # H of a 12-dimensional diagonal Gaussian = sum_k log_std_k + this
LOG_STD_BOUNDS = (math.log(0.01), math.log(1.0))
STAT_NAMES = ("surr", "vf", "entropy", "approx_kl", "clip_fraction")     # what a learner of a learn-std model returns (a fixed-std one: the first two)


def _wgrad(torch, x, g):
    """x^T g for a tall batch: hipBLASLt picks a 32x32 macro-tile for these (K = batch) shapes and fills a third of the
    chip; a 16-way split over the batch (one bmm + a sum) is 2.5-3x faster on MI355X (100 -> 35 us at 16384 x 160 x 512)."""
    B = x.shape[0]
    if B >= 4096 and B % 16 == 0:
        return torch.bmm(x.view(16, B // 16, x.shape[1]).transpose(1, 2), g.view(16, B // 16, g.shape[1])).sum(0)
    return x.t() @ g


def _linear(torch, relu):
    """x W + b (optionally ReLU) as one GEMM with a bias (+ ReLU) epilogue; the backward is spelled out because
    torch._addmm_activation has no autograd formula and to route the weight gradient through _wgrad."""
    if relu not in _LINEAR:
        class Linear(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w, b):
                h = torch._addmm_activation(b, x, w) if relu else torch.addmm(b, x, w)
                ctx.save_for_backward(x, w, h if relu else b)
                return h

            @staticmethod
            def backward(ctx, gh):
                x, w, h = ctx.saved_tensors
                gz = gh * (h > 0).to(gh.dtype) if relu else gh
                gx = gz @ w.t() if ctx.needs_input_grad[0] else None
                return gx, _wgrad(torch, x, gz.contiguous()), gz.sum(dim=0)
        _LINEAR[relu] = Linear.apply
    return _LINEAR[relu]


class ActorCritic(object):
    """Trainable twin of policy.MLPPolicy (same parameter names as the stable-baselines zips).

    priv_dim = 48 makes the critic privileged (the asymmetric actor-critic): model/vf_fc0/w:0 is [obs_dim + priv_dim, 512] and reads
    cat(obs, priv), priv = env.privileged_obs(); the actor is what it is without, so its part of a saved zip loads wherever the plain
    policy loads.  With `params` the width is taken from that matrix.  priv_dim = 0: every path is the plain one.

    actor_priv_dim = 48 (with priv_dim = 48 only) makes the actor privileged as well - a teacher policy: model/pi_fc0/w:0 is
    [obs_dim + 48, 512] too, and mean(), log_prob() and act() take `priv`.  Such a policy cannot be deployed (nor loaded by the reference);
    Distill / learner_hip.FusedDistill turn it into a plain one.  With `params` the width is taken from model/pi_fc0/w:0.
    actor_priv_dim = 0: every path is the one without.

    history = 16 (with actor_priv_dim = 48 only) adds an encoder over the last 16 steps' sensors, model/enc_fc0 [512, 256] (ReLU) and
    model/enc_fc1 [256, 48]: a history student.  encode(hist) estimates the privileged row from hist [N, 512] (history_push), and mean() and
    act() take `hist` in the row's place - the teacher's actor and critic on cat(obs, encode(hist)).  Such a policy is deployable: it reads
    its own sensors only.  The encoder is drawn after every other parameter, so history = 0 is the model without, draw for draw.  With
    `params` the presence of model/enc_fc0/w:0 decides.  act(obs, hist=hist, critic_priv=priv) is the asymmetric form PPOHistory trains: the
    actor on the estimate, the value from the true row.

    learn_std = True adds model/pi/logstd:0 [1, 12], filled with log(std): a state-independent log-std that PPO / learner_hip.FusedPPO train
    (with an entropy bonus, ent_coef).  act() then samples mean + exp(log_std) * noise and log_prob() is the per-dimension Gaussian's.  It is
    filled, not drawn: every other parameter is what it is without, draw for draw.  With `params` the presence of the key decides.  `log_std`
    is the device tensor, and the one thing rollout and update paths read; `std` is then the twelve values on the host, for logging only.

    obs_norm = True puts a running normaliser in front of both nets: `obs_norm`, a RunningNorm over the 160 observation words, and with
    priv_dim `priv_norm` over the 48 of the privileged row.  mean(), value(), log_prob() and the torch path of act() normalise what they
    are given, (x - mean) * rstd spelled out; the fused path runs on raw inputs with the normaliser folded into the packed layer 0
    (orr_policy_pack_norm).  The statistics are not parameters: nothing trains them, update_obs_norm() merges a rollout segment into them,
    state_dict() carries them as obs_norm/count, /mean, /var, /eps (priv_norm/*), and with `params` their presence decides.  A history
    policy with obs_norm is refused."""

    def __init__(self, device, obs_dim=160, act_dim=12, hidden=(512, 256), std=pol.PI_STD, params=None, seed=0, priv_dim=0, actor_priv_dim=0,
                 history=0, learn_std=False, obs_norm=False):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self._std = float(std)
        if params is not None and "model/vf_fc0/w:0" in params:
            priv_dim = int(np.shape(params["model/vf_fc0/w:0"])[0]) - obs_dim
        if priv_dim not in (0, pol.PRIV_DIM):
            raise ValueError("priv_dim must be 0 or %d, got %r" % (pol.PRIV_DIM, priv_dim))
        self.priv_dim = int(priv_dim)
        if params is not None and "model/pi_fc0/w:0" in params:
            actor_priv_dim = int(np.shape(params["model/pi_fc0/w:0"])[0]) - obs_dim
        if actor_priv_dim not in (0, pol.PRIV_DIM):
            raise ValueError("actor_priv_dim must be 0 or %d, got %r" % (pol.PRIV_DIM, actor_priv_dim))
        if actor_priv_dim and not self.priv_dim:
            raise ValueError("a privileged actor (actor_priv_dim = %d) needs the privileged critic (priv_dim = %d)" % (pol.PRIV_DIM, pol.PRIV_DIM))
        self.actor_priv_dim = int(actor_priv_dim)
        if params is not None:
            history = HISTORY_STEPS if "model/enc_fc0/w:0" in params else 0
        if history not in (0, HISTORY_STEPS):
            raise ValueError("history must be 0 or %d, got %r" % (HISTORY_STEPS, history))
        if history and not self.actor_priv_dim:
            raise ValueError("a history encoder (history = %d) feeds a privileged actor (actor_priv_dim = %d)" % (HISTORY_STEPS, pol.PRIV_DIM))
        self.history = int(history)
        g = torch.Generator().manual_seed(seed)
        self.p = {}
        dims = [obs_dim] + list(hidden)
        for net, out in (("pi", act_dim), ("vf", 1)):
            for i in range(len(hidden)):
                fan_in = dims[i] + (self.priv_dim if (net, i) == ("vf", 0) else 0) + (self.actor_priv_dim if (net, i) == ("pi", 0) else 0)
                self._init("model/%s_fc%d" % (net, i), fan_in, dims[i + 1], g, math.sqrt(2.0))
            self._init("model/%s" % net, dims[-1], out, g, 0.01 if net == "pi" else 1.0)
        if self.history:           # after every other draw
            self._init("model/enc_fc0", HISTORY_DIM, ENC_HIDDEN, g, math.sqrt(2.0))
            self._init("model/enc_fc1", ENC_HIDDEN, pol.PRIV_DIM, g, 1.0)
        if params is not None:
            learn_std = LOGSTD in params
        self.learn_std = bool(learn_std)
        if self.learn_std:         # filled, no draw
            if not self._std > 0.0:
                raise ValueError("learn_std needs std > 0, got %r" % (std,))
            self.p[LOGSTD] = torch.full((1, act_dim), math.log(self._std), dtype=torch.float32, device=self.device)
        # obs_norm: a RunningNorm over the 160 observation words, and one over the privileged row of a model that reads it.  With `params`
        # the presence of obs_norm/count decides, and the statistics are the file's.  No draw: every parameter is what it is without
        obs_state, priv_state = _norm_state(params, "obs_norm"), _norm_state(params, "priv_norm")
        if params is not None:
            obs_norm = obs_state is not None
        self.obs_norm = self.priv_norm = None
        if obs_norm:
            if self.history:
                raise ValueError("obs_norm with a history policy is not built: the encoder's frames are a subset of the observation and would "
                                 "need the same statistics; train the history policy on raw observations")
            self.obs_norm = RunningNorm(self.device, obs_dim)
            if obs_state is not None:
                self.obs_norm.load_state_dict(obs_state)
            if self.priv_dim:
                self.priv_norm = RunningNorm(self.device, self.priv_dim)
                if priv_state is not None:
                    self.priv_norm.load_state_dict(priv_state)
        self.extra = {}            # variables of a loaded zip that this learner does not train (model/q/*): re-emitted by state_dict()
        if params is not None:
            for k, v in params.items():
                if k.startswith(("obs_norm/", "priv_norm/")):
                    continue
                if k in self.p:
                    self.p[k].data.copy_(torch.as_tensor(np.asarray(v), dtype=torch.float32))
                else:
                    self.extra[k] = np.asarray(v, dtype=np.float32).copy()
        for v in self.p.values():
            v.requires_grad_(True)
        self.fused = None          # policy_hip.FusedActorCritic once enable_fused() was called
        self._fused_dirty = True

    @property
    def std(self):
        """The fixed std; of a learn-std model the twelve current values as a host array - a device read, for logging only."""
        if self.learn_std:
            return self.p[LOGSTD].detach().exp().reshape(-1).cpu().numpy()
        return self._std

    @property
    def log_std(self):
        """The learned log-std on the device, [1, 12] (a view of the learner's flat buffer once a fused learner owns it)."""
        if not self.learn_std:
            raise AttributeError("this model has a fixed std (learn_std = False)")
        return self.p[LOGSTD]

    @std.setter
    def std(self, value):
        """One number for the sampler AND the log-probabilities: the fused forward pass takes std by value at every launch, so a policy
        whose std is changed after enable_fused() must hand it on (a re-captured rollout graph sampled with the old std while
        the log-probabilities used the new one)."""
        if self.learn_std:
            raise AttributeError("a learn-std model's std is exp(log_std), a trained parameter: write model.log_std on the device and call "
                                 "mark_updated(), which makes the fused sampler renew its copy")
        self._std = float(value)
        if getattr(self, "fused", None) is not None:
            self.fused.std = self._std

    def enable_fused(self):
        """Route act() through the fused matrix-core forward pass (csrc/orr_policy.hip).  The packed weight copy is
        refreshed lazily after mark_updated() (the learner calls it after every optimiser step)."""
        from . import policy_hip
        self.fused = policy_hip.FusedActorCritic(self.p, self.device, std=self._std, obs_norm=self.obs_norm, priv_norm=self.priv_norm)
        self._fused_dirty = False
        return self

    def update_obs_norm(self, obs, priv=None):
        """Merge a rollout segment into the statistics: obs [T N, 160] (and priv [T N, 48] for a model that reads the row), one
        orr_running_stats_update per record on the GPU.  Call it AFTER the learner's update - old log-probabilities, old values and the
        learner's first forward pass must all see the function the rollout ran - and mark_updated() behind it: the fused forward pass
        folds the new statistics into layer 0 at its next refresh()."""
        if self.obs_norm is None:
            raise ValueError("this model has no observation normaliser (obs_norm = False)")
        if (priv is not None) != (self.priv_norm is not None):
            raise ValueError("priv is needed by a model that normalises the privileged row (priv_dim = %d) and by no other" % pol.PRIV_DIM)
        self.obs_norm.update(obs)
        if priv is not None:
            self.priv_norm.update(priv)
        self._fused_dirty = True

    def mark_updated(self):
        self._fused_dirty = True
        self.updates = getattr(self, "updates", 0) + 1      # whoever keeps a packed copy of its own compares this count (FusedDistillHistory)

    def _init(self, name, fan_in, fan_out, g, gain):
        t = self.torch
        w = t.randn(fan_in, fan_out, generator=g) * (gain / math.sqrt(fan_in))
        self.p[name + "/w:0"] = w.to(self.device)
        self.p[name + "/b:0"] = t.zeros(fan_out, device=self.device)

    def parameters(self):
        return [self.p[k] for k in sorted(self.p)]

    def _mlp(self, net, x):
        t = self.torch   # bias and ReLU ride in the GEMM epilogue (hipBLASLt): one kernel per layer instead of three
        f, out = _linear(t, True), _linear(t, False)
        h = f(x, self.p["model/%s_fc0/w:0" % net], self.p["model/%s_fc0/b:0" % net])
        h = f(h, self.p["model/%s_fc1/w:0" % net], self.p["model/%s_fc1/b:0" % net])
        return out(h, self.p["model/%s/w:0" % net], self.p["model/%s/b:0" % net])

    def _actor_input(self, obs, priv):
        if (priv is not None) != (self.actor_priv_dim > 0):
            raise ValueError("priv is needed by a privileged actor (actor_priv_dim = %d) and by no other" % pol.PRIV_DIM)
        obs, priv = self._normalized(obs, priv)
        return obs if priv is None else self.torch.cat((obs, priv), dim=1)

    def _normalized(self, obs, priv):
        """What layer 0 reads of (obs, priv): themselves, or with obs_norm (x - mean) * rstd of each, spelled out in torch - the reference of
        the fused forward pass's folded layer 0 and of the learners' normalised batch."""
        if self.obs_norm is None:
            return obs, priv
        return self.obs_norm.apply(obs), (None if priv is None else self.priv_norm.apply(priv))

    def actor_priv(self, priv):
        """What mean() and log_prob() take as `priv` when the caller holds the critic's: the vector for a privileged actor, None for a plain one."""
        return priv if self.actor_priv_dim else None

    def encode(self, hist):
        """hist [N, 512] (history_push) -> the encoder's estimate of the privileged row [N, 48]."""
        if not self.history:
            raise ValueError("this model has no history encoder (history = 0)")
        t = self.torch
        h = _linear(t, True)(hist, self.p["model/enc_fc0/w:0"], self.p["model/enc_fc0/b:0"])
        return _linear(t, False)(h, self.p["model/enc_fc1/w:0"], self.p["model/enc_fc1/b:0"])

    def _latent(self, priv, hist):
        """The row the actor and the critic read: `priv` itself, or the encoder's estimate from `hist` (one of the two)."""
        if hist is None:
            return priv
        if priv is not None:
            raise ValueError("give priv or hist, not both")
        return self.encode(hist)

    def mean(self, obs, priv=None, hist=None):
        return self._mlp("pi", self._actor_input(obs, self._latent(priv, hist)))

    def _critic_input(self, obs, priv):
        if (priv is not None) != (self.priv_dim > 0):
            raise ValueError("priv is needed by a privileged critic (priv_dim = %d) and by no other" % pol.PRIV_DIM)
        obs, priv = self._normalized(obs, priv)
        return obs if priv is None else self.torch.cat((obs, priv), dim=1)

    def value(self, obs, priv=None):
        return self._mlp("vf", self._critic_input(obs, priv))[:, 0]

    def act(self, obs, priv=None, deterministic=False, generator=None, noise=None, out_raw=None, out_value=None, hist=None, out_latent=None,
            critic_priv=None):
        """-> (clipped action, raw action, value).  `noise` ([N,12] standard normal) overrides the generator; `priv` ([N,48], the
        privileged observation) goes to a privileged critic, and to a privileged actor.  `hist` ([N,512], a history student's input)
        takes its place: actor and critic read the encoder's estimate, which out_latent [N,48] receives.  `critic_priv` ([N,48], with
        `hist` only) makes the critic asymmetric: the actor still reads the estimate, the value comes from the true row -
        mean(obs, hist=hist) and value(obs, critic_priv), what PPOHistory trains."""
        t = self.torch
        if critic_priv is not None:
            if hist is None:
                raise ValueError("critic_priv goes with hist: the actor reads the encoder's estimate, the critic the true row")
            if tuple(critic_priv.shape) != (obs.shape[0], pol.PRIV_DIM):
                raise ValueError("critic_priv must have shape (%d, %d), got %s" % (obs.shape[0], pol.PRIV_DIM, tuple(critic_priv.shape)))
        if hist is not None:
            if priv is not None:
                raise ValueError("give priv or hist, not both")
            if not self.history:
                raise ValueError("this model has no history encoder (history = 0)")
            if self.fused is None:
                with t.no_grad():
                    priv = self.encode(hist)
                    if out_latent is not None:
                        out_latent.copy_(priv)
        if hist is None and out_latent is not None:
            raise ValueError("out_latent belongs to hist")
        if hist is None and (priv is not None) != (self.priv_dim > 0):
            raise ValueError("priv is needed by a privileged critic (priv_dim = %d) and by no other" % pol.PRIV_DIM)
        if self.fused is not None:
            if self._fused_dirty:
                self.fused.refresh()
                self._fused_dirty = False
            if noise is None and not deterministic:
                noise = t.randn((obs.shape[0], 12), device=obs.device, generator=generator)
            if hist is not None:
                a, raw, v, _ = self.fused.forward(obs, None if deterministic else noise, out_raw=out_raw, out_value=out_value, hist=hist,
                                                  out_latent=out_latent, **({} if critic_priv is None else {"critic_priv": critic_priv}))
            else:
                a, raw, v, _ = self.fused.forward(obs, None if deterministic else noise, out_raw=out_raw, out_value=out_value, priv=priv)
            return a, raw, v
        with t.no_grad():
            mu = self.mean(obs, self.actor_priv(priv))
            if noise is None and not deterministic:
                noise = t.randn(mu.shape, device=mu.device, generator=generator)
            a = mu if deterministic else mu + (self.p[LOGSTD].exp() if self.learn_std else self.std) * noise
            return t.clamp(a, -2.0 * math.pi, 2.0 * math.pi), a, self.value(obs, priv if critic_priv is None else critic_priv)

    def log_prob(self, obs, actions, priv=None, hist=None):
        mu = self.mean(obs, priv, hist)
        if self.learn_std:
            ls = self.p[LOGSTD]
            z = (actions - mu) * self.torch.exp(-ls)
            return (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
        var = self.std * self.std
        return (-0.5 * ((actions - mu) ** 2) / var - 0.5 * math.log(2.0 * math.pi * var)).sum(dim=1)

    def state_dict(self):
        d = {k: v.detach().cpu().numpy() for k, v in self.p.items()}
        d.update(self.extra)
        if not self.learn_std:      # carried from a learn-std teacher (train.py: history_student) but not sampled with: a zip that held it would
            d.pop(LOGSTD, None)     # reload as a learn-std policy with the teacher's stds, not the fixed std this model was rolled out with
        for prefix, norm in (("obs_norm", self.obs_norm), ("priv_norm", self.priv_norm)):
            if norm is not None:
                d.update({"%s/%s" % (prefix, k): v for k, v in norm.state_dict().items()})
        return d
