"""PPO learner in PyTorch-ROCm -- the consumer of rollout.py's [T, N] buffers.

Restates the update of agents/ppo_imitation.py:156-258,352-382 (stable-baselines PPO1 graph) without TF1/MPI:
  * actor 160 -> 512 -> 256 -> 12 and critic 160 -> 512 -> 256 -> 1, ReLU (run.py:101-105), fixed-variance diagonal
    Gaussian, std 0.125 (agents/imitation_policies.py:44-51,96-107);
  * clipped surrogate with clip_param 0.2, value loss mean((v - tdlamret)^2), Adam lr 1e-5, eps 1e-5, one epoch over
    the segment (run.py:111-125; ppo1/pposgd_simple.py loss terms);
  * data-parallel: one process per GPU, gradients averaged with ONE all-reduce of a flat 1.7 MB buffer per minibatch
    (RCCL over xGMI; replaces MpiAdam's Allreduce, stable_baselines/common/mpi_adam.py:40-62).
The env never leaves the device, so a full iteration is: collect_rollout -> gae -> normalize_per_robot -> update.
"""
import math

import numpy as np

from . import policy as pol


_LINEAR = {}

LOGSTD = pol.LOGSTD                # the learned log-std [1, 12] of ActorCritic(learn_std=True); the reference declares it and freezes it (imitation_policies.py:48)
ENTROPY_CONST = 6.0 * math.log(2.0 * math.pi * math.e)     # H of a 12-dimensional diagonal Gaussian = sum_k log_std_k + this
LOG_STD_BOUNDS = (math.log(0.01), math.log(1.0))
STAT_NAMES = ("surr", "vf", "entropy", "approx_kl", "clip_fraction")     # what a learner of a learn-std model returns (a fixed-std one: the first two)

# the sensor history of a history student (include/openroborl_policy.h: ORR_HISTORY_*): 16 frames of 32 words, newest first
HISTORY_STEPS, HISTORY_FRAME, HISTORY_DIM = 16, 32, 512
ENC_HIDDEN = 256


def history_frame(obs):
    """The newest reading of each sensor history inside obs [N,160] + four zeros: IMU obs[0:4], last action obs[12:24], motor angles obs[48:60]."""
    import torch
    return torch.cat((obs[:, 0:4], obs[:, 12:24], obs[:, 48:60], obs.new_zeros(obs.shape[0], 4)), dim=1)


def history_push(hist, obs, done):
    """The plain-torch statement of orr_history_push: hist [N,512] before the step (None with done None), obs [N,160] the observation after
    it, done [N] the step's flags (None: everybody starts an episode) -> the history after it, a new tensor.  Slot 0 is obs's frame; a robot
    whose episode just ended has that frame in all 16 slots; everybody else's slots move one back."""
    import torch
    frame = history_frame(obs)
    fresh = frame.repeat(1, HISTORY_STEPS)
    if done is None:
        return fresh
    shifted = torch.cat((frame, hist[:, :HISTORY_DIM - HISTORY_FRAME]), dim=1)
    return torch.where(done.to(torch.bool)[:, None], fresh, shifted)


NORM_EPS = pol.NORM_EPS            # rstd = 1 / (sqrt(var) + eps), rsl_rl's EmpiricalNormalization: at most 100
NORM_KEYS = ("count", "mean", "var")


class RunningNorm(object):
    """Running mean / variance of `dim` network inputs and the normaliser (x - mean) * rstd they define, rstd = 1 / (sqrt(var) + eps).

    The statistics are ONE record of 4 + 3 dim 32-bit words (include/openroborl_learner.h: an int64 count and pad, then mean, var, rstd), on
    the GPU at a fixed address: update() is orr_running_stats_update on it (one pass over the batch, merged by the parallel formula, no host
    round trip), and whoever folds or applies the normaliser inside a captured graph reads the same words after every update.  A record on
    the CPU has the same layout; update() is then the torch statement of the same merge, in float64 on float32 inputs with float32
    results - the yardstick of the kernel.  A fresh record is the identity: count 0, mean 0, var 1, rstd 1.  `frozen` makes update() a
    no-op."""

    def __init__(self, device, dim, eps=NORM_EPS):
        import torch
        from . import _abi
        self.torch = torch
        self.device = torch.device(device)
        self.dim, self.eps = int(dim), float(np.float32(eps))
        if self.dim < 4 or self.dim > 256 or self.dim % 4:
            raise ValueError("RunningNorm: dim must be a multiple of 4 from 4 to 256, got %r" % (dim,))
        if not (self.eps > 0.0 and math.isfinite(self.eps)):
            raise ValueError("RunningNorm: eps must be positive and finite")
        self.rec = torch.zeros(_abi.running_stats_floats(self.dim), dtype=torch.float32, device=self.device)
        om, ov, orr = _abi.running_stats_offsets(self.dim)
        self.count_word = self.rec[:2].view(torch.int64)          # [1]
        self.mean, self.var, self.rstd = self.rec[om:om + self.dim], self.rec[ov:ov + self.dim], self.rec[orr:orr + self.dim]
        self.var.fill_(1.0)
        self.rstd.fill_(1.0)
        self.frozen = False
        self._partials = None

    @property
    def count(self):
        """Rows seen so far - a device read."""
        return int(self.count_word.item())

    def _check(self, x, name):
        t = self.torch
        if x.dtype != t.float32 or x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] < 1 or x.device != self.rec.device or not x.is_contiguous():
            raise ValueError("RunningNorm: %s must be a contiguous float32 [n, %d] tensor on %s" % (name, self.dim, self.rec.device))

    def _rstd_of(self, var):
        """float32 var -> float32 rstd, the kernel's arithmetic: float64 on the stored float32 value, rounded once."""
        return (1.0 / (var.double().sqrt() + self.eps)).float()

    def update(self, x):
        """Merge the moments of x [n, dim] into the record.  Returns self."""
        if self.frozen:
            return self
        t = self.torch
        x = x.detach()
        self._check(x, "x")
        n = int(x.shape[0])
        with t.no_grad():
            if x.is_cuda:
                import ctypes as C
                from . import _lib
                L = _lib.load()
                need = int(L.orr_running_stats_partials(n, self.dim))
                if self._partials is None or self._partials.numel() < need:
                    self._partials = t.empty(need, dtype=t.float32, device=self.rec.device)
                _lib.check(L.orr_running_stats_update(x.data_ptr(), n, self.dim, self.eps, self.rec.data_ptr(), self._partials.data_ptr(),
                                                      C.c_void_p(t.cuda.current_stream(self.rec.device).cuda_stream)), L)
                return self
            xd = x.double()
            mean_b = xd.mean(dim=0)
            m2_b = ((xd - mean_b) ** 2).sum(dim=0)
            na = int(self.count_word.item())
            if na > 0:
                tot = float(na + n)
                delta = mean_b - self.mean.double()
                m2_b = self.var.double() * float(na) + m2_b + delta * delta * (float(na) * float(n) / tot)
                mean_b = self.mean.double() + delta * (float(n) / tot)
            self.mean.copy_(mean_b.float())
            self.var.copy_((m2_b / float(max(na, 0) + n)).float())
            self.rstd.copy_(self._rstd_of(self.var))
            self.count_word.fill_(max(na, 0) + n)
        return self

    def apply(self, x):
        """(x - mean) * rstd as a torch expression, float32, two roundings: the reference of orr_normalize_rows and of the folded layer."""
        return (x - self.mean) * self.rstd

    def normalize(self, x, out=None):
        """(x - mean) * rstd into `out` (default: a new tensor; `out` may be x).  On the GPU one orr_normalize_rows launch."""
        t = self.torch
        self._check(x, "x")
        if out is None:
            out = t.empty_like(x)
        else:
            self._check(out, "out")
        with t.no_grad():
            if x.is_cuda:
                import ctypes as C
                from . import _lib
                L = _lib.load()
                _lib.check(L.orr_normalize_rows(x.data_ptr(), int(x.shape[0]), self.dim, self.mean.data_ptr(), self.rstd.data_ptr(), out.data_ptr(),
                                                C.c_void_p(t.cuda.current_stream(self.rec.device).cuda_stream)), L)
            else:
                out.copy_(self.apply(x))
        return out

    def state_dict(self):
        """{"count": int64 [], "mean": float32 [dim], "var": float32 [dim], "eps": float32 []}; rstd follows from var and eps."""
        return {"count": np.asarray(self.count, dtype=np.int64), "mean": self.mean.detach().cpu().numpy().copy(),
                "var": self.var.detach().cpu().numpy().copy(), "eps": np.asarray(self.eps, dtype=np.float32)}

    def load_state_dict(self, d):
        t = self.torch
        mean, var = (np.asarray(d[k], dtype=np.float32).reshape(-1) for k in ("mean", "var"))
        if mean.shape != (self.dim,) or var.shape != (self.dim,) or not (var >= 0.0).all() or int(np.asarray(d["count"]).reshape(-1)[0]) < 0:
            raise ValueError("RunningNorm: statistics of %d columns with var >= 0 and count >= 0 expected" % self.dim)
        if "eps" in d:
            self.eps = float(np.float32(np.asarray(d["eps"]).reshape(-1)[0]))
        with t.no_grad():
            self.mean.copy_(t.from_numpy(mean))
            self.var.copy_(t.from_numpy(var))
            self.rstd.copy_(self._rstd_of(self.var))
            self.count_word.fill_(int(np.asarray(d["count"]).reshape(-1)[0]))
        return self


def _norm_state(params, prefix):
    """The statistics a parameter dict carries under `prefix`/ (policy.save_parameters_zip), or None."""
    if params is None or prefix + "/count" not in params:
        return None
    return {k: params["%s/%s" % (prefix, k)] for k in NORM_KEYS + ("eps",) if "%s/%s" % (prefix, k) in params}


def _no_obs_norm(model, who):
    if getattr(model, "obs_norm", None) is not None:
        raise ValueError("%s: a model with an observation normaliser (ActorCritic(obs_norm=True)) is trained by PPO / learner_hip.FusedPPO; "
                         "normalisers for the history and distillation learners are not built" % who)


def _no_history(model, who):
    if getattr(model, "history", 0):
        raise ValueError("%s: a history policy (history = %d) is trained by PPOHistory / learner_hip.FusedPPOHistory (PPO with the critic on the "
                         "true privileged row) or by DistillHistory / learner_hip.FusedDistillHistory" % (who, model.history))


def _entropy_args(model, who, ent_coef, log_std_bounds):
    """-> (learn_std, ent_coef, (lo, hi)) of a PPO learner, checked."""
    learn = bool(getattr(model, "learn_std", False))
    ent_coef = float(ent_coef)
    lo, hi = float(log_std_bounds[0]), float(log_std_bounds[1])
    if not learn and ent_coef != 0.0:
        raise ValueError("%s: ent_coef = %g needs a learn-std model (ActorCritic(learn_std=True)): the entropy of a fixed std has no gradient" % (who, ent_coef))
    if not (math.isfinite(ent_coef) and lo < hi and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("%s: ent_coef must be finite and log_std_bounds (lo, hi) finite with lo < hi" % who)
    return learn, ent_coef, (lo, hi)


KL_LR_BOUNDS = (0.01, 10.0)        # the KL-adaptive learning rate stays within these multiples of lr


def _control_args(who, max_grad_norm=None, kl_stop=None, kl_target=None, kl_lr_bounds=KL_LR_BOUNDS):
    """-> (max_grad_norm, kl_stop, kl_target, (lo, hi)) of a learner's update controls, checked; None: that control is off."""
    out = []
    for name, x in (("max_grad_norm", max_grad_norm), ("kl_stop", kl_stop), ("kl_target", kl_target)):
        if x is not None and not (float(x) > 0.0 and math.isfinite(float(x))):
            raise ValueError("%s: %s must be positive and finite (None: off)" % (who, name))
        out.append(None if x is None else float(x))
    lo, hi = float(kl_lr_bounds[0]), float(kl_lr_bounds[1])
    if not (0.0 < lo <= hi and math.isfinite(hi)):
        raise ValueError("%s: kl_lr_bounds (lo, hi) are multipliers of lr with 0 < lo <= hi" % who)
    return out[0], out[1], out[2], (lo, hi)


class _UpdateControl(object):
    """The update controls of the torch learners, the yardstick of learner_hip's device path (orr_update_control, orr_adam_step_ctl) with the
    same float32 arithmetic: the global gradient norm and torch.nn.utils.clip_grad_norm_'s coefficient, a guard that skips the step of a
    non-finite gradient (or KL), a learning-rate multiplier set by the caller (set_lr_mult), an early stop of the update() once a minibatch's
    approx_kl exceeds kl_stop, and the KL-adaptive learning rate (above 2 kl_target: / 1.5, below kl_target / 2: * 1.5, within kl_lr_bounds).
    A skipped step skips opt.step() altogether: the optimiser's step count stands.  The KL rules read the minibatch's KL on the host, one
    sync per minibatch.  Without any of the arguments the learners call opt.step() as they always did."""

    def _control_init(self, max_grad_norm=None, kl_stop=None, kl_target=None, kl_lr_bounds=KL_LR_BOUNDS, device_lr=False):
        self.max_grad_norm, self.kl_stop, self.kl_target, self.kl_lr_bounds = _control_args(type(self).__name__, max_grad_norm, kl_stop, kl_target,
                                                                                            kl_lr_bounds)
        self.kl_on = self.kl_stop is not None or self.kl_target is not None
        self.control_on = self.max_grad_norm is not None or self.kl_on or bool(device_lr)
        self.base_lr = float(self.opt.param_groups[0]["lr"])
        self.lr_mult, self.kl_lr_mult, self.kl_stopped = 1.0, 1.0, False
        self.grad_norms = []                 # every minibatch's norm since construction, in order (the tests place their thresholds by it)
        self.kls = []                        # likewise the KLs the rules saw
        self._clear_counters()

    def _clear_counters(self):
        self.ctl = {"grad_norm": 0.0, "grad_norm_max": 0.0, "grad_norm_sum": 0.0, "calls": 0, "clipped": 0, "skipped_nonfinite": 0, "skipped_kl": 0}

    def set_lr_mult(self, x):
        """The schedule's multiplier of lr from the next step on."""
        self.control_on = True
        self.lr_mult = float(x)

    def control_stats(self):
        """The diagnostics since the last call, and clears the counters (learner_hip's control_stats())."""
        c = self.ctl
        out = dict(c, grad_norm_mean=c["grad_norm_sum"] / max(c["calls"], 1), lr_mult=self.lr_mult, kl_lr_mult=self.kl_lr_mult)
        del out["grad_norm_sum"]
        self._clear_counters()
        return out

    def _begin_update(self):
        self.kl_stopped = False              # the stop holds for one update()

    def _step(self, kl=None):
        """opt.step() under the controls; kl: the minibatch's approx_kl (a tensor) when a KL rule is on.  Returns whether the step was taken."""
        if not self.control_on:
            self.opt.step()
            return True
        t, f32, c = self.torch, np.float32, self.ctl
        grads = [p.grad for grp in self.opt.param_groups for p in grp["params"] if p.grad is not None]
        norm = f32(float(t.linalg.vector_norm(t.stack([t.linalg.vector_norm(g) for g in grads]))))
        kl = f32(float(kl)) if (kl is not None and self.kl_on) else f32(0.0)
        self.grad_norms.append(float(norm))
        self.kls.append(float(kl))
        bad = not (np.isfinite(norm) and np.isfinite(kl))
        if not bad and self.kl_stop is not None and kl > f32(self.kl_stop):
            self.kl_stopped = True
        skip = bad or self.kl_stopped
        if not skip and self.kl_target is not None:
            tgt, m = f32(self.kl_target), f32(self.kl_lr_mult)
            if kl > f32(2.0) * tgt:
                m = max(f32(self.kl_lr_bounds[0]), m / f32(1.5))
            elif kl > 0.0 and kl < f32(0.5) * tgt:
                m = min(f32(self.kl_lr_bounds[1]), m * f32(1.5))
            self.kl_lr_mult = float(m)
        scale = f32(1.0)
        if bad:
            c["skipped_nonfinite"] += 1
        else:
            if self.max_grad_norm is not None:
                scale = min(f32(1.0), f32(self.max_grad_norm) / (norm + f32(1e-6)))
            c["clipped"] += int(scale < 1.0)
            c["grad_norm_max"] = max(c["grad_norm_max"], float(norm))
            c["grad_norm_sum"] += float(norm)
            c["calls"] += 1
        c["skipped_kl"] += int(self.kl_stopped)
        c["grad_norm"] = float(norm)
        if skip:
            return False
        if self.max_grad_norm is not None:
            for g in grads:
                g.mul_(float(scale))
        lr = float(f32(self.base_lr) * f32(self.lr_mult) * f32(self.kl_lr_mult))
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        self.opt.step()
        return True


def _approx_kl(logp, old_logp):
    """mean((ratio - 1) - log ratio), the estimator of orr_ppo_head_logstd's stats[3]."""
    log_ratio = (logp - old_logp).detach()
    return ((log_ratio.exp() - 1.0) - log_ratio).mean()


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


class PPO(_UpdateControl):
    """With a learn-std model (ActorCritic(learn_std=True)) the loss gains -ent_coef * H (pol_entpen, agents/ppo_imitation.py:196-210),
    log_std is clamped to log_std_bounds after every optimiser step, and update() returns the five STAT_NAMES.  A fixed-std model is the
    code path it always was and returns (surrogate, value loss); ent_coef != 0 is refused for it, the term would have no gradient.
    max_grad_norm, kl_stop, kl_target / kl_lr_bounds and set_lr_mult(): _UpdateControl."""

    _history = False            # PPOHistory alone takes a model with an encoder

    def __init__(self, model, clip_param=0.2, lr=1e-5, adam_eps=1e-5, minibatch=4096, vf_coef=1.0, group=None, ent_coef=0.0,
                 log_std_bounds=LOG_STD_BOUNDS, max_grad_norm=None, kl_stop=None, kl_target=None, kl_lr_bounds=KL_LR_BOUNDS):
        import torch
        self.torch = torch
        if not self._history:
            _no_history(model, "PPO")
        self.model = model
        self.learn_std, self.ent_coef, self.log_std_bounds = _entropy_args(model, type(self).__name__, ent_coef, log_std_bounds)
        self.clip = clip_param
        self.minibatch = int(minibatch)
        self.vf_coef = vf_coef
        self.group = group
        params = model.parameters()
        # one fused multi-tensor kernel per step on the GPU (the default foreach path is ~7 launches, 0.2 ms per step)
        self.opt = torch.optim.Adam(params, lr=lr, eps=adam_eps, fused=bool(params and params[0].is_cuda))
        self._control_init(max_grad_norm, kl_stop, kl_target, kl_lr_bounds)

    def _mean_kl(self, logp, old_logp):
        """The minibatch's approx_kl for the KL rules, averaged over the ranks so that every replica decides alike; None when no rule is on."""
        if not self.kl_on:
            return None
        import torch.distributed as dist
        kl = _approx_kl(logp, old_logp)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(kl, group=self.group)
            kl = kl / dist.get_world_size(self.group)
        return kl

    def _allreduce_grads(self):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self.group) == 1:
            return
        t = self.torch
        params = [p for p in self.model.parameters() if p.grad is not None]
        flat = t.cat([p.grad.reshape(-1) for p in params])
        dist.all_reduce(flat, group=self.group)
        flat /= dist.get_world_size(self.group)
        off = 0
        for p in params:
            n = p.grad.numel()
            p.grad.copy_(flat[off:off + n].view_as(p.grad))
            off += n

    def update(self, obs, actions, adv, ret, old_logp=None, epochs=1, generator=None, priv=None):
        """obs [B,160], actions [B,12] (unclipped samples), adv [B] (already normalised), ret [B] (TD(lambda) targets); priv [B,48] the
        privileged observations, for a model with a privileged critic."""
        t = self.torch
        B = obs.shape[0]
        if (priv is not None) != (getattr(self.model, "priv_dim", 0) > 0):
            raise ValueError("priv is needed by a privileged critic and by no other")
        # a privileged actor (model.actor_priv_dim) reads the same rows
        actor_priv = (lambda x: (x,)) if getattr(self.model, "actor_priv_dim", 0) else (lambda x: ())
        if old_logp is None:
            with t.no_grad():
                old_logp = self.model.log_prob(obs, actions, *actor_priv(priv))
        stats = []
        self._begin_update()
        for _ in range(epochs):
            perm = t.randperm(B, device=obs.device, generator=generator)
            # one gather per epoch; the minibatches are then contiguous views
            obs_p, act_p, adv_p, ret_p, old_p = obs[perm], actions[perm], adv[perm], ret[perm], old_logp[perm]
            priv_p = None if priv is None else priv[perm]
            for s in range(0, B, self.minibatch):
                e = s + self.minibatch
                logp = self.model.log_prob(obs_p[s:e], act_p[s:e], *actor_priv(None if priv_p is None else priv_p[s:e]))
                ratio = t.exp(logp - old_p[s:e])
                a = adv_p[s:e]
                surr = -t.min(ratio * a, t.clamp(ratio, 1.0 - self.clip, 1.0 + self.clip) * a).mean()
                v = self.model.value(obs_p[s:e]) if priv_p is None else self.model.value(obs_p[s:e], priv_p[s:e])
                vf = ((v - ret_p[s:e]) ** 2).mean()
                loss = surr + self.vf_coef * vf
                if self.learn_std:
                    ent = self.model.p[LOGSTD].sum() + ENTROPY_CONST
                    loss = loss - self.ent_coef * ent
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._allreduce_grads()
                self._step(self._mean_kl(logp, old_p[s:e]))
                if self.learn_std:
                    with t.no_grad():
                        self.model.p[LOGSTD].clamp_(*self.log_std_bounds)
                        log_ratio = (logp - old_p[s:e]).detach()
                        r = ratio.detach()
                        kl = ((r - 1.0) - log_ratio).mean()
                        clipped = ((r < 1.0 - self.clip) | (r > 1.0 + self.clip)).to(r.dtype).mean()
                if hasattr(self.model, "mark_updated"):
                    self.model.mark_updated()
                if self.learn_std:
                    stats.append(t.stack((surr.detach(), vf.detach(), ent.detach(), kl, clipped)))
                else:
                    stats.append(t.stack((surr.detach(), vf.detach())))   # stays on the device: no sync per minibatch
        return t.stack(stats).mean(dim=0).cpu().numpy()


class PPOHistory(PPO):
    """PPO on a history policy with an asymmetric critic, in plain torch (RMA's third phase, or one-stage training with an auxiliary
    estimation loss; the fp32 reference of learner_hip.FusedPPOHistory).  The actor reads obs | encode(hist) and is trained by the clipped
    surrogate, the gradient flowing through its layer 0 into the encoder; the critic reads obs | priv, the TRUE privileged row:
      loss = surrogate(log_prob(obs, a, hist=hist)) + vf_coef * mean((value(obs, priv) - ret)^2) [- ent_coef * H]
             + latent_coef * mean_i sum_c (encode(hist)_ic - priv_ic)^2
    All parameters train: actor, critic, encoder, and the log-std of a learn-std model.  update() returns PPO's stats followed by the latent
    loss, which is reported even when its coefficient is 0."""

    _history = True

    def __init__(self, model, clip_param=0.2, lr=1e-5, adam_eps=1e-5, minibatch=4096, vf_coef=1.0, group=None, ent_coef=0.0,
                 log_std_bounds=LOG_STD_BOUNDS, latent_coef=0.0, max_grad_norm=None, kl_stop=None, kl_target=None, kl_lr_bounds=KL_LR_BOUNDS):
        if not getattr(model, "history", 0):
            raise ValueError("PPOHistory: the model needs a history encoder (ActorCritic(history=16)); a model without is trained by PPO")
        self.latent_coef = float(latent_coef)
        if not (self.latent_coef >= 0.0 and math.isfinite(self.latent_coef)):
            raise ValueError("PPOHistory: latent_coef must be finite and not negative")
        PPO.__init__(self, model, clip_param, lr, adam_eps, minibatch, vf_coef, group, ent_coef, log_std_bounds, max_grad_norm, kl_stop, kl_target,
                     kl_lr_bounds)

    def update(self, obs, hist, priv, actions, adv, ret, old_logp=None, epochs=1, generator=None):
        """obs [B,160], hist [B,512] (history_push), priv [B,48] (env.privileged_obs on the same states), actions [B,12] (unclipped
        samples), adv [B] (already normalised), ret [B] (TD(lambda) targets)."""
        t = self.torch
        B = obs.shape[0]
        if tuple(hist.shape) != (B, HISTORY_DIM) or tuple(priv.shape) != (B, pol.PRIV_DIM):
            raise ValueError("PPOHistory: hist must have shape (%d, %d) and priv (%d, %d)" % (B, HISTORY_DIM, B, pol.PRIV_DIM))
        if old_logp is None:
            with t.no_grad():
                old_logp = self.model.log_prob(obs, actions, hist=hist)
        stats = []
        self._begin_update()
        for _ in range(epochs):
            perm = t.randperm(B, device=obs.device, generator=generator)
            obs_p, hist_p, priv_p, act_p, adv_p, ret_p, old_p = (x[perm] for x in (obs, hist, priv, actions, adv, ret, old_logp))
            for s in range(0, B, self.minibatch):
                e = s + self.minibatch
                z = self.model.encode(hist_p[s:e])             # one encode() for the actor and the latent loss
                logp = self.model.log_prob(obs_p[s:e], act_p[s:e], priv=z)
                ratio = t.exp(logp - old_p[s:e])
                a = adv_p[s:e]
                surr = -t.min(ratio * a, t.clamp(ratio, 1.0 - self.clip, 1.0 + self.clip) * a).mean()
                vf = ((self.model.value(obs_p[s:e], priv_p[s:e]) - ret_p[s:e]) ** 2).mean()
                latent = ((z - priv_p[s:e]) ** 2).sum(dim=1).mean()
                loss = surr + self.vf_coef * vf
                if self.learn_std:
                    ent = self.model.p[LOGSTD].sum() + ENTROPY_CONST
                    loss = loss - self.ent_coef * ent
                if self.latent_coef != 0.0:
                    loss = loss + self.latent_coef * latent
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._allreduce_grads()
                self._step(self._mean_kl(logp, old_p[s:e]))
                row = [surr.detach(), vf.detach()]
                if self.learn_std:
                    with t.no_grad():
                        self.model.p[LOGSTD].clamp_(*self.log_std_bounds)
                        log_ratio = (logp - old_p[s:e]).detach()
                        r = ratio.detach()
                        row += [ent.detach(), ((r - 1.0) - log_ratio).mean(), ((r < 1.0 - self.clip) | (r > 1.0 + self.clip)).to(r.dtype).mean()]
                if hasattr(self.model, "mark_updated"):
                    self.model.mark_updated()
                stats.append(t.stack(row + [latent.detach()]))
        return t.stack(stats).mean(dim=0).cpu().numpy()


class Distill(_UpdateControl):
    """Policy distillation in plain torch (DAgger's supervised step; the fp32 reference of learner_hip.FusedDistill): the student's mean is
    regressed on a teacher's, loss = mean over the samples of sum_j (mean_j - target_j)^2.  Only the actor (model/pi*) is trained; the
    critic's parameters are not touched and have no optimiser state.  The student is a plain policy (actor_priv_dim = 0)."""

    def __init__(self, student, lr=1e-4, adam_eps=1e-5, minibatch=4096, max_grad_norm=None):
        import torch
        self.torch = torch
        _no_history(student, "Distill")
        if getattr(student, "actor_priv_dim", 0):
            raise ValueError("Distill: the student's actor must read the 160 observation words only")
        self.model = student
        self.minibatch = int(minibatch)
        params = [student.p[k] for k in sorted(student.p) if k.startswith("model/pi") and k != LOGSTD]     # a log-std is neither read nor trained here
        self.opt = torch.optim.Adam(params, lr=lr, eps=adam_eps, fused=bool(params and params[0].is_cuda))
        self._control_init(max_grad_norm)            # max_grad_norm and set_lr_mult(): _UpdateControl

    def update(self, obs, target_mean, epochs=1, generator=None):
        """obs [B,160], target_mean [B,12] (the teacher's actor output on the same states); returns the mean loss over the minibatches."""
        t = self.torch
        B = obs.shape[0]
        stats = []
        for _ in range(epochs):
            perm = t.randperm(B, device=obs.device, generator=generator)
            obs_p, tgt_p = obs[perm], target_mean[perm]
            for s in range(0, B, self.minibatch):
                e = s + self.minibatch
                loss = ((self.model.mean(obs_p[s:e]) - tgt_p[s:e]) ** 2).sum(dim=1).mean()
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._step()
                if hasattr(self.model, "mark_updated"):
                    self.model.mark_updated()
                stats.append(loss.detach())
        return float(t.stack(stats).mean())


class DistillHistory(_UpdateControl):
    """The learner of a history student's encoder in plain torch (RMA's second phase; the fp32 reference of learner_hip.FusedDistillHistory):
    encode(hist) is regressed on the recorded privileged rows, loss = mean over the samples of sum_j (z_j - priv_j)^2.  Only model/enc_* train;
    the actor and the critic - the teacher's - are not touched and have no optimiser state.

    action_coef > 0 adds the action loss ("Learning quadrupedal locomotion over challenging terrain": action imitation next to the latent
    regression): loss = action_coef * mean_i sum_j (actor(obs, encode(hist))_ij - target_mean_ij)^2 + latent_coef * the loss above, the
    gradient flowing through the frozen actor into the encoder.  update() then takes obs and the teacher's means as well.  The defaults
    (0, 1) are the latent regression alone, by the code path it always had."""

    def __init__(self, student, lr=1e-4, adam_eps=1e-5, minibatch=4096, action_coef=0.0, latent_coef=1.0, max_grad_norm=None):
        import torch
        self.torch = torch
        if not getattr(student, "history", 0):
            raise ValueError("DistillHistory: the student needs a history encoder (ActorCritic(history=16))")
        self.model = student
        self.minibatch = int(minibatch)
        self.action_coef, self.latent_coef = float(action_coef), float(latent_coef)
        if self.action_coef < 0.0 or self.latent_coef < 0.0:
            raise ValueError("DistillHistory: action_coef and latent_coef must not be negative")
        self.last_latent_loss = self.last_action_loss = None     # the means over the last update's minibatches
        params = [student.p[k] for k in sorted(student.p) if k.startswith("model/enc_")]
        self.params = params
        self.opt = torch.optim.Adam(params, lr=lr, eps=adam_eps, fused=bool(params and params[0].is_cuda))
        self._control_init(max_grad_norm)            # max_grad_norm and set_lr_mult(): _UpdateControl

    def update(self, hist, target_priv, epochs=1, generator=None, obs=None, target_mean=None):
        """hist [B,512], target_priv [B,48] (env.privileged_obs on the same states); with action_coef > 0 also obs [B,160] and target_mean [B,12]
        (the teacher's actor output on the same states).  Returns the mean total loss over the minibatches."""
        t = self.torch
        B = hist.shape[0]
        plain = self.action_coef == 0.0 and self.latent_coef == 1.0
        if self.action_coef > 0.0:
            if obs is None or target_mean is None:
                raise ValueError("DistillHistory: action_coef > 0 needs obs and target_mean")
            if tuple(obs.shape) != (B, 160) or tuple(target_mean.shape) != (B, 12):
                raise ValueError("DistillHistory: obs must have shape (%d, 160) and target_mean (%d, 12)" % (B, B))
        stats, lat, act = [], [], []
        for _ in range(epochs):
            perm = t.randperm(B, device=hist.device, generator=generator)
            hist_p, tgt_p = hist[perm], target_priv[perm]
            if self.action_coef > 0.0:
                obs_p, mean_p = obs[perm], target_mean[perm]
            for s in range(0, B, self.minibatch):
                e = s + self.minibatch
                self.opt.zero_grad(set_to_none=True)
                if self.action_coef > 0.0:      # z feeds the frozen actor as well: model.mean(obs, hist=hist) with the one encode() shared
                    z = self.model.encode(hist_p[s:e])
                    latent = ((z - tgt_p[s:e]) ** 2).sum(dim=1).mean()
                    action = ((self.model.mean(obs_p[s:e], priv=z) - mean_p[s:e]) ** 2).sum(dim=1).mean()
                    loss = self.action_coef * action + self.latent_coef * latent
                    act.append(action.detach())
                    for p, g in zip(self.params, t.autograd.grad(loss, self.params)):      # the encoder's gradients only: the actor keeps none
                        p.grad = g
                else:
                    latent = ((self.model.encode(hist_p[s:e]) - tgt_p[s:e]) ** 2).sum(dim=1).mean()
                    loss = latent if plain else self.latent_coef * latent
                    loss.backward()
                self._step()
                if hasattr(self.model, "mark_updated"):
                    self.model.mark_updated()
                stats.append(loss.detach())
                lat.append(latent.detach())
        self.last_latent_loss = float(t.stack(lat).mean())
        self.last_action_loss = float(t.stack(act).mean()) if act else 0.0
        return float(t.stack(stats).mean())
