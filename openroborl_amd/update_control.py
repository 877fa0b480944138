"""What the torch learners (ppo) and the fused ones (learner_hip) share on the host: the checks of their arguments and of the model they are
given, and _UpdateControl, the update controls of the torch learners.  ppo re-exports every name."""
import math

import numpy as np


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
