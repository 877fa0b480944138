"""PPO learner in PyTorch-ROCm -- the consumer of rollout.py's [T, N] buffers.

Restates the update of agents/ppo_imitation.py:156-258,352-382 (stable-baselines PPO1 graph) without TF1/MPI:
  * actor 160 -> 512 -> 256 -> 12 and critic 160 -> 512 -> 256 -> 1, ReLU (run.py:101-105), fixed-variance diagonal
    Gaussian, std 0.125 (agents/imitation_policies.py:44-51,96-107);
  * clipped surrogate with clip_param 0.2, value loss mean((v - tdlamret)^2), Adam lr 1e-5, eps 1e-5, one epoch over
    the segment (run.py:111-125; ppo1/pposgd_simple.py loss terms);
  * data-parallel: one process per GPU, gradients averaged with ONE all-reduce of a flat 1.7 MB buffer per minibatch
    (RCCL over xGMI; replaces MpiAdam's Allreduce, stable_baselines/common/mpi_adam.py:40-62).
The env never leaves the device, so a full iteration is: collect_rollout -> gae -> normalize_per_robot -> update.

This module holds the four torch learners - PPO, PPOHistory, Distill, DistillHistory: the float32 yardsticks of learner_hip's - and is the
public face of what they train and share, which lives in actor_critic.py (ActorCritic and its layers), obs_norm.py (RunningNorm),
history.py (the sensor history) and update_control.py (the argument checks and _UpdateControl): every name of theirs is a name of ppo.
"""
import math

from . import policy as pol
from .actor_critic import ENTROPY_CONST, LOG_STD_BOUNDS, LOGSTD, STAT_NAMES, ActorCritic, _linear, _wgrad  # noqa: F401
from .history import ENC_HIDDEN, HISTORY_DIM, HISTORY_FRAME, HISTORY_STEPS, history_frame, history_push  # noqa: F401
from .obs_norm import NORM_EPS, NORM_KEYS, RunningNorm, _norm_state  # noqa: F401
from .update_control import KL_LR_BOUNDS, _control_args, _entropy_args, _no_history, _no_obs_norm, _UpdateControl  # noqa: F401


def _approx_kl(logp, old_logp):
    """mean((ratio - 1) - log ratio), the estimator of orr_ppo_head_logstd's stats[3]."""
    log_ratio = (logp - old_logp).detach()
    return ((log_ratio.exp() - 1.0) - log_ratio).mean()


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

    def _mean_kl(self, kl):
        """The minibatch's approx_kl for the KL rules, averaged over the ranks so that every replica decides alike; None when no rule is on."""
        if not self.kl_on:
            return None
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            kl = kl.clone()                      # this rank's own stays what update() reports
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

    def _actor_priv(self, priv):
        """log_prob()'s arguments behind the actions: a privileged actor (model.actor_priv_dim) reads the critic's rows."""
        return (priv,) if getattr(self.model, "actor_priv_dim", 0) else ()

    def _forward(self, mb):
        """A minibatch's (log-probabilities, values, further loss terms as (coefficient, term) pairs); mb: the batch's tensors by name.  A
        further term is reported behind PPO's stats whatever its coefficient, and enters the loss unless that is 0."""
        priv = mb.get("priv")
        logp = self.model.log_prob(mb["obs"], mb["actions"], *self._actor_priv(priv))
        return logp, (self.model.value(mb["obs"]) if priv is None else self.model.value(mb["obs"], priv)), ()

    def _update(self, batch, epochs, generator):
        """The PPO epochs over `batch`: [B, ...] tensors by name, obs, actions, adv, ret and old_logp among them, and what _forward reads."""
        t = self.torch
        B = batch["obs"].shape[0]
        stats = []
        self._begin_update()
        for _ in range(epochs):
            perm = t.randperm(B, device=batch["obs"].device, generator=generator)
            # one gather per epoch; the minibatches are then contiguous views
            shuffled = {k: x[perm] for k, x in batch.items()}
            for s in range(0, B, self.minibatch):
                mb = {k: x[s:s + self.minibatch] for k, x in shuffled.items()}
                logp, v, more = self._forward(mb)
                ratio = t.exp(logp - mb["old_logp"])
                a = mb["adv"]
                surr = -t.min(ratio * a, t.clamp(ratio, 1.0 - self.clip, 1.0 + self.clip) * a).mean()
                vf = ((v - mb["ret"]) ** 2).mean()
                loss = surr + self.vf_coef * vf
                if self.learn_std:
                    ent = self.model.p[LOGSTD].sum() + ENTROPY_CONST
                    loss = loss - self.ent_coef * ent
                for coef, term in more:
                    if coef != 0.0:
                        loss = loss + coef * term
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._allreduce_grads()
                kl = _approx_kl(logp, mb["old_logp"]) if (self.learn_std or self.kl_on) else None
                self._step(self._mean_kl(kl))
                row = [surr.detach(), vf.detach()]       # stays on the device: no sync per minibatch
                if self.learn_std:
                    with t.no_grad():
                        self.model.p[LOGSTD].clamp_(*self.log_std_bounds)
                        r = ratio.detach()
                        row += [ent.detach(), kl, ((r < 1.0 - self.clip) | (r > 1.0 + self.clip)).to(r.dtype).mean()]
                if hasattr(self.model, "mark_updated"):
                    self.model.mark_updated()
                stats.append(t.stack(row + [term.detach() for _, term in more]))
        return t.stack(stats).mean(dim=0).cpu().numpy()

    def update(self, obs, actions, adv, ret, old_logp=None, epochs=1, generator=None, priv=None):
        """obs [B,160], actions [B,12] (unclipped samples), adv [B] (already normalised), ret [B] (TD(lambda) targets); priv [B,48] the
        privileged observations, for a model with a privileged critic."""
        if (priv is not None) != (getattr(self.model, "priv_dim", 0) > 0):
            raise ValueError("priv is needed by a privileged critic and by no other")
        if old_logp is None:
            with self.torch.no_grad():
                old_logp = self.model.log_prob(obs, actions, *self._actor_priv(priv))
        batch = dict(obs=obs, actions=actions, adv=adv, ret=ret, old_logp=old_logp)
        if priv is not None:
            batch["priv"] = priv
        return self._update(batch, epochs, generator)


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

    def _forward(self, mb):
        z = self.model.encode(mb["hist"])             # one encode() for the actor and the latent loss
        logp = self.model.log_prob(mb["obs"], mb["actions"], priv=z)
        v = self.model.value(mb["obs"], mb["priv"])
        return logp, v, ((self.latent_coef, ((z - mb["priv"]) ** 2).sum(dim=1).mean()),)

    def update(self, obs, hist, priv, actions, adv, ret, old_logp=None, epochs=1, generator=None):
        """obs [B,160], hist [B,512] (history_push), priv [B,48] (env.privileged_obs on the same states), actions [B,12] (unclipped
        samples), adv [B] (already normalised), ret [B] (TD(lambda) targets)."""
        B = obs.shape[0]
        if tuple(hist.shape) != (B, HISTORY_DIM) or tuple(priv.shape) != (B, pol.PRIV_DIM):
            raise ValueError("PPOHistory: hist must have shape (%d, %d) and priv (%d, %d)" % (B, HISTORY_DIM, B, pol.PRIV_DIM))
        if old_logp is None:
            with self.torch.no_grad():
                old_logp = self.model.log_prob(obs, actions, hist=hist)
        return self._update(dict(obs=obs, hist=hist, priv=priv, actions=actions, adv=adv, ret=ret, old_logp=old_logp), epochs, generator)


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
