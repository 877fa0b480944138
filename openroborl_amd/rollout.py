"""Device-resident rollout buffers + per-robot GAE.

Replaces the host-side trajectory generator (agents/imitation_runners.py:22-208) and
`add_vtarg_and_adv` (agents/ppo_imitation.py:68-93) plus the per-robot advantage normalisation
(ppo_imitation.py:329-338) with [T, N] tensors that never leave the GPU:

  obs [T,N,160], actions [T,N,12], rewards [T,N], dones [T,N], vpred [T,N], next_vpred [T,N]

Semantics kept from the reference: gamma = lam = 0.95 (run.py:113,120); the value after a finished episode is
0 and -- the reference's quirk -- so is the bootstrap value at the end of a segment
(imitation_runners.py:98-100 `last_vpred = 0.0`); advantages are standardised per robot over the segment.
Deliberate divergences: robots reset individually (auto-reset inside env.step) instead of the whole env
resetting when any robot is done, and the GAE recursion uses each robot's own done flags by default (the reference
indexes `episode_starts[(step*num_robot+i) + (1+i)]`, ppo_imitation.py:88, which reads a neighbouring
robot's flag; `legacy_gae_index=True` reproduces exactly that, for comparisons with the reference at num_robot > 1).
"""
from ._abi import HISTORY_DIM, PRIV_DIM


def _teacher_labels(teacher, obs, priv, out_mean, out_action):
    """The teacher's actor output on (obs, priv) into out_mean [N,12] and its clipped copy into out_action [N,12]: no noise, no value (a
    privileged actor's fused pass then skips the critic)."""
    fused = getattr(teacher, "fused", None)
    if fused is not None:
        if teacher._fused_dirty:
            fused.refresh()
            teacher._fused_dirty = False
        fused.forward(obs, None, out_action=out_action, out_mean=out_mean, want_value=False, priv=priv if teacher.priv_dim else None)
    else:
        import math
        import torch
        with torch.no_grad():
            out_mean.copy_(teacher.mean(obs, teacher.actor_priv(priv)))
            torch.clamp(out_mean, -2.0 * math.pi, 2.0 * math.pi, out=out_action)


def collect_rollout(env, policy, horizon, obs=None, deterministic=False, generator=None, noise=None, priv=None, teacher=None, teacher_mask=None,
                    hist=None, critic_priv=False):
    """Run `horizon` env steps of all robots.  Returns a dict of [T, N, ...] tensors + the final observation.
    noise: optional [T, N, 12] standard-normal samples for the fused policy (default: drawn from `generator`).
    A policy with a privileged critic (priv_dim > 0) also gets env.privileged_obs() at every step: "priv" [T, N, 48] and "last_priv" are
    returned; priv: the one that belongs to `obs` (the previous segment's last_priv; None = computed here with done=None).
    teacher: a second policy (a ppo.ActorCritic, usually one with a privileged actor) that labels every visited state for distillation
    (DAgger: the student `policy` drives, the teacher labels): env.privileged_obs() then follows every step whatever the student's
    priv_dim, and "teacher_mean" [T, N, 12] - the teacher's actor output on (obs[k], priv[k]) - is returned with "priv" and "last_priv".
    teacher_mask: uint8 [N]; robots with the mask set are stepped with the teacher's clipped mean instead of the student's sampled
    action ("actions" stays the student's raw sample).
    A history student (policy.history > 0) reads hist[k] in the place of priv[k]: "hist" [T, N, 512] and "last_hist" are returned next to
    "priv" and "last_priv" (the encoder's regression targets); after every step and its privileged_obs the history is pushed
    (policy_hip.history_push(obs[k + 1], dones[k], hist[k], out=hist[k + 1])).  hist: the one that belongs to `obs` (the previous segment's
    last_hist; None = computed here with done=None).
    critic_priv=True, for a history policy only (PPO on it: ppo.PPOHistory): the critic is asymmetric, step k's forward pass gets hist[k] for
    the actor and priv[k], the true row, for the value.  False: the estimate feeds both."""
    t = env.torch
    n = env.num_robot
    dev = env.device
    if obs is None:
        obs = env.reset()
    priv_dim = int(getattr(policy, "priv_dim", 0))
    history = int(getattr(policy, "history", 0))
    if teacher_mask is not None and teacher is None:
        raise ValueError("teacher_mask without a teacher")
    if critic_priv and not history:
        raise ValueError("critic_priv is for a history policy (policy.history > 0): every other critic reads what its actor reads or its own priv")
    hbuf = None
    if history:
        from . import policy_hip
        hbuf = t.empty((horizon + 1, n, HISTORY_DIM), device=dev)
        if hist is None:
            policy_hip.history_push(obs, None, None, hbuf[0])
        else:
            hbuf[0].copy_(hist)
    pbuf = None
    if priv_dim or teacher is not None:
        pbuf = t.empty((horizon + 1, n, PRIV_DIM), device=dev)
        if priv is None:
            env.privileged_obs(out=pbuf[0], done=None)
        else:
            pbuf[0].copy_(priv)
    buf = {
        "obs": t.empty((horizon, n, obs.shape[1]), device=dev), "actions": t.empty((horizon, n, 12), device=dev),
        "rewards": t.empty((horizon, n), device=dev), "dones": t.empty((horizon, n), dtype=t.bool, device=dev),
        "vpred": t.empty((horizon, n), device=dev),
    }
    if teacher is not None:
        buf["teacher_mean"], tclip = t.empty((horizon, n, 12), device=dev), t.empty((n, 12), device=dev)
    fused = getattr(policy, "fused", None) is not None
    if fused and not deterministic and noise is None:   # one launch for the whole segment's exploration noise
        noise = t.randn((horizon, n, 12), device=dev, generator=generator)
    if not fused or deterministic:
        noise = None
    for k in range(horizon):
        row = {"hist": hbuf[k]} if history else ({"priv": pbuf[k]} if priv_dim else {})     # what the policy reads next to obs
        if critic_priv:
            row["critic_priv"] = pbuf[k]
        if fused:   # one fused launch writes the raw action and the value straight into the buffers
            clipped, _, _ = policy.act(obs, deterministic=deterministic, noise=None if noise is None else noise[k],
                                       out_raw=buf["actions"][k], out_value=buf["vpred"][k], **row)
            buf["obs"][k].copy_(obs)
        else:
            clipped, raw, v = policy.act(obs, deterministic=deterministic, generator=generator, **row)
            buf["obs"][k].copy_(obs)
            buf["actions"][k].copy_(raw)
            buf["vpred"][k].copy_(v)
        if teacher is not None:
            _teacher_labels(teacher, obs, pbuf[k], buf["teacher_mean"][k], tclip)
            if teacher_mask is not None:
                clipped = t.where(teacher_mask.view(t.bool)[:, None], tclip, clipped)
        obs, rew, done, _ = env.step(clipped.contiguous())
        buf["rewards"][k].copy_(rew)
        buf["dones"][k].copy_(done.bool())
        if pbuf is not None:    # of the state the new observation belongs to; robots that just ended an episode: no contact / push words
            env.privileged_obs(out=pbuf[k + 1], done=done)
        if hbuf is not None:
            policy_hip.history_push(obs.contiguous(), buf["dones"][k], hbuf[k], hbuf[k + 1])
    buf["last_obs"] = obs
    if hbuf is not None:
        buf["hist"], buf["last_hist"] = hbuf[:horizon], hbuf[horizon]
    if pbuf is not None:
        buf["priv"], buf["last_priv"] = pbuf[:horizon], pbuf[horizon]
    if noise is not None:
        # log-probability of the sampled actions under the sampling policy: a - mean = std * noise
        import math
        if getattr(policy, "learn_std", False):     # from the tensor, on the device: -1/2 sum noise^2 - sum log_std - 6 log(2 pi)
            buf["logp"] = -0.5 * (noise * noise).sum(dim=-1) - policy.log_std.detach().sum() - 6.0 * math.log(2.0 * math.pi)
        else:
            std = float(policy.std)
            buf["logp"] = -0.5 * (noise * noise).sum(dim=-1) - 12.0 * math.log(std * math.sqrt(2.0 * math.pi))
    return buf


class GraphRollout(object):
    """collect_rollout() for the fused policy with static [T, N] buffers: the policy forward pass writes actions and values, and
    env.step_into writes observations, rewards and done flags, straight into their rows, and the segment's launches (weight
    re-pack, T x (policy, env step), log-probabilities) are captured once and replayed as ONE hipGraph.  The first segment runs
    eagerly (first launches load code objects, which a capture must not do); the capture happens on the second call.

    Kernel arguments that are passed by value - the env's configuration incl. the seed (env.seed()), the policy's std - are frozen
    into a captured graph; collect() notices when they change (env.launch_params_generation, policy.std) and captures again.

    With a privileged critic (policy.priv_dim > 0) the segment also holds priv [T + 1, N, 48]: env.privileged_obs(out=priv[k + 1],
    done=dones[k]) follows every step_into inside the captured segment, priv[k] goes to the forward pass, and "priv" / "last_priv" are
    returned.

    With a `teacher` (collect_rollout's: the student `policy` drives, the teacher labels - DAgger) the segment holds priv whatever the
    student's priv_dim, and teacher_mean [T, N, 12]: after the student's forward pass the teacher's (no noise, no value) writes
    teacher_mean[k] from (obs[k], priv[k]), and the robots whose `teacher_mask` (uint8 [N], a static tensor of the collector: change it
    in place between collects, no new capture) is set are stepped with the teacher's clipped mean, the others with the student's sampled
    action; "actions" stays the student's raw sample.  All of it is inside the captured segment, the teacher's weight re-pack included.

    With a history student (policy.history > 0) the segment also holds hist [T + 1, N, 512]: hist[k] goes to the forward pass in priv[k]'s
    place, and after step_into and privileged_obs the push history_push(obs[k + 1], dones[k], hist[k], out=hist[k + 1]) runs inside the
    captured segment; "hist" and "last_hist" are returned next to "priv" and "last_priv", the encoder's regression targets.  critic_priv=True
    (a history policy only; PPO on it) also hands priv[k] to the forward pass: the actor reads the estimate, the value comes from the true row
    (orr_policy_forward_history_priv).  False is the segment without, launch for launch.

    With a learned log-std (policy.learn_std) the segment opens with ONE orr_gauss_prepare over noise [T N][12]: it writes scaled [T, N, 12] =
    exp(log_std) * noise and logp, the forward passes read scaled[k] with std = 1, and no std is among the launch parameters - log_std is read
    on the device, from the copy the segment's weight re-pack renews, so the graph is captured once and replayed for good while the learner
    moves it.

    The returned tensors are views of the static buffers: they are overwritten by the next collect() (clone what must survive it,
    e.g. the last row of `dones` that the next segment's GAE takes as first_starts)."""

    def __init__(self, env, policy, horizon, teacher=None, critic_priv=False):
        t = env.torch
        if getattr(policy, "fused", None) is None or (teacher is not None and getattr(teacher, "fused", None) is None):
            raise RuntimeError("GraphRollout needs the fused policy (ActorCritic.enable_fused()); the plain path is collect_rollout()")
        self.env, self.policy, self.T, self.teacher = env, policy, int(horizon), teacher
        n, dev, T = env.num_robot, env.device, self.T
        f = lambda *shape: t.empty(shape, dtype=t.float32, device=dev)   # noqa: E731
        self.obs, self.actions, self.clipped = f(T + 1, n, 160), f(T, n, 12), f(n, 12)
        self.rewards, self.vpred, self.noise, self.logp = f(T, n), f(T, n), f(T, n, 12), f(T, n)
        self.dones = t.zeros((T, n), dtype=t.uint8, device=dev)
        self.priv_dim = int(getattr(policy, "priv_dim", 0))
        self.priv = f(T + 1, n, self.priv_dim or PRIV_DIM) if (self.priv_dim or teacher is not None) else None
        self.history = int(getattr(policy, "history", 0))
        self.hist = f(T + 1, n, HISTORY_DIM) if self.history else None
        if critic_priv and not self.history:
            raise ValueError("critic_priv is for a history policy (policy.history > 0)")
        self.critic_priv = bool(critic_priv)
        if teacher is not None:
            self.teacher_mean, self.teacher_clipped, self.step_action = f(T, n, 12), f(n, 12), f(n, 12)
            self.teacher_mask = t.zeros(n, dtype=t.uint8, device=dev)
        self.learn_std = bool(getattr(policy, "learn_std", False))
        self.scaled = f(T, n, 12) if self.learn_std else None
        self.graph, self.calls = None, 0
        self._captured_for = None          # (env.launch_params_generation, policy.std) the graph was captured with

    def _launch_params(self):
        if self.learn_std:         # no std by value: the twelve are read on the device
            return (getattr(self.env, "launch_params_generation", 0),)
        return (getattr(self.env, "launch_params_generation", 0), float(self.policy.std))

    def _segment(self):
        import math
        from . import policy_hip
        t, env, fused = self.env.torch, self.env, self.policy.fused
        fused.refresh()                   # inside the graph: every replay re-packs the weights the learner has just updated
        if self.teacher is not None:
            self.teacher.fused.refresh()
        noise, more = self.noise, {}
        if self.learn_std:
            T, n = self.T, self.env.num_robot
            fused.prepare(self.noise.view(T * n, 12), self.scaled.view(T * n, 12), self.logp.view(T * n))
            noise, more = self.scaled, {"scaled": True}
        for k in range(self.T):
            if self.critic_priv:
                fused.forward(self.obs[k], noise[k], out_action=self.clipped, out_raw=self.actions[k], out_value=self.vpred[k], hist=self.hist[k],
                              critic_priv=self.priv[k], **more)
            elif self.history:
                fused.forward(self.obs[k], noise[k], out_action=self.clipped, out_raw=self.actions[k], out_value=self.vpred[k], hist=self.hist[k], **more)
            elif self.priv_dim:
                fused.forward(self.obs[k], noise[k], out_action=self.clipped, out_raw=self.actions[k], out_value=self.vpred[k], priv=self.priv[k], **more)
            else:
                fused.forward(self.obs[k], noise[k], out_action=self.clipped, out_raw=self.actions[k], out_value=self.vpred[k], **more)
            action = self.clipped
            if self.teacher is not None:
                self.teacher.fused.forward(self.obs[k], None, out_action=self.teacher_clipped, out_mean=self.teacher_mean[k], want_value=False,
                                           priv=self.priv[k] if self.teacher.priv_dim else None)
                action = t.where(self.teacher_mask.view(t.bool)[:, None], self.teacher_clipped, self.clipped, out=self.step_action)
            env.step_into(action, self.obs[k + 1], self.rewards[k], self.dones[k])
            if self.priv is not None:
                env.privileged_obs(out=self.priv[k + 1], done=self.dones[k])
            if self.history:
                policy_hip.history_push(self.obs[k + 1], self.dones[k], self.hist[k], self.hist[k + 1])
        if self.learn_std:
            return                        # orr_gauss_prepare wrote logp
        # log-probability of the sampled actions under the sampling policy: a - mean = std * noise
        t.sum(self.noise * self.noise, dim=-1, out=self.logp)
        self.logp.mul_(-0.5).sub_(12.0 * math.log(float(self.policy.std) * math.sqrt(2.0 * math.pi)))

    def collect(self, obs, generator=None, noise=None, priv=None, hist=None):
        """priv: the privileged observation that belongs to `obs` (the previous segment's "last_priv"), for a policy with a privileged
        critic; None = computed here with done=None (right after a reset; otherwise the contact and push words start as zeros).
        hist: likewise the history that belongs to `obs` (the previous segment's "last_hist"), for a history student; None = obs's frame
        in every slot."""
        t, env = self.env.torch, self.env
        with t.no_grad():
            if obs.data_ptr() != self.obs[0].data_ptr():
                self.obs[0].copy_(obs)
            if self.hist is not None:
                if hist is None:
                    from . import policy_hip
                    policy_hip.history_push(self.obs[0], None, None, self.hist[0])
                elif hist.data_ptr() != self.hist[0].data_ptr():
                    self.hist[0].copy_(hist)
            if self.priv is not None:
                if priv is None:
                    env.privileged_obs(out=self.priv[0], done=None)
                elif priv.data_ptr() != self.priv[0].data_ptr():
                    self.priv[0].copy_(priv)
            if noise is not None:
                self.noise.copy_(noise)
            else:
                self.noise.normal_(generator=generator)
            self.calls += 1
            if self.calls == 1:
                self._segment()
            else:
                # the captured launches carry the env's configuration (seed) and the policy's std as BY-VALUE kernel arguments: a graph
                # captured before env.seed(new) / a new std would silently replay the old values - drop it and capture again
                if self.graph is not None and self._captured_for != self._launch_params():
                    self.graph = None
                if self.graph is None:
                    self._captured_for = self._launch_params()
                    counter = env._env_step_counter
                    self.graph = t.cuda.CUDAGraph()
                    with t.cuda.graph(self.graph):
                        self._segment()
                    env._env_step_counter = counter          # the capture launched nothing
                self.graph.replay()
                env._env_step_counter += self.T
            self.policy._fused_dirty = False
            if self.teacher is not None:
                self.teacher._fused_dirty = False
        buf = {"obs": self.obs[:self.T], "actions": self.actions, "rewards": self.rewards, "dones": self.dones.view(t.bool),
               "vpred": self.vpred, "logp": self.logp, "last_obs": self.obs[self.T]}
        if self.priv is not None:
            buf["priv"], buf["last_priv"] = self.priv[:self.T], self.priv[self.T]
        if self.hist is not None:
            buf["hist"], buf["last_hist"] = self.hist[:self.T], self.hist[self.T]
        if self.teacher is not None:
            buf["teacher_mean"] = self.teacher_mean
        return buf


def legacy_nonterminal(dones, first_starts=None):
    """The flags the reference's recursion actually reads for num_robot > 1: `1 - episode_starts[(step*N+i) + (1+i)]` of the flat
    [T*N] (+ N x False) array (agents/ppo_imitation.py:75,88), with episode_starts[t] = done[t-1] (imitation_runners.py:178) and
    `first_starts` ([N] bool, default all True) for the first step of the segment."""
    import torch
    T, n = dones.shape
    starts = torch.empty((T + 1, n), dtype=torch.bool, device=dones.device)
    starts[0] = True if first_starts is None else first_starts.to(torch.bool)
    starts[1:T] = dones[:-1]
    flat = torch.cat([starts[:T].reshape(-1), torch.zeros(2 * n, dtype=torch.bool, device=dones.device)])
    idx = (torch.arange(T, device=dones.device)[:, None] * n + 2 * torch.arange(n, device=dones.device)[None, :] + 1)
    return ~flat[idx]


def gae(rewards, vpred, dones, gamma=0.95, lam=0.95, bootstrap=None, legacy_gae_index=False, first_starts=None):
    """Per-robot GAE(lambda) on [T, N] tensors.  next value = vpred[t+1] unless the episode ended at t (then 0);
    at the end of the segment `bootstrap` ([N], default 0 like the reference).  legacy_gae_index=True reproduces the reference's
    neighbouring-robot flag index in the recursion (see legacy_nonterminal; identical for N = 1)."""
    import torch
    T, n = rewards.shape
    nonterminal = (~dones).to(rewards.dtype)
    nxt = torch.empty_like(vpred)
    nxt[:-1] = vpred[1:]
    nxt[-1] = 0.0 if bootstrap is None else bootstrap
    nxt = nxt * nonterminal
    delta = rewards + gamma * nxt - vpred
    rec = legacy_nonterminal(dones, first_starts).to(rewards.dtype) if legacy_gae_index else nonterminal
    adv = torch.empty_like(rewards)
    last = torch.zeros(n, dtype=rewards.dtype, device=rewards.device)
    for k in range(T - 1, -1, -1):
        last = delta[k] + gamma * lam * rec[k] * last
        adv[k] = last
    return adv, adv + vpred


def normalize_per_robot(adv, eps=0.0):
    """ppo_imitation.py:329-338: (a - mean) / std over each robot's own samples (population std, like numpy)."""
    return (adv - adv.mean(dim=0, keepdim=True)) / (adv.std(dim=0, unbiased=False, keepdim=True) + eps)


def gae_fused(rewards, vpred, dones, gamma=0.95, lam=0.95, bootstrap=None, normalize=True, eps=0.0, legacy_gae_index=False, first_starts=None):
    """gae() + normalize_per_robot() in one HIP launch (include/openroborl_policy.h: orr_gae_flags).  GPU tensors only;
    returns (advantages [T,N] - standardised per robot when `normalize` -, TD(lambda) targets [T,N])."""
    import ctypes as C
    import torch
    from . import _lib
    L = _lib.load()
    T, n = rewards.shape
    rewards, vpred = rewards.contiguous(), vpred.contiguous()
    d8 = dones.to(torch.uint8).contiguous()
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    boot = None if bootstrap is None else bootstrap.to(rewards.dtype).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream)
    fs = None if first_starts is None else first_starts.to(torch.uint8).contiguous()
    flags = (1 if normalize else 0) | (2 if legacy_gae_index else 0)          # ORR_GAE_NORMALIZE | ORR_GAE_LEGACY_INDEX
    _lib.check(L.orr_gae_flags(rewards.data_ptr(), vpred.data_ptr(), d8.data_ptr(), None if fs is None else fs.data_ptr(),
                               None if boot is None else boot.data_ptr(), int(T), int(n), float(gamma), float(lam), flags, float(eps),
                               adv.data_ptr(), ret.data_ptr(), stream), L)
    return adv, ret
