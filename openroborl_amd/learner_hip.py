"""The four learners whose non-GEMM part is hand-written HIP and whose whole epoch replays as one hipGraph
(include/openroborl_learner.h, csrc/orr_learner.hip):
  FusedPPO             the PPO update of both nets (the torch reference is ppo.PPO: agents/ppo_imitation.py:156-258 + Adam);
  FusedPPOHistory      that update on a history policy: the actor on obs | encode(hist), the critic on the true privileged row (ppo.PPOHistory);
  FusedDistill         a student's actor regressed on a teacher's means (ppo.Distill);
  FusedDistillHistory  a history student's encoder regressed on the privileged rows, optionally through the frozen actor (ppo.DistillHistory).
Same arithmetic as their references (which stay the fp32 yardsticks the tests compare these against), different execution.  What they
share stands once, in _FusedLearner:
  * the trained parameters, their gradients and Adam moments live in ONE flat buffer each (the model's tensors become views of it): the
    gradient all-reduce needs no packing and Adam is one launch (434 k floats for PPO);
  * a plan per (samples, minibatch) of static buffers: forward = GEMMs with bias(+ReLU) epilogues writing into static activations; backward =
    GEMMs written out by hand (no autograd graph) with the ReLU masks, the gradient through an output layer of fan-out 12 or 1 (no GEMM),
    every bias gradient and the loss head in a handful of HIP launches (7 per PPO minibatch) - autograd spends ~70 elementwise / reduction
    launches per minibatch on the same work, more GPU time than the GEMMs;
  * the two chains a minibatch is made of, each as buffers / forward / backward: a 3-layer net (_mlp_*) and the history encoder (_enc_*,
    the two history learners'); where a loss lands in the minibatch's own row of stats, P["jobs_s"][s] is that minibatch's job table;
  * one update driver: an epoch (gathers of all minibatches, forward, backward, Adam) is captured once and replayed - ~30 launches per
    minibatch cost no host time.  FusedPPO alone has ranks; several ranks: one graph per minibatch, the all-reduce (RCCL) and Adam between
    replays.  ORR_FORCE_DIST=1 with an initialised process group takes the several-ranks path even for ONE rank (a one-GPU box can then run
    per-minibatch graphs + the RCCL all-reduce + Adam between replays; the result equals the one-graph path bit for bit).
Scalar hyper-parameters (lr, betas, eps, clip, vf_coef, a fixed policy std, the loss coefficients, the world size) are by-value kernel
arguments, i.e. frozen into a captured graph: the driver compares them with the values the graphs were captured with and captures again
when one changed (the reference feeds optim_stepsize * cur_lrmult every step: ppo1/pposgd_simple.py; run.py uses schedule='constant').
The update controls are the exception: with max_grad_norm, device_lr or (FusedPPO, FusedPPOHistory) a KL rule the optimiser step reads a
record in device memory (orr_update_ctl) that orr_update_control writes inside the captured epoch from the flat gradient's norm and the
minibatch's approx_kl - the clip coefficient, a guard that skips the step of a non-finite gradient, the KL stop of the rest of an update()
and the KL-adaptive learning rate -, and that set_lr_mult() writes for a schedule (the reference's schedule='linear',
agents/ppo_imitation.py:296-299): none of them captures again and none costs a host round trip; control_stats() reads the diagnostics.
Without those arguments a learner launches what it always did (orr_adam_step, self.ctl is None).
A model with an observation normaliser (ppo.ActorCritic(obs_norm=True)) is FusedPPO's alone: its update() fills the plan's static obs /
priv inputs through orr_normalize_rows instead of a copy, so the captured epoch is the one it would be without; the other three refuse it.
There is no fallback: without a GPU and the HIP library the constructors raise.
"""
import ctypes as C
import os

from . import _abi, _lib
from .actor_critic import LOG_STD_BOUNDS, LOGSTD     # LOGSTD: the learned log-std of ppo.ActorCritic(learn_std=True)
# the argument checks the torch learners share; _no_obs_norm: the learners without a normalising fill() refuse a model with a normaliser
from .update_control import KL_LR_BOUNDS, _control_args, _entropy_args, _no_obs_norm

NETS = ("pi", "vf")


def _jobs(entries):
    """The job table of an orr_colsum_finish from (partials, out, rows, cols) entries, in their order, and its length."""
    return (_abi.OrrColsumJob * len(entries))(*(_abi.OrrColsumJob(p.data_ptr(), o.data_ptr(), r, c) for p, o, r, c in entries)), len(entries)


class _FusedLearner(object):
    """What the fused learners share: the flat buffers of the parameters `names` of `model`, Adam, the plan cache, the chains of a 3-layer
    net and of the history encoder and the update driver.  A learner adds its plan's buffers (_buffers), its _minibatch and its update."""

    def __init__(self, model, names, stats, lr, adam_eps, minibatch, betas, use_graph, mpi_adam_epsilon=False, max_grad_norm=None, device_lr=False,
                 kl_stop=None, kl_target=None, kl_lr_bounds=None):
        import torch
        self.torch = torch
        self.max_grad_norm, self.kl_stop, self.kl_target, self.kl_lr_bounds = _control_args(type(self).__name__, max_grad_norm, kl_stop, kl_target,
                                                                                            kl_lr_bounds or KL_LR_BOUNDS)
        self.kl_on = self.kl_stop is not None or self.kl_target is not None
        control = self.max_grad_norm is not None or self.kl_on or bool(device_lr)
        self.model = model
        self.dev = model.device
        self.L = _lib.load()
        self.lr, self.eps, self.b1, self.b2 = float(lr), float(adam_eps), float(betas[0]), float(betas[1])
        self.minibatch = int(minibatch)
        self.adam_flags = 1 if mpi_adam_epsilon else 0          # ORR_ADAM_MPI_EPSILON
        self.use_graph = bool(use_graph)
        self.n_stats = stats                                    # losses a minibatch reports: the columns of a plan's stats
        # ---- one flat buffer for the parameters (16-byte aligned slots), the model's tensors become views of it ----
        self.slots, off = {}, 0
        for k in names:
            n = model.p[k].numel()
            self.slots[k] = (off, n, tuple(model.p[k].shape))
            off += (n + 3) // 4 * 4
        self.total = off
        z = lambda: torch.zeros(self.total, dtype=torch.float32, device=self.dev)   # noqa: E731
        self.flat_p, self.flat_g, self.m, self.v = z(), z(), z(), z()
        self.state = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.w, self.g = {}, {}
        with torch.no_grad():
            for k in names:
                o, n, shape = self.slots[k]
                self.w[k] = self.flat_p[o:o + n].view(shape)
                self.w[k].copy_(model.p[k].detach())
                self.g[k] = self.flat_g[o:o + n].view(shape)
                model.p[k] = self.w[k].detach().requires_grad_(True)        # same storage: the torch path and the zip export keep working
        self._mark_updated()
        self._plans = {}
        # ---- the update controls (orr_update_control + orr_adam_step_ctl): one orr_update_ctl on the device and the norm's partial sums ----
        self.ctl = None                      # None: the path without, orr_adam_step
        self.lr_mult = 1.0
        if control:
            self.ctl = torch.zeros(len(_abi.UPDATE_CTL_WORDS), dtype=torch.int32, device=self.dev)
            self.ctl_f = self.ctl.view(torch.float32)            # the same twelve words, for the float members
            self.ctl_f[:3].fill_(1.0)                            # lr_mult, kl_lr_mult, grad_scale
            self.ctl_partials = torch.zeros(int(self.L.orr_update_control_partials(self.total)), dtype=torch.float32, device=self.dev)

    # ---- the update controls -------------------------------------------------------------------------------------------------
    def _need_ctl(self, who):
        if self.ctl is None:
            raise RuntimeError("%s.%s needs the control path: construct the learner with device_lr=True (or max_grad_norm / a KL rule)"
                               % (type(self).__name__, who))

    def set_lr_mult(self, x):
        """The schedule's multiplier of lr from the next step on: one device word, written on the stream.  Never a capture."""
        self._need_ctl("set_lr_mult")
        self.lr_mult = float(x)
        self.ctl_f[_abi.UPDATE_CTL_WORDS.index("lr_mult")].fill_(self.lr_mult)

    def control_stats(self):
        """The diagnostics of the control path since the last call (one sync), and clears the counters on the device."""
        self._need_ctl("control_stats")
        raw = self.ctl.cpu()
        w = dict(zip(_abi.UPDATE_CTL_WORDS, zip(raw.tolist(), raw.view(self.torch.float32).tolist())))       # name -> (as int, as float)
        first = _abi.UPDATE_CTL_WORDS.index("grad_norm_max")
        self.ctl[first:].zero_()
        calls = w["n_calls"][0]
        return {"grad_norm": w["grad_norm"][1], "grad_norm_max": w["grad_norm_max"][1], "grad_norm_mean": w["grad_norm_sum"][1] / max(calls, 1),
                "calls": calls, "clipped": w["n_clipped"][0], "skipped_nonfinite": w["n_nonfinite"][0], "skipped_kl": w["n_kl_skipped"][0],
                "lr_mult": w["lr_mult"][1], "kl_lr_mult": w["kl_lr_mult"][1]}

    def _kl_ptr(self, P, s):
        """Device address of minibatch s's approx_kl for the KL rules; None: no rule (the learners without a PPO loss head)."""
        return None

    def _need_gpu(self, model):
        if model.device.type != "cuda":
            name = type(self).__name__
            raise RuntimeError("%s needs a GPU device (the torch reference is ppo.%s)" % (name, name[len("Fused"):]))

    def _mark_updated(self):
        if hasattr(self.model, "mark_updated"):
            self.model.mark_updated()

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _graph_key(self):
        key = (self.lr, self.b1, self.b2, self.eps, self.adam_flags)
        if self.ctl is not None:      # orr_update_control's by-value arguments (the multipliers and the gate live on the device: no keys)
            key += ("ctl", self.max_grad_norm, self.kl_stop, self.kl_target) + self.kl_lr_bounds
        return key

    @staticmethod
    def fit_minibatch(num_samples, minibatch):
        """Largest minibatch size <= `minibatch` that divides `num_samples` (update() needs equal minibatches: static buffers)."""
        m = max(1, min(int(minibatch), int(num_samples)))
        while num_samples % m:
            m -= 1
        return m

    def _adam(self, world, kl=None):
        """The optimiser step on flat_g; on the control path orr_update_control first (kl: _kl_ptr of the minibatch), then the step under it."""
        L, st = self.L, self._stream()
        if self.ctl is None:
            _lib.check(L.orr_adam_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.total,
                                       self.lr, self.b1, self.b2, self.eps, 1.0 / world, self.adam_flags, self.state.data_ptr(), st), L)
            return
        lo, hi = self.kl_lr_bounds
        _lib.check(L.orr_update_control(self.flat_g.data_ptr(), self.total, 1.0 / world, self.max_grad_norm or 0.0, kl, self.kl_stop or 0.0,
                                        self.kl_target or 0.0, lo, hi, self.ctl_partials.data_ptr(), self.ctl.data_ptr(), st), L)
        _lib.check(L.orr_adam_step_ctl(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.total,
                                       self.lr, self.b1, self.b2, self.eps, 1.0 / world, self.adam_flags, self.state.data_ptr(),
                                       self.ctl.data_ptr(), st), L)

    def _wgrad(self, x, g, part, out):
        """out = x^T g.  Tall batches: 16 partial products in one batched GEMM (see ppo._wgrad: the library's plain GEMM fills a
        third of the chip for these K = batch shapes); their sum is one of the jobs of the minibatch's orr_colsum_finish."""
        t = self.torch
        if part is not None:
            M = x.shape[0]
            t.bmm(x.view(16, M // 16, x.shape[1]).transpose(1, 2), g.view(16, M // 16, g.shape[1]), out=part)
        else:
            t.mm(x.t(), g, out=out)

    def _plan(self, B, M):
        """Static buffers for B samples per update in minibatches of M."""
        key = (B, M)
        if key not in self._plans:
            t = self.torch
            f = lambda *shape: t.empty(shape, dtype=t.float32, device=self.dev)   # noqa: E731
            P = {"B": B, "M": M, "nmb": B // M, "perm": t.empty(B, dtype=t.int64, device=self.dev),
                 "stats": t.zeros(B // M, self.n_stats, dtype=t.float32, device=self.dev), "graphs": None}
            # split: the weight gradients of a tall minibatch are 16 partial products (_wgrad); rows: of partial sums a kernel leaves per column
            self._buffers(P, f, M >= 4096 and M % 16 == 0, int(self.L.orr_learner_partial_rows(M)))
            self._plans[key] = P
        return self._plans[key]

    # ---- a 3-layer net model/<net>*: k0 -> 512 -> 256 -> k, its buffers under the plan keys h1<sfx>, h2<sfx>, y<sfx>, ... ------------------
    def _mlp_buffers(self, P, f, net, sfx, k0, k, split, rows):
        """The net's activations and the partial sums of its backward pass; returns the jobs that finish the two bias gradients and the
        output layer's weight gradient, and those of the two split weight gradients (none unless split).  The column sums behind them are
        deferred: each producer leaves its per-workgroup partial sums in its own buffer and ONE launch adds them all up (orr_colsum_finish)."""
        M, g = P["M"], self.g
        P["h1" + sfx], P["h2" + sfx], P["y" + sfx] = f(M, 512), f(M, 256), f(M, k)
        P["part1" + sfx], P["part0" + sfx] = (f(16, 512, 256), f(16, k0, 512)) if split else (None, None)
        ws2 = P["ws2" + sfx] = f(int(self.L.orr_learner_workspace_floats(M, 256)))      # [rows][256] | [rows][256 * 12]
        ws1 = P["ws1" + sfx] = f(rows * 512)
        sums = [(ws2, g["model/%s_fc1/b:0" % net], rows, 256), (ws2[rows * 256:], g["model/%s/w:0" % net], rows, 256 * k),
                (ws1, g["model/%s_fc0/b:0" % net], rows, 512)]
        if not split:
            return sums, []
        return sums, [(P["part1" + sfx], g["model/%s_fc1/w:0" % net], 16, 512 * 256), (P["part0" + sfx], g["model/%s_fc0/w:0" % net], 16, k0 * 512)]

    def _mlp_forward(self, P, net, sfx, x):
        t, w = self.torch, self.w
        t._addmm_activation(w["model/%s_fc0/b:0" % net], x, w["model/%s_fc0/w:0" % net], out=P["h1" + sfx])
        t._addmm_activation(w["model/%s_fc1/b:0" % net], P["h1" + sfx], w["model/%s_fc1/w:0" % net], out=P["h2" + sfx])
        t.addmm(w["model/%s/b:0" % net], P["h2" + sfx], w["model/%s/w:0" % net], out=P["y" + sfx])

    def _mlp_backward(self, P, net, sfx, x, gy, k, st):
        """From gy = d loss / d y [M, k] to the net's weight gradients and the partial sums of its bias gradients (P["gz2"], P["gh1"]: scratch)."""
        t, L, M, w, g = self.torch, self.L, P["M"], self.w, self.g
        h1 = P["h1" + sfx]
        _lib.check(L.orr_head_backward(gy.data_ptr(), k, w["model/%s/w:0" % net].data_ptr(), P["h2" + sfx].data_ptr(), M, 256, P["gz2"].data_ptr(),
                                       None, None, P["ws2" + sfx].data_ptr(), st), L)
        self._wgrad(h1, P["gz2"], P["part1" + sfx], g["model/%s_fc1/w:0" % net])
        t.mm(P["gz2"], w["model/%s_fc1/w:0" % net].t(), out=P["gh1"])
        _lib.check(L.orr_relu_backward(P["gh1"].data_ptr(), h1.data_ptr(), M, 512, None, P["ws1" + sfx].data_ptr(), st), L)
        self._wgrad(x, P["gh1"], P["part0" + sfx], g["model/%s_fc0/w:0" % net])

    # ---- the history encoder model/enc_*: 512 -> 256 -> 48, its buffers under the plan keys xh, he, z, g_z, g_he, ws1e, part0 ---------------
    def _enc_buffers(self, P, f, split, rows):
        """The encoder's activations and the partial sums of its backward pass; returns the jobs that finish enc_fc0's bias gradient and, when
        split, its weight gradient.  enc_fc1's bias gradient is left by whoever produces g_z, the learner's loss head: a job of its own."""
        M, g = P["M"], self.g
        D, H, Z = _abi.HISTORY_DIM, 256, _abi.POLICY_PRIV_DIM
        P.update({"xh": f(M, D), "he": f(M, H), "z": f(M, Z), "g_z": f(M, Z), "g_he": f(M, H), "ws1e": f(rows * H), "part0": f(16, D, H) if split else None})
        return [(P["ws1e"], g["model/enc_fc0/b:0"], rows, H)] + ([(P["part0"], g["model/enc_fc0/w:0"], 16, D * H)] if split else [])

    def _enc_forward(self, P):
        t, w = self.torch, self.w
        t._addmm_activation(w["model/enc_fc0/b:0"], P["xh"], w["model/enc_fc0/w:0"], out=P["he"])
        t.addmm(w["model/enc_fc1/b:0"], P["he"], w["model/enc_fc1/w:0"], out=P["z"])

    def _enc_backward(self, P, st):
        """From P["g_z"] = d loss / d z [M, 48] to the encoder's weight gradients and the partial sums of enc_fc0's bias gradient."""
        t, L, w, g = self.torch, self.L, self.w, self.g
        t.mm(P["he"].t(), P["g_z"], out=g["model/enc_fc1/w:0"])
        t.mm(P["g_z"], w["model/enc_fc1/w:0"].t(), out=P["g_he"])
        _lib.check(L.orr_relu_backward(P["g_he"].data_ptr(), P["he"].data_ptr(), P["M"], 256, None, P["ws1e"].data_ptr(), st), L)
        self._wgrad(P["xh"], P["g_he"], P["part0"], g["model/enc_fc0/w:0"])

    # ---- the update driver ----------------------------------------------------------------------------------------------
    def _epoch_eager(self, P, world, reduce):
        for s in range(P["nmb"]):
            self._minibatch(P, s)
            if reduce:
                reduce(P, s)
            self._adam(world, self._kl_ptr(P, s))

    def _capture(self, P, several):
        """One rank: one graph for the whole epoch.  Several ranks: one graph per minibatch (the collective runs between replays)."""
        t = self.torch
        live = (self.flat_p, self.m, self.v, self.state) + (() if self.ctl is None else (self.ctl,))
        keep = [x.clone() for x in live]
        P["perm"].copy_(t.arange(P["B"], device=self.dev))
        side = t.cuda.Stream(device=self.dev)
        side.wait_stream(t.cuda.current_stream(self.dev))
        with t.cuda.stream(side):                    # warm-up outside the capture: library handles, workspaces, kernel selection
            for _ in range(2):
                self._minibatch(P, 0)
                self._adam(1, self._kl_ptr(P, 0))
        t.cuda.current_stream(self.dev).wait_stream(side)
        graphs = []
        if not several:
            gr = t.cuda.CUDAGraph()
            with t.cuda.graph(gr):
                for s in range(P["nmb"]):
                    self._minibatch(P, s)
                    self._adam(1, self._kl_ptr(P, s))
            graphs.append(gr)
        else:
            pool = None
            for s in range(P["nmb"]):
                gr = t.cuda.CUDAGraph()
                with t.cuda.graph(gr, pool=pool):
                    self._minibatch(P, s)
                pool = pool or gr.pool()
                graphs.append(gr)
        for dst, src in zip(live, keep):     # the warm-up took real optimiser steps (and control calls): undo them
            dst.copy_(src)
        P["graphs"] = graphs

    def _run(self, B, fill, epochs, generator, world=1, reduce=None):
        """`epochs` passes over B samples: fill(P) copies the caller's tensors into the plan's static inputs, every epoch draws a permutation
        and runs its minibatches, captured or eager.  `reduce` (the several-ranks path) runs between a minibatch's gradients and its Adam step,
        of `world` ranks.  Returns the sum of the minibatches' stats rows, still on the device, and the number of minibatches behind it."""
        t = self.torch
        M = min(self.minibatch, B)
        if B % M:
            raise ValueError("%s: the number of samples (%d) must be a multiple of the minibatch size (%d); "
                             "FusedPPO.fit_minibatch(%d, %d) = %d is the largest size that divides it"
                             % (type(self).__name__, B, M, B, M, self.fit_minibatch(B, M)))
        several = reduce is not None
        with t.no_grad():
            P = self._plan(B, M)
            fill(P)
            key = self._graph_key() + (world, several)
            if self.use_graph and (P["graphs"] is None or P.get("graph_key") != key):
                self._capture(P, several)
                P["graph_key"] = key
            total = t.zeros(self.n_stats, dtype=t.float32, device=self.dev)
            if self.ctl is not None:         # the KL stop holds for one update(): clear the gate (bit 0 is rewritten by every control call)
                self.ctl[_abi.UPDATE_CTL_WORDS.index("skip")].zero_()
            for _ in range(epochs):
                P["perm"].copy_(t.randperm(B, device=self.dev, generator=generator))
                if not self.use_graph:
                    self._epoch_eager(P, world, reduce)
                elif not several:
                    P["graphs"][0].replay()
                else:
                    for s, gr in enumerate(P["graphs"]):
                        gr.replay()
                        reduce(P, s)
                        self._adam(world, self._kl_ptr(P, s))
                total += P["stats"].sum(dim=0)
        self._mark_updated()
        return total, float(epochs * P["nmb"])

    def steps_taken(self):
        return int(self.state[0].item())

    def sync(self):                 # train.py calls both on every learner; one without ranks has no replicas to compare
        pass

    def check_synced(self):
        pass


class FusedPPO(_FusedLearner):
    """The PPO update on the device, the only learner with ranks (see the module's text).

    A learn-std model (ppo.ActorCritic(learn_std=True)): model/pi/logstd:0 is one more slot of the flat buffer - Adam, the all-reduce, sync and
    check_synced cover it as they cover every slot -, the loss head is orr_ppo_head_logstd, which reads the twelve from that slot and writes
    their gradient into flat_g's (loss - ent_coef * H), and a clamp of the slot to log_std_bounds follows every orr_adam_step (inside the
    captured epoch on one rank, between replays on several).  update() then returns ppo.STAT_NAMES' five.  No std is frozen into the graphs:
    they are captured once while log_std moves.  A fixed-std model is the path it always was; ent_coef != 0 is refused for it."""

    _history = False            # FusedPPOHistory alone takes a model with an encoder

    def __init__(self, model, clip_param=0.2, lr=1e-5, adam_eps=1e-5, minibatch=4096, vf_coef=1.0, group=None, betas=(0.9, 0.999),
                 mpi_adam_epsilon=False, use_graph=True, ent_coef=0.0, log_std_bounds=None, max_grad_norm=None, device_lr=False, kl_stop=None,
                 kl_target=None, kl_lr_bounds=None):
        self._need_gpu(model)
        if getattr(model, "history", 0) and not self._history:
            raise ValueError("FusedPPO: a history policy is trained by FusedPPOHistory (PPO with the critic on the true privileged row) or by "
                             "FusedDistillHistory")
        self.learn_std, self.ent_coef, self.log_std_bounds = _entropy_args(model, type(self).__name__, ent_coef, log_std_bounds or LOG_STD_BOUNDS)
        self.clip, self.vf_coef = float(clip_param), float(vf_coef)
        self.group = group
        # a privileged critic (ppo.ActorCritic(priv_dim=48)): its layer 0 reads x | priv, [M, 160 + 48]; everything behind layer 0 and the
        # whole actor are what they are without (the kernels of orr_learner.hip see hidden and output layers only)
        self.priv_dim = int(getattr(model, "priv_dim", 0))
        # a privileged actor as well (ppo.ActorCritic(actor_priv_dim=48), a teacher): its layer 0 reads the same x | priv
        self.actor_priv_dim = int(getattr(model, "actor_priv_dim", 0))
        # a KL rule needs approx_kl on the device: the loss head is then orr_ppo_head_logstd for a fixed-std model too, on a constant buffer of
        # log(std) (renewed by every update()), with ent_coef = 0 and the log-std's gradient sent to scratch; update() still returns its two stats
        self.logstd_head = self.learn_std or kl_stop is not None or kl_target is not None
        self.head_stats = 5 if self.logstd_head else 2        # what the loss head writes; FusedPPOHistory's latent loss follows them
        _FusedLearner.__init__(self, model, sorted(model.p), self.head_stats + (1 if self._history else 0), lr, adam_eps, minibatch, betas, use_graph,
                               mpi_adam_epsilon, max_grad_norm, device_lr, kl_stop, kl_target, kl_lr_bounds)
        if self.logstd_head and not self.learn_std:
            self.fixed_logstd = self.torch.zeros(12, dtype=self.torch.float32, device=self.dev)
            self.g_fixed_logstd = self.torch.zeros(12, dtype=self.torch.float32, device=self.dev)

    def _graph_key(self):
        if self.learn_std:          # the std is read on the device: not a key
            return _FusedLearner._graph_key(self) + (self.clip, self.vf_coef, self.ent_coef) + self.log_std_bounds
        return _FusedLearner._graph_key(self) + (self.clip, self.vf_coef, float(self.model.std))

    def _adam(self, world, kl=None):
        _FusedLearner._adam(self, world, kl)
        if self.learn_std:
            self.w[LOGSTD].clamp_(*self.log_std_bounds)

    def _kl_ptr(self, P, s):
        return P["stats"][s][3:].data_ptr() if self.kl_on else None

    def _refresh_std(self):
        """A fixed-std model under a KL rule: the loss head's constant log-std buffer follows model.std."""
        if self.logstd_head and not self.learn_std:
            import math
            self.fixed_logstd.fill_(math.log(float(self.model.std)))

    def _returned(self, stats):
        """What update() returns of a minibatch's mean stats row: everything, or a fixed-std model's two (+ the latent loss) under a KL rule."""
        if self.logstd_head and not self.learn_std:
            return self.torch.cat((stats[:2], stats[5:]))
        return stats

    def _buffers(self, P, f, split, rows):
        B, M, pd = P["B"], P["M"], self.priv_dim
        P.update({"obs": f(B, 160), "aux": f(B, 16), "x": f(M, 160), "batch": f(M, 16), "gz2": f(M, 256), "gh1": f(M, 512), "g_pi": f(M, 12),
                  "g_vf": f(M), "ws": f(int(self.L.orr_learner_workspace_floats(M, 32 if self.logstd_head else 16)))})
        P["aux"].zero_()
        if pd:      # the privileged observations, gathered with the same permutation; xv = x | xp is the critic's layer-0 input
            P["priv"], P["xp"], P["xv"] = f(B, pd), f(M, pd), f(M, 160 + pd)
        pi, pi_parts = self._mlp_buffers(P, f, "pi", "_pi", 160 + self.actor_priv_dim, 12, split, rows)
        vf, vf_parts = self._mlp_buffers(P, f, "vf", "_vf", 160 + pd, 1, split, rows)
        P["jobs"], P["n_jobs"] = _jobs(pi + vf + pi_parts + vf_parts)

    def _minibatch(self, P, s):
        """Gather, forward, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M = self.torch, self.L, P["M"]
        st = self._stream()
        idx = P["perm"][s * M:(s + 1) * M]
        t.index_select(P["obs"], 0, idx, out=P["x"])
        t.index_select(P["aux"], 0, idx, out=P["batch"])
        x = P["x"]
        xin = {"pi": x, "vf": x}                   # each net's layer-0 input
        if self.priv_dim:
            t.index_select(P["priv"], 0, idx, out=P["xp"])
            t.cat((x, P["xp"]), dim=1, out=P["xv"])
            xin["vf"] = P["xv"]
            if self.actor_priv_dim:
                xin["pi"] = P["xv"]
        for net in NETS:
            self._mlp_forward(P, net, "_" + net, xin[net])
        self._loss_head(P, s, st)
        for net, k, gy in (("pi", 12, P["g_pi"]), ("vf", 1, P["g_vf"])):
            self._mlp_backward(P, net, "_" + net, xin[net], gy, k, st)
        _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)

    def _loss_head(self, P, s, st):
        """orr_ppo_head or orr_ppo_head_logstd on the two nets' outputs: g_pi, g_vf, the output layers' bias gradients, stats[s]."""
        L, M, g, ws = self.L, P["M"], self.g, P["ws"].data_ptr()
        if self.logstd_head:
            log_std, g_log_std = (self.w[LOGSTD], g[LOGSTD]) if self.learn_std else (self.fixed_logstd, self.g_fixed_logstd)
            _lib.check(L.orr_ppo_head_logstd(P["y_pi"].data_ptr(), P["y_vf"].data_ptr(), P["batch"].data_ptr(), log_std.data_ptr(), M, self.clip,
                                             self.vf_coef, self.ent_coef, P["g_pi"].data_ptr(), P["g_vf"].data_ptr(), g_log_std.data_ptr(),
                                             g["model/pi/b:0"].data_ptr(), g["model/vf/b:0"].data_ptr(), P["stats"][s].data_ptr(), ws, st), L)
        else:
            _lib.check(L.orr_ppo_head(P["y_pi"].data_ptr(), P["y_vf"].data_ptr(), P["batch"].data_ptr(), M, float(self.model.std), self.clip,
                                      self.vf_coef, P["g_pi"].data_ptr(), P["g_vf"].data_ptr(), g["model/pi/b:0"].data_ptr(),
                                      g["model/vf/b:0"].data_ptr(), P["stats"][s].data_ptr(), ws, st), L)

    # ---- the learner interface (ppo.PPO.update) --------------------------------------------------------------------------
    def update(self, obs, actions, adv, ret, old_logp=None, epochs=1, generator=None, priv=None):
        """obs [B,160], actions [B,12] (unclipped samples), adv [B] (already normalised), ret [B] (TD(lambda) targets); priv [B,48]
        the privileged observations, for a model with a privileged critic;
        returns the mean (surrogate, value loss) over the minibatches like ppo.PPO.update; of a learn-std model the means of ppo.STAT_NAMES' five."""
        B = int(obs.shape[0])
        if (priv is not None) != (self.priv_dim > 0):
            raise ValueError("FusedPPO: priv is needed by a privileged critic and by no other")
        if priv is not None and tuple(priv.shape) != (B, self.priv_dim):
            raise ValueError("FusedPPO: priv must have shape (%d, %d)" % (B, self.priv_dim))

        def fill(P):
            logp = self.model.log_prob(obs, actions, *((priv,) if self.actor_priv_dim else ())) if old_logp is None else old_logp
            self._refresh_std()
            # a model with an observation normaliser: the static inputs hold (x - mean) * rstd (orr_normalize_rows instead of the copy),
            # so nothing inside the captured epoch changes; the statistics are the ones the rollout ran with
            norm, pnorm = getattr(self.model, "obs_norm", None), getattr(self.model, "priv_norm", None)
            if norm is not None:
                norm.normalize(obs.contiguous(), out=P["obs"])
            else:
                P["obs"].copy_(obs)
            if priv is not None:
                if pnorm is not None:
                    pnorm.normalize(priv.contiguous(), out=P["priv"])
                else:
                    P["priv"].copy_(priv)
            self._fill_aux(P, actions, logp, adv, ret)
        total, n = self._run(B, fill, epochs, generator, self._world(), self._allreduce if self._several() else None)
        return self._returned(total / n).cpu().numpy()

    def _fill_aux(self, P, actions, logp, adv, ret):
        """The loss head's per-sample row (ORR_PPO_BATCH_COLS): the actions, then old log-probability, advantage and return."""
        aux = P["aux"]
        aux[:, :12].copy_(actions)
        aux[:, 12].copy_(logp)
        aux[:, 13].copy_(adv)
        aux[:, 14].copy_(ret)

    # ---- ranks: the gradient all-reduce and replica consistency (MpiAdam, stable_baselines/common/mpi_adam.py) -----------------------
    def _world(self):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.group)

    def _several(self):
        """The several-ranks execution (per-minibatch graphs, all-reduce and Adam between replays): more than one rank, or
        ORR_FORCE_DIST=1 with a process group (one-rank rehearsal of exactly that path, e.g. on RCCL with the one GPU of a test box)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return False
        return dist.get_world_size(self.group) > 1 or (os.environ.get("ORR_FORCE_DIST", "0") == "1")

    def _allreduce(self, P=None, s=0):
        """Sum of the flat gradient over the ranks; orr_adam_step divides by the world size (mpi_adam.py:51-53).  Under a KL rule minibatch
        s's approx_kl becomes its mean over the ranks as well, in place in the plan's stats, before orr_update_control reads it: every replica
        then takes the same decision."""
        import torch.distributed as dist
        kl = P["stats"][s][3:4] if (self.kl_on and P is not None) else None
        if dist.get_backend(self.group) == "gloo":            # rehearsal of the multi-rank path on a one-GPU box: stage through the host
            for x in (self.flat_g,) + (() if kl is None else (kl,)):
                tmp = x.cpu()
                dist.all_reduce(tmp, group=self.group)
                x.copy_(tmp)
        else:
            dist.all_reduce(self.flat_g, group=self.group)   # RCCL, in place on the device
            if kl is not None:
                dist.all_reduce(kl, group=self.group)
        if kl is not None:
            kl /= dist.get_world_size(self.group)

    def _bcast_root(self):
        import torch.distributed as dist
        root = self.flat_p.clone()
        # `src` of a broadcast is a GLOBAL rank: the root of a subgroup is its own rank 0, whatever global rank that is
        src = 0 if self.group is None else dist.get_global_rank(self.group, 0)
        if dist.get_backend(self.group) == "gloo":
            host = root.cpu()
            dist.broadcast(host, src=src, group=self.group)
            root.copy_(host)
        else:
            dist.broadcast(root, src=src, group=self.group)
        return root

    def sync(self):
        """Every rank takes rank 0's parameters (mpi_adam.py:64-70; the reference calls it once before training)."""
        if self._several():
            with self.torch.no_grad():
                self.flat_p.copy_(self._bcast_root())
            self._mark_updated()

    def check_synced(self):
        """Raises unless this rank's parameters equal rank 0's bit for bit (mpi_adam.py:72-82; the reference checks every 100 steps)."""
        if self._several() and not bool(self.torch.equal(self._bcast_root(), self.flat_p)):
            raise RuntimeError("FusedPPO.check_synced: this rank's parameters differ from rank 0's")


class FusedPPOHistory(FusedPPO):
    """PPO on a history policy with an asymmetric critic, on the device (the torch reference is ppo.PPOHistory; RMA's third phase, or
    one-stage training with an auxiliary estimation loss): the actor reads obs | z, z = encode(hist), the critic obs | priv, the TRUE row.
      loss = FusedPPO's on those two inputs + latent_coef * mean_i sum_c (z_ic - priv_ic)^2
    Everything trains.  The flat buffer over all slots (model/enc_* among them), Adam, the log-std clamp, the all-reduce, sync and
    check_synced are FusedPPO's.  A minibatch: the gathers of obs, hist, priv and aux, the encoder's two GEMMs, the two 3-layer chains and
    the loss head as in FusedPPO, the critic's backward pass and then the actor's - which leaves d loss / d (the pre-activation of the
    actor's layer 0) in the shared scratch -, orr_policy_pack of W0_pi[160:]^T (inside the captured epoch, at a fixed address: the actor
    moves every step), orr_latent_backward from there to d loss / d z (+ the latent loss's own gradient, the column sums behind enc_fc1's
    bias gradient and the loss), the encoder's backward pass as in FusedDistillHistory, and two orr_colsum_finish: FusedPPO's jobs, then
    the encoder's (14 jobs for a split minibatch, ORR_COLSUM_MAX_JOBS is 12).  update() returns FusedPPO's stats followed by the latent
    loss; with latent_coef = 0 orr_latent_backward reads neither z nor priv, and the loss that is still reported costs an orr_regress_head."""

    _history = True

    def __init__(self, model, clip_param=0.2, lr=1e-5, adam_eps=1e-5, minibatch=4096, vf_coef=1.0, group=None, betas=(0.9, 0.999),
                 mpi_adam_epsilon=False, use_graph=True, ent_coef=0.0, log_std_bounds=None, latent_coef=0.0, max_grad_norm=None, device_lr=False,
                 kl_stop=None, kl_target=None, kl_lr_bounds=None):
        import math
        _no_obs_norm(model, "FusedPPOHistory")
        if not getattr(model, "history", 0):
            raise ValueError("FusedPPOHistory: the model needs a history encoder (ActorCritic(history=16)); a model without is trained by FusedPPO")
        self.latent_coef = float(latent_coef)
        if not (self.latent_coef >= 0.0 and math.isfinite(self.latent_coef)):
            raise ValueError("FusedPPOHistory: latent_coef must be finite and not negative")
        FusedPPO.__init__(self, model, clip_param, lr, adam_eps, minibatch, vf_coef, group, betas, mpi_adam_epsilon, use_graph, ent_coef, log_std_bounds,
                          max_grad_norm, device_lr, kl_stop, kl_target, kl_lr_bounds)

    def _graph_key(self):
        return FusedPPO._graph_key(self) + (self.latent_coef,)

    def _buffers(self, P, f, split, rows):
        FusedPPO._buffers(self, P, f, split, rows)           # obs, aux, priv and both nets at k0 = 160 + 48; xv = x | xp feeds the critic
        M, Z = P["M"], _abi.POLICY_PRIV_DIM
        lrows = _abi.latent_backward_rows(M)
        own = self._enc_buffers(P, f, split, rows)
        P.update({"hist": f(P["B"], _abi.HISTORY_DIM), "xz": f(M, 160 + Z), "lp": f(49 * lrows), "w0z": f(512, Z),
                  "w0zt": f(int(self.L.orr_policy_packed_size(512, Z)))})
        own.append((P["lp"], self.g["model/enc_fc1/b:0"], lrows, Z))
        lat = self.latent_coef != 0.0     # the latent loss then lands behind the head's stats, in the minibatch's own row: a table per minibatch
        P["jobs_s"] = [_jobs(own + ([(P["lp"][Z * lrows:], P["stats"][s][self.head_stats:], lrows, 1)] if lat else [])) for s in range(P["nmb"])]
        if not lat:                       # orr_latent_backward leaves no loss: orr_regress_head reports it
            P.update({"wsr": f(int(self.L.orr_learner_workspace_floats(M, 64))), "gr": f(M, Z), "gbr": f(Z)})

    def _minibatch(self, P, s):
        """Gather, forward, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M, w = self.torch, self.L, P["M"], self.w
        st = self._stream()
        Z = _abi.POLICY_PRIV_DIM
        idx = P["perm"][s * M:(s + 1) * M]
        for src, dst in (("obs", "x"), ("hist", "xh"), ("priv", "xp"), ("aux", "batch")):
            t.index_select(P[src], 0, idx, out=P[dst])
        self._enc_forward(P)
        t.cat((P["x"], P["z"]), dim=1, out=P["xz"])
        t.cat((P["x"], P["xp"]), dim=1, out=P["xv"])
        xin = {"pi": P["xz"], "vf": P["xv"]}
        for net in NETS:
            self._mlp_forward(P, net, "_" + net, xin[net])
        self._loss_head(P, s, st)
        # the critic first: the actor's pass then leaves ITS layer-0 gradient in the scratch the two share (gh1, masked by orr_relu_backward)
        for net, k, gy in (("vf", 1, P["g_vf"]), ("pi", 12, P["g_pi"])):
            self._mlp_backward(P, net, "_" + net, xin[net], gy, k, st)
        P["w0z"].copy_(w["model/pi_fc0/w:0"][160:].t())
        _lib.check(L.orr_policy_pack(P["w0z"].data_ptr(), 512, Z, P["w0zt"].data_ptr(), st), L)
        lat = self.latent_coef != 0.0
        _lib.check(L.orr_latent_backward(P["gh1"].data_ptr(), P["w0zt"].data_ptr(), P["z"].data_ptr() if lat else None,
                                         P["xp"].data_ptr() if lat else None, M, self.latent_coef, P["g_z"].data_ptr(), P["lp"].data_ptr(), st), L)
        if not lat:
            _lib.check(L.orr_regress_head(P["z"].data_ptr(), P["xp"].data_ptr(), M, Z, P["gr"].data_ptr(), P["gbr"].data_ptr(),
                                          P["stats"][s][self.head_stats:].data_ptr(), P["wsr"].data_ptr(), st), L)
        self._enc_backward(P, st)
        _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)
        _lib.check(L.orr_colsum_finish(*P["jobs_s"][s], st), L)

    def update(self, obs, hist, priv, actions, adv, ret, old_logp=None, epochs=1, generator=None):
        """obs [B,160], hist [B,512] (history_push), priv [B,48] (env.privileged_obs on the same states), actions [B,12] (unclipped samples),
        adv [B] (already normalised), ret [B] (TD(lambda) targets); returns FusedPPO's stats followed by the latent loss, like
        ppo.PPOHistory.update."""
        B = int(obs.shape[0])
        if tuple(hist.shape) != (B, _abi.HISTORY_DIM) or tuple(priv.shape) != (B, _abi.POLICY_PRIV_DIM):
            raise ValueError("FusedPPOHistory: hist must have shape (%d, %d) and priv (%d, %d)" % (B, _abi.HISTORY_DIM, B, _abi.POLICY_PRIV_DIM))

        def fill(P):
            logp = self.model.log_prob(obs, actions, hist=hist) if old_logp is None else old_logp
            self._refresh_std()
            P["obs"].copy_(obs)
            P["hist"].copy_(hist)
            P["priv"].copy_(priv)
            self._fill_aux(P, actions, logp, adv, ret)
        total, n = self._run(B, fill, epochs, generator, self._world(), self._allreduce if self._several() else None)
        return self._returned(total / n).cpu().numpy()


class FusedDistill(_FusedLearner):
    """Policy distillation on the device (the supervised step of DAgger; the torch reference is ppo.Distill): the student's mean is
    regressed on a teacher's, loss = mean over the samples of sum_j (mean_j - target_j)^2 (orr_distill_head).  The actor alone: only
    model/pi* move into the flat buffer and take Adam steps - the critic's parameters stay where and what they are, and have no moments
    here -, FusedPPO's chain for one net with orr_distill_head as the loss head: three forward GEMMs, the loss head, orr_head_backward,
    orr_relu_backward and one orr_colsum_finish per minibatch, equal minibatches in static buffers, an epoch captured once and replayed as
    one hipGraph (a single chain on one stream).  One rank: there is no gradient all-reduce here."""

    def __init__(self, student, lr=1e-4, minibatch=4096, adam_eps=1e-5, betas=(0.9, 0.999), use_graph=True, max_grad_norm=None, device_lr=False):
        _no_obs_norm(student, "FusedDistill")
        if getattr(student, "actor_priv_dim", 0):
            raise ValueError("FusedDistill: the student's actor must read the 160 observation words only")
        self._need_gpu(student)
        if getattr(student, "history", 0):
            raise ValueError("FusedDistill: a history student is trained by FusedDistillHistory, or with PPO by FusedPPOHistory")
        _FusedLearner.__init__(self, student, sorted(k for k in student.p if k.startswith("model/pi") and k != LOGSTD), 1, lr, adam_eps, minibatch, betas, use_graph,
                               max_grad_norm=max_grad_norm, device_lr=device_lr)

    def _buffers(self, P, f, split, rows):
        B, M = P["B"], P["M"]
        P.update({"obs": f(B, 160), "target": f(B, 12), "x": f(M, 160), "tgt": f(M, 12), "g_y": f(M, 12), "gz2": f(M, 256), "gh1": f(M, 512),
                  "ws": f(int(self.L.orr_learner_workspace_floats(M, 16)))})
        sums, parts = self._mlp_buffers(P, f, "pi", "", 160, 12, split, rows)
        P["jobs"], P["n_jobs"] = _jobs(sums + parts)

    def _minibatch(self, P, s):
        """Gather, the actor's forward pass, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M = self.torch, self.L, P["M"]
        st = self._stream()
        idx = P["perm"][s * M:(s + 1) * M]
        t.index_select(P["obs"], 0, idx, out=P["x"])
        t.index_select(P["target"], 0, idx, out=P["tgt"])
        self._mlp_forward(P, "pi", "", P["x"])
        _lib.check(L.orr_distill_head(P["y"].data_ptr(), P["tgt"].data_ptr(), M, P["g_y"].data_ptr(), self.g["model/pi/b:0"].data_ptr(),
                                      P["stats"][s].data_ptr(), P["ws"].data_ptr(), st), L)
        self._mlp_backward(P, "pi", "", P["x"], P["g_y"], 12, st)
        _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)

    def update(self, obs, target_mean, epochs=1, generator=None):
        """obs [B,160], target_mean [B,12] (the teacher's actor output on the same states); returns the mean loss over the minibatches,
        like ppo.Distill.update."""
        B = int(obs.shape[0])
        if tuple(target_mean.shape) != (B, 12):
            raise ValueError("FusedDistill: target_mean must have shape (%d, 12)" % B)

        def fill(P):
            P["obs"].copy_(obs)
            P["target"].copy_(target_mean)
        total, n = self._run(B, fill, epochs, generator)
        return float(total.item() / n)


class FusedDistillHistory(_FusedLearner):
    """The learner of a history student's encoder on the device (the torch reference is ppo.DistillHistory): encode(hist) is regressed on the
    recorded privileged rows, loss = mean over the samples of sum_j (z_j - priv_j)^2 (orr_regress_head).  The encoder alone: only
    model/enc_* move into the flat buffer and take Adam steps - the actor and the critic, the teacher's, stay where and what they are -,
    two forward GEMMs, the loss head, the two products behind it, orr_relu_backward at c = 256, the layer-0 weight gradient
    (split for minibatches of 4096 and more) and one orr_colsum_finish per minibatch; an epoch replays as one hipGraph.  One rank.

    action_coef > 0: loss = action_coef * mean_i sum_j (actor(obs, z)_ij - target_mean_ij)^2 + latent_coef * the loss above.  The loss head is then
    orr_history_student_head - the frozen actor's forward pass, both losses and the backward pass down to d loss / d z in one launch, against a
    packed copy of the actor and of the three transposes its backward pass streams (made once, and again when somebody else called the
    model's mark_updated()) -, everything behind it is the same.  The defaults (0, 1) are the path above, launch for launch."""

    def __init__(self, student, lr=1e-4, minibatch=4096, adam_eps=1e-5, betas=(0.9, 0.999), use_graph=True, action_coef=0.0, latent_coef=1.0,
                 max_grad_norm=None, device_lr=False):
        self.action_coef, self.latent_coef = float(action_coef), float(latent_coef)
        if self.action_coef < 0.0 or self.latent_coef < 0.0:
            raise ValueError("FusedDistillHistory: action_coef and latent_coef must not be negative")
        self.head = not (self.action_coef == 0.0 and self.latent_coef == 1.0)      # orr_history_student_head instead of orr_regress_head
        self.last_latent_loss = self.last_action_loss = None     # the means over the last update's minibatches
        self._actor, self._actor_seen = None, None
        _no_obs_norm(student, "FusedDistillHistory")
        self._need_gpu(student)
        if not getattr(student, "history", 0):
            raise ValueError("FusedDistillHistory: the student needs a history encoder (ActorCritic(history=16))")
        _FusedLearner.__init__(self, student, sorted(k for k in student.p if k.startswith("model/enc_")), 2 if self.head else 1, lr, adam_eps,
                               minibatch, betas, use_graph, max_grad_norm=max_grad_norm, device_lr=device_lr)

    def _graph_key(self):
        return _FusedLearner._graph_key(self) + (self.action_coef, self.latent_coef)

    def _pack_actor(self):
        """The frozen actor as orr_history_student_head reads it: its three matrices and the three transposes of the backward pass in
        orr_policy_pack's fragments, its biases as copies, all at fixed addresses (a captured epoch replays after a re-pack)."""
        t, L, p = self.torch, self.L, self.model.p
        Z = _abi.POLICY_PRIV_DIM
        w0, w1, w2 = (p["model/pi%s/w:0" % s].detach() for s in ("_fc0", "_fc1", ""))
        if tuple(w0.shape) != (160 + Z, 512) or tuple(w1.shape) != (512, 256) or tuple(w2.shape) != (256, 12):
            raise ValueError("FusedDistillHistory: the actor must be %d -> 512 -> 256 -> 12" % (160 + Z))
        w2t = t.zeros(16, 256, dtype=t.float32, device=self.dev)
        w2t[:12].copy_(w2.t())
        src = {"w0_pi": w0, "w1_pi": w1, "w2_pi": w2, "w2t": w2t, "w1t": w1.t(), "w0zt": w0[160:].t()}
        biases = (("b0_pi", "model/pi_fc0/b:0"), ("b1_pi", "model/pi_fc1/b:0"), ("b2_pi", "model/pi/b:0"))
        if self._actor is None:
            A = {"net": _abi.OrrPolicyNet()}                  # the vf members stay NULL: they are not read
            for name, w in src.items():
                A[name] = t.empty(int(L.orr_policy_packed_size(int(w.shape[0]), int(w.shape[1]))), dtype=t.float32, device=self.dev)
            for name, key in biases:
                A[name] = t.empty_like(p[key].detach(), dtype=t.float32, device=self.dev)
            for name in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi"):
                setattr(A["net"], name, A[name].data_ptr())
            self._actor = A
        A = self._actor
        for name, w in src.items():
            w = w.to(device=self.dev, dtype=t.float32).contiguous()
            _lib.check(L.orr_policy_pack(w.data_ptr(), int(w.shape[0]), int(w.shape[1]), A[name].data_ptr(), self._stream()), L)
        for name, key in biases:
            A[name].copy_(p[key].detach())

    def _buffers(self, P, f, split, rows):
        B, M, g, Z = P["B"], P["M"], self.g, _abi.POLICY_PRIV_DIM
        own = self._enc_buffers(P, f, split, rows)
        P.update({"hist": f(B, _abi.HISTORY_DIM), "target": f(B, Z), "tgt": f(M, Z), "ws": f(int(self.L.orr_learner_workspace_floats(M, 64)))})
        P["jobs"], P["n_jobs"] = _jobs(own)
        if self.head:
            # obs and the teacher's means, gathered with the same permutation; the head's partial sums (ORR_STUDENT_HEAD_PARTIAL_FLOATS) are two
            # more jobs of the minibatch's orr_colsum_finish: the bias gradient of enc_fc1 and the two losses, which land in the minibatch's own
            # row of stats - hence one job list per minibatch
            hrows = _abi.student_head_rows(M)
            P.update({"obs": f(B, 160), "tmean": f(B, 12), "xo": f(M, 160), "tm": f(M, 12), "hp": f(50 * hrows)})
            P["jobs_s"] = [_jobs(own + [(P["hp"], g["model/enc_fc1/b:0"], hrows, Z), (P["hp"][Z * hrows:], P["stats"][s], hrows, 2)])
                           for s in range(P["nmb"])]

    def _minibatch(self, P, s):
        """Gather, the encoder's forward pass, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M = self.torch, self.L, P["M"]
        st = self._stream()
        idx = P["perm"][s * M:(s + 1) * M]
        for src, dst in (("hist", "xh"), ("target", "tgt")) + ((("obs", "xo"), ("tmean", "tm")) if self.head else ()):
            t.index_select(P[src], 0, idx, out=P[dst])
        self._enc_forward(P)
        if self.head:
            A = self._actor
            _lib.check(L.orr_history_student_head(C.byref(A["net"]), A["w2t"].data_ptr(), A["w1t"].data_ptr(), A["w0zt"].data_ptr(), P["xo"].data_ptr(),
                                                  P["z"].data_ptr(), P["tm"].data_ptr(), P["tgt"].data_ptr(), M, self.action_coef, self.latent_coef,
                                                  P["g_z"].data_ptr(), None, P["hp"].data_ptr(), st), L)
        else:
            _lib.check(L.orr_regress_head(P["z"].data_ptr(), P["tgt"].data_ptr(), M, _abi.POLICY_PRIV_DIM, P["g_z"].data_ptr(),
                                          self.g["model/enc_fc1/b:0"].data_ptr(), P["stats"][s].data_ptr(), P["ws"].data_ptr(), st), L)
        self._enc_backward(P, st)
        _lib.check(L.orr_colsum_finish(*(P["jobs_s"][s] if self.head else (P["jobs"], P["n_jobs"])), st), L)

    def update(self, hist, target_priv, epochs=1, generator=None, obs=None, target_mean=None):
        """hist [B,512], target_priv [B,48] (env.privileged_obs on the same states); with action_coef > 0 also obs [B,160] and target_mean [B,12]
        (the teacher's actor output on the same states).  Returns the mean total loss over the minibatches, like ppo.DistillHistory.update."""
        B = int(hist.shape[0])
        if tuple(hist.shape) != (B, _abi.HISTORY_DIM) or tuple(target_priv.shape) != (B, _abi.POLICY_PRIV_DIM):
            raise ValueError("FusedDistillHistory: hist must have shape (B, %d) and target_priv (B, %d)" % (_abi.HISTORY_DIM, _abi.POLICY_PRIV_DIM))
        if self.action_coef > 0.0:
            if obs is None or target_mean is None:
                raise ValueError("FusedDistillHistory: action_coef > 0 needs obs and target_mean")
            if tuple(obs.shape) != (B, 160) or tuple(target_mean.shape) != (B, 12):
                raise ValueError("FusedDistillHistory: obs must have shape (%d, 160) and target_mean (%d, 12)" % (B, B))

        def fill(P):
            P["hist"].copy_(hist)
            P["target"].copy_(target_priv)
            if self.head:
                if self.action_coef > 0.0:
                    P["obs"].copy_(obs)
                    P["tmean"].copy_(target_mean)
                elif "cleared" not in P:                    # no action loss: its inputs are multiplied by zero, they only have to be finite
                    P["obs"].zero_()
                    P["tmean"].zero_()
                    P["cleared"] = True
                seen = getattr(self.model, "updates", None)
                if self._actor is None or seen is None or seen != self._actor_seen:
                    self._pack_actor()
        total, n = self._run(B, fill, epochs, generator)
        self._actor_seen = getattr(self.model, "updates", None)      # the encoder's steps are this learner's own: the packed actor stands
        total = [x / n for x in total.tolist()]
        if self.head:
            self.last_action_loss, self.last_latent_loss = total
            return self.action_coef * total[0] + self.latent_coef * total[1]
        self.last_action_loss, self.last_latent_loss = 0.0, total[0]
        return total[0]
