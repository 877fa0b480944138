"""The PPO update with its non-GEMM part in hand-written HIP and the whole epoch replayed as one hipGraph
(include/openroborl_learner.h, csrc/orr_learner.hip).

Same arithmetic as ppo.PPO.update (the plain PyTorch restatement of agents/ppo_imitation.py:156-258 + Adam, which stays the
fp32 reference the tests compare this against), different execution:
  * parameters, gradients and Adam moments live in ONE flat buffer each (the model's tensors become views of it): the gradient
    all-reduce needs no packing and Adam is one launch over 434 k floats;
  * forward = six GEMMs with bias(+ReLU) epilogues writing into static activations; backward = ten GEMMs written out by hand
    (no autograd graph) with the ReLU masks, the gradient through the two output layers (fan-out 12 and 1: no GEMM), every bias
    gradient and the loss head in a handful of HIP launches (7 per minibatch) - autograd spends ~70 elementwise / reduction launches per
    minibatch on the same work, more GPU time than the GEMMs;
  * one rank: an epoch (gathers of all minibatches, forward, backward, Adam) is captured once and replayed - ~30 launches per
    minibatch cost no host time; several ranks: one graph per minibatch, the all-reduce (RCCL) and Adam between replays.
    ORR_FORCE_DIST=1 with an initialised process group takes the several-ranks path even for ONE rank (a one-GPU box can then run
    per-minibatch graphs + the RCCL all-reduce + Adam between replays; the result equals the one-graph path bit for bit).
Scalar hyper-parameters (lr, betas, eps, clip, vf_coef, the policy's std, the world size) are by-value kernel arguments, i.e. frozen
into a captured graph: update() compares them with the values the graphs were captured with and captures again when one changed
(the reference feeds optim_stepsize * cur_lrmult every step: ppo1/pposgd_simple.py; run.py uses schedule='constant').
There is no fallback: without a GPU and the HIP library the constructor raises.
"""
import ctypes as C
import os

from . import _abi, _lib

NETS = ("pi", "vf")


class FusedPPO(object):
    _takes_history = False        # a history student (ppo.ActorCritic(history=16)) is trained by FusedDistillHistory only

    def __init__(self, model, clip_param=0.2, lr=1e-5, adam_eps=1e-5, minibatch=4096, vf_coef=1.0, group=None, betas=(0.9, 0.999),
                 mpi_adam_epsilon=False, use_graph=True):
        import torch
        self.torch = torch
        self.model = model
        self.dev = model.device
        if self.dev.type != "cuda":
            raise RuntimeError("FusedPPO needs a GPU device (the torch reference is ppo.PPO)")
        if bool(getattr(model, "history", 0)) != self._takes_history:
            raise ValueError("%s: %s" % (type(self).__name__, "the student needs a history encoder (ActorCritic(history=16))" if self._takes_history
                                         else "a history student is trained by FusedDistillHistory only"))
        self.L = _lib.load()
        self.clip, self.lr, self.eps, self.vf_coef = float(clip_param), float(lr), float(adam_eps), float(vf_coef)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        self.minibatch = int(minibatch)
        self.group = group
        self.adam_flags = 1 if mpi_adam_epsilon else 0          # ORR_ADAM_MPI_EPSILON
        self.use_graph = bool(use_graph)
        # a privileged critic (ppo.ActorCritic(priv_dim=48)): its layer 0 reads x | priv, [M, 160 + 48]; everything behind layer 0 and the
        # whole actor are what they are without (the kernels of orr_learner.hip see hidden and output layers only)
        self.priv_dim = int(getattr(model, "priv_dim", 0))
        # a privileged actor as well (ppo.ActorCritic(actor_priv_dim=48), a teacher): its layer 0 reads the same x | priv
        self.actor_priv_dim = int(getattr(model, "actor_priv_dim", 0))
        # ---- one flat buffer for the parameters (16-byte aligned slots), the model's tensors become views of it ----
        names = self._trained(model)
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
        if hasattr(model, "mark_updated"):
            model.mark_updated()
        self._plans = {}

    @staticmethod
    def _trained(model):
        """Names of the parameters this learner owns: they move into its flat buffer and take its Adam steps."""
        return sorted(model.p)

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

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

    def _graph_key(self, several):
        return (self.lr, self.b1, self.b2, self.eps, self.clip, self.vf_coef, float(self.model.std), self.adam_flags, self._world(), several)

    @staticmethod
    def fit_minibatch(num_samples, minibatch):
        """Largest minibatch size <= `minibatch` that divides `num_samples` (update() needs equal minibatches: static buffers)."""
        m = max(1, min(int(minibatch), int(num_samples)))
        while num_samples % m:
            m -= 1
        return m

    def _adam(self, world):
        _lib.check(self.L.orr_adam_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.total,
                                        self.lr, self.b1, self.b2, self.eps, 1.0 / world, self.adam_flags, self.state.data_ptr(),
                                        self._stream()), self.L)

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
        if key in self._plans:
            return self._plans[key]
        t = self.torch
        f = lambda *shape: t.empty(shape, dtype=t.float32, device=self.dev)   # noqa: E731
        split = M >= 4096 and M % 16 == 0
        pd = self.priv_dim
        P = {"B": B, "M": M, "nmb": B // M, "obs": f(B, 160), "aux": f(B, 16), "perm": t.empty(B, dtype=t.int64, device=self.dev),
             "x": f(M, 160), "batch": f(M, 16), "gz2": f(M, 256), "gh1": f(M, 512), "g_pi": f(M, 12), "g_vf": f(M),
             "stats": t.zeros(B // M, 2, dtype=t.float32, device=self.dev),
             "ws": f(int(self.L.orr_learner_workspace_floats(M, 16))), "graphs": None}
        P["aux"].zero_()
        if pd:      # the privileged observations, gathered with the same permutation; xv = x | xp is the critic's layer-0 input
            P["priv"], P["xp"], P["xv"] = f(B, pd), f(M, pd), f(M, 160 + pd)
        # the column sums behind the six bias gradients and the two output-layer weight gradients of a minibatch are deferred: each
        # producer leaves its per-workgroup partial sums in its own buffer and ONE launch adds them all up (orr_colsum_finish)
        rows = int(self.L.orr_learner_partial_rows(M))
        jobs = (_abi.OrrColsumJob * 10)()
        for i, (net, k) in enumerate((("pi", 12), ("vf", 1))):
            P["h1_" + net], P["h2_" + net], P["y_" + net] = f(M, 512), f(M, 256), f(M, k)
            k0 = 160 + (pd if net == "vf" else self.actor_priv_dim)          # rows of the net's layer-0 weight
            P["part1_" + net], P["part0_" + net] = (f(16, 512, 256), f(16, k0, 512)) if split else (None, None)
            if split:
                jobs[6 + 2 * i] = _abi.OrrColsumJob(P["part1_" + net].data_ptr(), self.g["model/%s_fc1/w:0" % net].data_ptr(), 16, 512 * 256)
                jobs[7 + 2 * i] = _abi.OrrColsumJob(P["part0_" + net].data_ptr(), self.g["model/%s_fc0/w:0" % net].data_ptr(), 16, k0 * 512)
            P["ws2_" + net] = f(int(self.L.orr_learner_workspace_floats(M, 256)))      # [rows][256] | [rows][256 * 12]
            P["ws1_" + net] = f(rows * 512)
            for j, (buf, off, out, cols) in enumerate(((P["ws2_" + net], 0, self.g["model/%s_fc1/b:0" % net], 256),
                                                       (P["ws2_" + net], rows * 256, self.g["model/%s/w:0" % net], 256 * k),
                                                       (P["ws1_" + net], 0, self.g["model/%s_fc0/b:0" % net], 512))):
                jobs[3 * i + j] = _abi.OrrColsumJob(buf.data_ptr() + 4 * off, out.data_ptr(), rows, cols)
        P["jobs"], P["n_jobs"] = jobs, 10 if split else 6
        self._plans[key] = P
        return P

    def _minibatch(self, P, s):
        """Gather, forward, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M, w, g = self.torch, self.L, P["M"], self.w, self.g
        st, ws = self._stream(), P["ws"].data_ptr()
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
            t._addmm_activation(w["model/%s_fc0/b:0" % net], xin[net], w["model/%s_fc0/w:0" % net], out=P["h1_" + net])
            t._addmm_activation(w["model/%s_fc1/b:0" % net], P["h1_" + net], w["model/%s_fc1/w:0" % net], out=P["h2_" + net])
            t.addmm(w["model/%s/b:0" % net], P["h2_" + net], w["model/%s/w:0" % net], out=P["y_" + net])
        _lib.check(L.orr_ppo_head(P["y_pi"].data_ptr(), P["y_vf"].data_ptr(), P["batch"].data_ptr(), M, float(self.model.std), self.clip,
                                  self.vf_coef, P["g_pi"].data_ptr(), P["g_vf"].data_ptr(), g["model/pi/b:0"].data_ptr(),
                                  g["model/vf/b:0"].data_ptr(), P["stats"][s].data_ptr(), ws, st), L)
        for net, k, gy in (("pi", 12, P["g_pi"]), ("vf", 1, P["g_vf"])):
            h1, h2 = P["h1_" + net], P["h2_" + net]
            _lib.check(L.orr_head_backward(gy.data_ptr(), k, w["model/%s/w:0" % net].data_ptr(), h2.data_ptr(), M, 256, P["gz2"].data_ptr(),
                                           None, None, P["ws2_" + net].data_ptr(), st), L)
            self._wgrad(h1, P["gz2"], P["part1_" + net], g["model/%s_fc1/w:0" % net])
            t.mm(P["gz2"], w["model/%s_fc1/w:0" % net].t(), out=P["gh1"])
            _lib.check(L.orr_relu_backward(P["gh1"].data_ptr(), h1.data_ptr(), M, 512, None, P["ws1_" + net].data_ptr(), st), L)
            self._wgrad(xin[net], P["gh1"], P["part0_" + net], g["model/%s_fc0/w:0" % net])
        _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)

    def _allreduce(self):
        """Sum of the flat gradient over the ranks; orr_adam_step divides by the world size (mpi_adam.py:51-53)."""
        import torch.distributed as dist
        if dist.get_backend(self.group) == "gloo":            # rehearsal of the multi-rank path on a one-GPU box: stage through the host
            tmp = self.flat_g.cpu()
            dist.all_reduce(tmp, group=self.group)
            self.flat_g.copy_(tmp)
        else:
            dist.all_reduce(self.flat_g, group=self.group)   # RCCL, in place on the device

    def _epoch_eager(self, P, world, several):
        for s in range(P["nmb"]):
            self._minibatch(P, s)
            if several:
                self._allreduce()
            self._adam(world)

    def _capture(self, P, several):
        """One rank: one graph for the whole epoch.  Several ranks: one graph per minibatch (the collective runs between replays)."""
        t = self.torch
        keep = [x.clone() for x in (self.flat_p, self.m, self.v, self.state)]
        P["perm"].copy_(t.arange(P["B"], device=self.dev))
        side = t.cuda.Stream(device=self.dev)
        side.wait_stream(t.cuda.current_stream(self.dev))
        with t.cuda.stream(side):                    # warm-up outside the capture: library handles, workspaces, kernel selection
            for _ in range(2):
                self._minibatch(P, 0)
                self._adam(1)
        t.cuda.current_stream(self.dev).wait_stream(side)
        graphs = []
        if not several:
            gr = t.cuda.CUDAGraph()
            with t.cuda.graph(gr):
                for s in range(P["nmb"]):
                    self._minibatch(P, s)
                    self._adam(1)
            graphs.append(gr)
        else:
            pool = None
            for s in range(P["nmb"]):
                gr = t.cuda.CUDAGraph()
                with t.cuda.graph(gr, pool=pool):
                    self._minibatch(P, s)
                pool = pool or gr.pool()
                graphs.append(gr)
        for dst, src in zip((self.flat_p, self.m, self.v, self.state), keep):     # the warm-up took real optimiser steps: undo them
            dst.copy_(src)
        P["graphs"] = graphs

    # ---- the learner interface (ppo.PPO.update) --------------------------------------------------------------------------
    def update(self, obs, actions, adv, ret, old_logp=None, epochs=1, generator=None, priv=None):
        """obs [B,160], actions [B,12] (unclipped samples), adv [B] (already normalised), ret [B] (TD(lambda) targets); priv [B,48]
        the privileged observations, for a model with a privileged critic;
        returns the mean (surrogate, value loss) over the minibatches like ppo.PPO.update."""
        t = self.torch
        B = int(obs.shape[0])
        if (priv is not None) != (self.priv_dim > 0):
            raise ValueError("FusedPPO: priv is needed by a privileged critic and by no other")
        if priv is not None and tuple(priv.shape) != (B, self.priv_dim):
            raise ValueError("FusedPPO: priv must have shape (%d, %d)" % (B, self.priv_dim))
        M = min(self.minibatch, B)
        if B % M:
            raise ValueError("FusedPPO: the number of samples (%d) must be a multiple of the minibatch size (%d); "
                             "FusedPPO.fit_minibatch(%d, %d) = %d is the largest size that divides it" % (B, M, B, M, self.fit_minibatch(B, M)))
        world, several = self._world(), self._several()
        with t.no_grad():
            if old_logp is None:
                old_logp = self.model.log_prob(obs, actions, *((priv,) if self.actor_priv_dim else ()))
            P = self._plan(B, M)
            P["obs"].copy_(obs)
            if priv is not None:
                P["priv"].copy_(priv)
            aux = P["aux"]
            aux[:, :12].copy_(actions)
            aux[:, 12].copy_(old_logp)
            aux[:, 13].copy_(adv)
            aux[:, 14].copy_(ret)
            if self.use_graph and (P["graphs"] is None or P.get("graph_key") != self._graph_key(several)):
                self._capture(P, several)
                P["graph_key"] = self._graph_key(several)
            total = t.zeros(2, dtype=t.float32, device=self.dev)
            for _ in range(epochs):
                P["perm"].copy_(t.randperm(B, device=self.dev, generator=generator))
                if not self.use_graph:
                    self._epoch_eager(P, world, several)
                elif not several:
                    P["graphs"][0].replay()
                else:
                    for gr in P["graphs"]:
                        gr.replay()
                        self._allreduce()
                        self._adam(world)
                total += P["stats"].sum(dim=0)
        if hasattr(self.model, "mark_updated"):
            self.model.mark_updated()
        return (total / float(epochs * P["nmb"])).cpu().numpy()

    def steps_taken(self):
        return int(self.state[0].item())

    # ---- replica consistency (MpiAdam.sync / check_synced, stable_baselines/common/mpi_adam.py:64-82) -----------------------
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
            if hasattr(self.model, "mark_updated"):
                self.model.mark_updated()

    def check_synced(self):
        """Raises unless this rank's parameters equal rank 0's bit for bit (mpi_adam.py:72-82; the reference checks every 100 steps)."""
        if self._several() and not bool(self.torch.equal(self._bcast_root(), self.flat_p)):
            raise RuntimeError("FusedPPO.check_synced: this rank's parameters differ from rank 0's")


class FusedDistill(FusedPPO):
    """Policy distillation on the device (the supervised step of DAgger; the torch reference is ppo.Distill): the student's mean is
    regressed on a teacher's, loss = mean over the samples of sum_j (mean_j - target_j)^2 (orr_distill_head).  FusedPPO's machinery with
    the actor alone: only model/pi* move into the flat buffer and take Adam steps - the critic's parameters stay where and what they are,
    and have no moments here -, three forward GEMMs, the loss head, orr_head_backward, orr_relu_backward and one orr_colsum_finish per
    minibatch, equal minibatches in static buffers, an epoch captured once and replayed as one hipGraph (a single chain on one stream).
    One rank: there is no gradient all-reduce here."""

    def __init__(self, student, lr=1e-4, minibatch=4096, adam_eps=1e-5, betas=(0.9, 0.999), use_graph=True):
        if getattr(student, "actor_priv_dim", 0):
            raise ValueError("FusedDistill: the student's actor must read the 160 observation words only")
        FusedPPO.__init__(self, student, lr=lr, adam_eps=adam_eps, minibatch=minibatch, betas=betas, use_graph=use_graph)

    @staticmethod
    def _trained(model):
        return sorted(k for k in model.p if k.startswith("model/pi"))

    def _graph_key(self, several):
        return (self.lr, self.b1, self.b2, self.eps, self.adam_flags)

    def _plan(self, B, M):
        key = (B, M)
        if key in self._plans:
            return self._plans[key]
        t = self.torch
        f = lambda *shape: t.empty(shape, dtype=t.float32, device=self.dev)   # noqa: E731
        split = M >= 4096 and M % 16 == 0
        rows = int(self.L.orr_learner_partial_rows(M))
        P = {"B": B, "M": M, "nmb": B // M, "obs": f(B, 160), "target": f(B, 12), "perm": t.empty(B, dtype=t.int64, device=self.dev),
             "x": f(M, 160), "tgt": f(M, 12), "h1": f(M, 512), "h2": f(M, 256), "y": f(M, 12), "g_y": f(M, 12), "gz2": f(M, 256), "gh1": f(M, 512),
             "stats": t.zeros(B // M, 1, dtype=t.float32, device=self.dev), "ws": f(int(self.L.orr_learner_workspace_floats(M, 16))),
             "ws2": f(int(self.L.orr_learner_workspace_floats(M, 256))), "ws1": f(rows * 512),
             "part1": f(16, 512, 256) if split else None, "part0": f(16, 160, 512) if split else None, "graphs": None}
        g = self.g
        jobs = (_abi.OrrColsumJob * 5)()
        jobs[0] = _abi.OrrColsumJob(P["ws2"].data_ptr(), g["model/pi_fc1/b:0"].data_ptr(), rows, 256)
        jobs[1] = _abi.OrrColsumJob(P["ws2"].data_ptr() + 4 * rows * 256, g["model/pi/w:0"].data_ptr(), rows, 256 * 12)
        jobs[2] = _abi.OrrColsumJob(P["ws1"].data_ptr(), g["model/pi_fc0/b:0"].data_ptr(), rows, 512)
        if split:
            jobs[3] = _abi.OrrColsumJob(P["part1"].data_ptr(), g["model/pi_fc1/w:0"].data_ptr(), 16, 512 * 256)
            jobs[4] = _abi.OrrColsumJob(P["part0"].data_ptr(), g["model/pi_fc0/w:0"].data_ptr(), 16, 160 * 512)
        P["jobs"], P["n_jobs"] = jobs, 5 if split else 3
        self._plans[key] = P
        return P

    def _minibatch(self, P, s):
        """Gather, the actor's forward pass, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M, w, g = self.torch, self.L, P["M"], self.w, self.g
        st = self._stream()
        idx = P["perm"][s * M:(s + 1) * M]
        t.index_select(P["obs"], 0, idx, out=P["x"])
        t.index_select(P["target"], 0, idx, out=P["tgt"])
        t._addmm_activation(w["model/pi_fc0/b:0"], P["x"], w["model/pi_fc0/w:0"], out=P["h1"])
        t._addmm_activation(w["model/pi_fc1/b:0"], P["h1"], w["model/pi_fc1/w:0"], out=P["h2"])
        t.addmm(w["model/pi/b:0"], P["h2"], w["model/pi/w:0"], out=P["y"])
        _lib.check(L.orr_distill_head(P["y"].data_ptr(), P["tgt"].data_ptr(), M, P["g_y"].data_ptr(), g["model/pi/b:0"].data_ptr(),
                                      P["stats"][s].data_ptr(), P["ws"].data_ptr(), st), L)
        _lib.check(L.orr_head_backward(P["g_y"].data_ptr(), 12, w["model/pi/w:0"].data_ptr(), P["h2"].data_ptr(), M, 256, P["gz2"].data_ptr(),
                                       None, None, P["ws2"].data_ptr(), st), L)
        self._wgrad(P["h1"], P["gz2"], P["part1"], g["model/pi_fc1/w:0"])
        t.mm(P["gz2"], w["model/pi_fc1/w:0"].t(), out=P["gh1"])
        _lib.check(L.orr_relu_backward(P["gh1"].data_ptr(), P["h1"].data_ptr(), M, 512, None, P["ws1"].data_ptr(), st), L)
        self._wgrad(P["x"], P["gh1"], P["part0"], g["model/pi_fc0/w:0"])
        _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)

    def update(self, obs, target_mean, epochs=1, generator=None):
        """obs [B,160], target_mean [B,12] (the teacher's actor output on the same states); returns the mean loss over the minibatches,
        like ppo.Distill.update."""
        t = self.torch
        B = int(obs.shape[0])
        if tuple(target_mean.shape) != (B, 12):
            raise ValueError("FusedDistill: target_mean must have shape (%d, 12)" % B)
        M = min(self.minibatch, B)
        if B % M:
            raise ValueError("FusedDistill: the number of samples (%d) must be a multiple of the minibatch size (%d); "
                             "FusedPPO.fit_minibatch(%d, %d) = %d is the largest size that divides it" % (B, M, B, M, self.fit_minibatch(B, M)))
        with t.no_grad():
            P = self._plan(B, M)
            P["obs"].copy_(obs)
            P["target"].copy_(target_mean)
            if self.use_graph and (P["graphs"] is None or P.get("graph_key") != self._graph_key(False)):
                self._capture(P, False)
                P["graph_key"] = self._graph_key(False)
            total = t.zeros(1, dtype=t.float32, device=self.dev)
            for _ in range(epochs):
                P["perm"].copy_(t.randperm(B, device=self.dev, generator=generator))
                if self.use_graph:
                    P["graphs"][0].replay()
                else:
                    self._epoch_eager(P, 1, False)
                total += P["stats"].sum(dim=0)
        if hasattr(self.model, "mark_updated"):
            self.model.mark_updated()
        return float(total.item() / float(epochs * P["nmb"]))

    def sync(self):
        pass

    def check_synced(self):
        pass


class FusedDistillHistory(FusedDistill):
    """The learner of a history student's encoder on the device (the torch reference is ppo.DistillHistory): encode(hist) is regressed on the
    recorded privileged rows, loss = mean over the samples of sum_j (z_j - priv_j)^2 (orr_regress_head).  FusedDistill's machinery with the
    encoder alone: only model/enc_* move into the flat buffer and take Adam steps - the actor and the critic, the teacher's, stay where and what
    they are -, two forward GEMMs, the loss head, the two products behind it, orr_relu_backward at c = 256, the layer-0 weight gradient
    (split for minibatches of 4096 and more) and one orr_colsum_finish per minibatch; an epoch replays as one hipGraph.  One rank.

    action_coef > 0: loss = action_coef * mean_i sum_j (actor(obs, z)_ij - target_mean_ij)^2 + latent_coef * the loss above.  The loss head is then
    orr_history_student_head - the frozen actor's forward pass, both losses and the backward pass down to d loss / d z in one launch, against a
    packed copy of the actor and of the three transposes its backward pass streams (made once, and again when somebody else called the
    model's mark_updated()) -, everything behind it is the same.  The defaults (0, 1) are the path above, launch for launch."""
    _takes_history = True

    def __init__(self, student, lr=1e-4, minibatch=4096, adam_eps=1e-5, betas=(0.9, 0.999), use_graph=True, action_coef=0.0, latent_coef=1.0):
        self.action_coef, self.latent_coef = float(action_coef), float(latent_coef)
        if self.action_coef < 0.0 or self.latent_coef < 0.0:
            raise ValueError("FusedDistillHistory: action_coef and latent_coef must not be negative")
        self.head = not (self.action_coef == 0.0 and self.latent_coef == 1.0)      # orr_history_student_head instead of orr_regress_head
        self.last_latent_loss = self.last_action_loss = None     # the means over the last update's minibatches
        self._actor, self._actor_seen = None, None
        FusedPPO.__init__(self, student, lr=lr, adam_eps=adam_eps, minibatch=minibatch, betas=betas, use_graph=use_graph)

    @staticmethod
    def _trained(model):
        return sorted(k for k in model.p if k.startswith("model/enc_"))

    def _graph_key(self, several):
        return FusedDistill._graph_key(self, several) + (self.action_coef, self.latent_coef)

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
        if self._actor is None:
            A = {"net": _abi.OrrPolicyNet()}                  # the vf members stay NULL: they are not read
            for name, w in src.items():
                A[name] = t.empty(int(L.orr_policy_packed_size(int(w.shape[0]), int(w.shape[1]))), dtype=t.float32, device=self.dev)
            for name, key in (("b0_pi", "model/pi_fc0/b:0"), ("b1_pi", "model/pi_fc1/b:0"), ("b2_pi", "model/pi/b:0")):
                A[name] = t.empty_like(p[key].detach(), dtype=t.float32, device=self.dev)
            for name in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi"):
                setattr(A["net"], name, A[name].data_ptr())
            self._actor = A
        A = self._actor
        for name, w in src.items():
            w = w.to(device=self.dev, dtype=t.float32).contiguous()
            _lib.check(L.orr_policy_pack(w.data_ptr(), int(w.shape[0]), int(w.shape[1]), A[name].data_ptr(), self._stream()), L)
        for name, key in (("b0_pi", "model/pi_fc0/b:0"), ("b1_pi", "model/pi_fc1/b:0"), ("b2_pi", "model/pi/b:0")):
            A[name].copy_(p[key].detach())

    def _plan(self, B, M):
        key = (B, M)
        if key in self._plans:
            return self._plans[key]
        t = self.torch
        f = lambda *shape: t.empty(shape, dtype=t.float32, device=self.dev)   # noqa: E731
        split = M >= 4096 and M % 16 == 0
        rows = int(self.L.orr_learner_partial_rows(M))
        D, H, Z = _abi.HISTORY_DIM, 256, _abi.POLICY_PRIV_DIM
        P = {"B": B, "M": M, "nmb": B // M, "hist": f(B, D), "target": f(B, Z), "perm": t.empty(B, dtype=t.int64, device=self.dev),
             "x": f(M, D), "tgt": f(M, Z), "h": f(M, H), "z": f(M, Z), "g_z": f(M, Z), "g_h": f(M, H),
             "stats": t.zeros(B // M, 2 if self.head else 1, dtype=t.float32, device=self.dev), "ws": f(int(self.L.orr_learner_workspace_floats(M, 64))),
             "ws1": f(rows * H), "part0": f(16, D, H) if split else None, "graphs": None}
        jobs = (_abi.OrrColsumJob * 2)()
        jobs[0] = _abi.OrrColsumJob(P["ws1"].data_ptr(), self.g["model/enc_fc0/b:0"].data_ptr(), rows, H)
        if split:
            jobs[1] = _abi.OrrColsumJob(P["part0"].data_ptr(), self.g["model/enc_fc0/w:0"].data_ptr(), 16, D * H)
        P["jobs"], P["n_jobs"] = jobs, 2 if split else 1
        if self.head:
            # obs and the teacher's means, gathered with the same permutation; the head's partial sums (ORR_STUDENT_HEAD_PARTIAL_FLOATS) are two
            # more jobs of the minibatch's orr_colsum_finish: the bias gradient of enc_fc1 and the two losses, which land in the minibatch's own
            # row of stats - hence one job list per minibatch
            hrows = _abi.student_head_rows(M)
            P.update({"obs": f(B, 160), "tmean": f(B, 12), "xo": f(M, 160), "tm": f(M, 12), "hp": f(50 * hrows)})
            P["jobs_s"] = []
            for s in range(P["nmb"]):
                js = (_abi.OrrColsumJob * 4)()
                for j in range(P["n_jobs"]):
                    js[j] = jobs[j]
                js[P["n_jobs"]] = _abi.OrrColsumJob(P["hp"].data_ptr(), self.g["model/enc_fc1/b:0"].data_ptr(), hrows, Z)
                js[P["n_jobs"] + 1] = _abi.OrrColsumJob(P["hp"].data_ptr() + 4 * Z * hrows, P["stats"][s].data_ptr(), hrows, 2)
                P["jobs_s"].append(js)
        self._plans[key] = P
        return P

    def _minibatch(self, P, s):
        """Gather, the encoder's forward pass, loss head and backward of minibatch s of the current permutation; gradients land in flat_g."""
        t, L, M, w, g = self.torch, self.L, P["M"], self.w, self.g
        st = self._stream()
        idx = P["perm"][s * M:(s + 1) * M]
        t.index_select(P["hist"], 0, idx, out=P["x"])
        t.index_select(P["target"], 0, idx, out=P["tgt"])
        if self.head:
            t.index_select(P["obs"], 0, idx, out=P["xo"])
            t.index_select(P["tmean"], 0, idx, out=P["tm"])
        t._addmm_activation(w["model/enc_fc0/b:0"], P["x"], w["model/enc_fc0/w:0"], out=P["h"])
        t.addmm(w["model/enc_fc1/b:0"], P["h"], w["model/enc_fc1/w:0"], out=P["z"])
        if self.head:
            A = self._actor
            _lib.check(L.orr_history_student_head(C.byref(A["net"]), A["w2t"].data_ptr(), A["w1t"].data_ptr(), A["w0zt"].data_ptr(), P["xo"].data_ptr(),
                                                  P["z"].data_ptr(), P["tm"].data_ptr(), P["tgt"].data_ptr(), M, self.action_coef, self.latent_coef,
                                                  P["g_z"].data_ptr(), None, P["hp"].data_ptr(), st), L)
        else:
            _lib.check(L.orr_regress_head(P["z"].data_ptr(), P["tgt"].data_ptr(), M, _abi.POLICY_PRIV_DIM, P["g_z"].data_ptr(),
                                          g["model/enc_fc1/b:0"].data_ptr(), P["stats"][s].data_ptr(), P["ws"].data_ptr(), st), L)
        t.mm(P["h"].t(), P["g_z"], out=g["model/enc_fc1/w:0"])
        t.mm(P["g_z"], w["model/enc_fc1/w:0"].t(), out=P["g_h"])
        _lib.check(L.orr_relu_backward(P["g_h"].data_ptr(), P["h"].data_ptr(), M, 256, None, P["ws1"].data_ptr(), st), L)
        self._wgrad(P["x"], P["g_h"], P["part0"], g["model/enc_fc0/w:0"])
        if self.head:
            _lib.check(L.orr_colsum_finish(P["jobs_s"][s], P["n_jobs"] + 2, st), L)
        else:
            _lib.check(L.orr_colsum_finish(P["jobs"], P["n_jobs"], st), L)

    def update(self, hist, target_priv, epochs=1, generator=None, obs=None, target_mean=None):
        """hist [B,512], target_priv [B,48] (env.privileged_obs on the same states); with action_coef > 0 also obs [B,160] and target_mean [B,12]
        (the teacher's actor output on the same states).  Returns the mean total loss over the minibatches, like ppo.DistillHistory.update."""
        t = self.torch
        B = int(hist.shape[0])
        if tuple(hist.shape) != (B, _abi.HISTORY_DIM) or tuple(target_priv.shape) != (B, _abi.POLICY_PRIV_DIM):
            raise ValueError("FusedDistillHistory: hist must have shape (B, %d) and target_priv (B, %d)" % (_abi.HISTORY_DIM, _abi.POLICY_PRIV_DIM))
        if self.action_coef > 0.0:
            if obs is None or target_mean is None:
                raise ValueError("FusedDistillHistory: action_coef > 0 needs obs and target_mean")
            if tuple(obs.shape) != (B, 160) or tuple(target_mean.shape) != (B, 12):
                raise ValueError("FusedDistillHistory: obs must have shape (%d, 160) and target_mean (%d, 12)" % (B, B))
        M = min(self.minibatch, B)
        if B % M:
            raise ValueError("FusedDistillHistory: the number of samples (%d) must be a multiple of the minibatch size (%d); "
                             "FusedPPO.fit_minibatch(%d, %d) = %d is the largest size that divides it" % (B, M, B, M, self.fit_minibatch(B, M)))
        with t.no_grad():
            P = self._plan(B, M)
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
            if self.use_graph and (P["graphs"] is None or P.get("graph_key") != self._graph_key(False)):
                self._capture(P, False)
                P["graph_key"] = self._graph_key(False)
            total = t.zeros(P["stats"].shape[1], dtype=t.float32, device=self.dev)
            for _ in range(epochs):
                P["perm"].copy_(t.randperm(B, device=self.dev, generator=generator))
                if self.use_graph:
                    P["graphs"][0].replay()
                else:
                    self._epoch_eager(P, 1, False)
                total += P["stats"].sum(dim=0)
        if hasattr(self.model, "mark_updated"):
            self.model.mark_updated()
        self._actor_seen = getattr(self.model, "updates", None)      # the encoder's steps are this learner's own: the packed actor stands
        total = [x / float(epochs * P["nmb"]) for x in total.tolist()]
        if self.head:
            self.last_action_loss, self.last_latent_loss = total
            return self.action_coef * total[0] + self.latent_coef * total[1]
        self.last_action_loss, self.last_latent_loss = 0.0, total[0]
        return total[0]
