"""The running observation normaliser (ppo.ActorCritic(obs_norm=True)): RunningNorm, one record of statistics on the device or the host, and
how a parameter dict carries them.  ppo re-exports every name."""
import math

import numpy as np

from . import policy as pol

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
