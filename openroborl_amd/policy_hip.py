"""Fused actor / critic forward pass on the matrix cores (include/openroborl_policy.h, csrc/orr_policy.hip).

One launch per env step instead of the reference's one TF session call per robot (agents/imitation_runners.py:88-92)
and instead of ~15 torch kernels for the two 160 -> 512 -> 256 -> {12, 1} MLPs.  f32 in, f32 accumulate.
There is no fallback here: without the HIP library the constructor raises.
"""
import ctypes as C
import math

from . import _abi, _lib
from .policy import LOGSTD     # a learned log-std [1, 12] (ppo.ActorCritic(learn_std=True)): sampled with when the parameter dict holds it

KEYS = (("w0_pi", "model/pi_fc0/w:0"), ("b0_pi", "model/pi_fc0/b:0"), ("w1_pi", "model/pi_fc1/w:0"), ("b1_pi", "model/pi_fc1/b:0"),
        ("w2_pi", "model/pi/w:0"), ("b2_pi", "model/pi/b:0"), ("w0_vf", "model/vf_fc0/w:0"), ("b0_vf", "model/vf_fc0/b:0"),
        ("w1_vf", "model/vf_fc1/w:0"), ("b1_vf", "model/vf_fc1/b:0"), ("w2_vf", "model/vf/w:0"), ("b2_vf", "model/vf/b:0"))
# a history student's encoder (orr_policy_forward_history), packed when the parameter dict holds it
ENC_KEYS = (("w0", "model/enc_fc0/w:0"), ("b0", "model/enc_fc0/b:0"), ("w1", "model/enc_fc1/w:0"), ("b1", "model/enc_fc1/b:0"))
ENC_SHAPES = {"w0": (_abi.HISTORY_DIM, 256), "w1": (256, _abi.POLICY_PRIV_DIM)}
SHAPES = {"w0_pi": (160, 512), "w0_vf": (160, 512), "w1_pi": (512, 256), "w1_vf": (512, 256), "w2_pi": (256, 12), "w2_vf": (256, 1)}


class FusedActorCritic(object):
    """Device-resident packed copy of an actor-critic parameter dict (stable-baselines names, torch tensors on the GPU).
    Call `refresh()` after the parameters changed (e.g. after an optimiser step) and `forward()` once per env step.

    A dict with model/pi/logstd:0 samples with it instead of `std`: forward() first scales the noise by exp(log_std) (orr_gauss_prepare, into a
    static buffer) and then runs the forward kernel it would run anyway with std = 1, mean + 1 * x being mean + x.  The twelve values are
    read on the device, from this object's own copy at a fixed address (refresh() renews it), never on the host."""

    def __init__(self, params, device, std, clip=2.0 * math.pi, obs_norm=None, priv_norm=None):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FusedActorCritic needs a GPU device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.load()
        self.params = params
        self.std = float(std)
        self.clip = float(clip)
        self.packed = {}
        self.biases = {}
        self.priv_dim = 0             # 48 when model/vf_fc0/w:0 has 160 + 48 rows: forward() then takes `priv` and runs orr_policy_forward_priv
        self.actor_priv_dim = 0       # 48 when model/pi_fc0/w:0 has 160 + 48 rows as well (a teacher): orr_policy_forward_teacher
        for field, key in KEYS:
            w = params[key]
            if field.startswith("w"):
                k, n = SHAPES[field]
                if field == "w0_pi" and tuple(w.shape) == (k + _abi.POLICY_PRIV_DIM, n):
                    k += _abi.POLICY_PRIV_DIM     # a privileged actor: its layer 0 reads obs | priv too (orr_policy_forward_teacher)
                    self.actor_priv_dim = _abi.POLICY_PRIV_DIM
                if field == "w0_vf" and tuple(w.shape) == (k + _abi.POLICY_PRIV_DIM, n):
                    k += _abi.POLICY_PRIV_DIM     # a privileged critic: its layer 0 reads obs | priv (orr_policy_forward_priv)
                    self.priv_dim = _abi.POLICY_PRIV_DIM
                if tuple(w.shape) != (k, n):
                    raise ValueError("%s has shape %s, the fused kernel is built for %s" % (key, tuple(w.shape), (k, n)))
                size = int(self.L.orr_policy_packed_size(k, n))
                self.packed[field] = torch.empty(size, dtype=torch.float32, device=self.device)
        if self.actor_priv_dim and not self.priv_dim:
            raise ValueError("a privileged actor (model/pi_fc0/w:0 with %d rows) needs a privileged critic" % (160 + _abi.POLICY_PRIV_DIM))
        self.history = 0              # 16 when the dict holds model/enc_fc0/w:0 (a history student): forward() takes `hist` in priv's place
        self.enc = _abi.OrrHistoryEncoder()
        if ENC_KEYS[0][1] in params:
            if not self.actor_priv_dim:
                raise ValueError("a history encoder (model/enc_fc0/w:0) feeds a privileged actor (model/pi_fc0/w:0 with %d rows)" % (160 + _abi.POLICY_PRIV_DIM))
            self.history = _abi.HISTORY_STEPS
            for field, key in ENC_KEYS:
                if field in ENC_SHAPES:
                    if tuple(params[key].shape) != ENC_SHAPES[field]:
                        raise ValueError("%s has shape %s, the fused kernel is built for %s" % (key, tuple(params[key].shape), ENC_SHAPES[field]))
                    self.packed["enc_" + field] = torch.empty(int(self.L.orr_policy_packed_size(*ENC_SHAPES[field])), dtype=torch.float32, device=self.device)
        self.log_std = None           # the sampler's copy of model/pi/logstd:0, [12]
        self._scaled = {}             # n -> the static [n, 12] buffer of exp(log_std) * noise
        if LOGSTD in params:
            if params[LOGSTD].numel() != 12:
                raise ValueError("%s has shape %s, the sampler is built for (1, 12)" % (LOGSTD, tuple(params[LOGSTD].shape)))
            self.log_std = torch.empty(12, dtype=torch.float32, device=self.device)
        # an observation normaliser (ppo.RunningNorm over the 160 words; priv_norm over the 48 of the privileged row): folded into the two
        # layer-0 images and biases by refresh(), so forward() launches what it launches without.  The statistics are read on the device, from
        # the records' fixed addresses (a captured refresh() follows them); a 208-row matrix reads a table of its own, obs | priv
        self.obs_norm, self.priv_norm = obs_norm, priv_norm
        self._norm_tab = None
        if obs_norm is not None:
            if self.history:
                raise ValueError("an observation normaliser with a history encoder is not built")
            def here(norm):     # the record's device against this object's, both resolved (a tensor on "cuda" reports cuda:<current>)
                d = norm.rec.device
                return d.type == self.device.type and (torch.cuda.current_device() if d.index is None else d.index) == self.device.index
            if obs_norm.dim != 160 or not here(obs_norm) or (priv_norm is not None and (priv_norm.dim != _abi.POLICY_PRIV_DIM or not here(priv_norm))):
                raise ValueError("obs_norm must be a RunningNorm(160) and priv_norm a RunningNorm(%d) on %s" % (_abi.POLICY_PRIV_DIM, self.device))
            if self.priv_dim:
                k = 160 + _abi.POLICY_PRIV_DIM
                self._norm_tab = (torch.zeros(k, dtype=torch.float32, device=self.device), torch.ones(k, dtype=torch.float32, device=self.device))
        elif priv_norm is not None:
            raise ValueError("priv_norm goes with obs_norm")
        self.net = _abi.OrrPolicyNet()
        self.refresh()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def refresh(self):
        """Re-pack the weights (six small launches, eight with an encoder) and re-read the biases from the parameter tensors.  With an
        observation normaliser the two layer-0 matrices go through orr_policy_pack_norm, which also writes their folded biases."""
        t = self.torch
        if self.log_std is not None:
            self.log_std.copy_(self.params[LOGSTD].detach().reshape(12))
        if self._norm_tab is not None:         # the table of a 208-row layer 0: the observation's statistics, then the row's (or 0, 1 as built)
            for tab, name in zip(self._norm_tab, ("mean", "rstd")):
                tab[:160].copy_(getattr(self.obs_norm, name))
                if self.priv_norm is not None:
                    tab[160:].copy_(getattr(self.priv_norm, name))
        for struct, prefix, keys in ((self.net, "", KEYS),) + (((self.enc, "enc_", ENC_KEYS),) if self.history else ()):
            done = set()                       # biases the folded pack has written
            for field, key in keys:
                w = self.params[key].detach()
                if w.dtype != t.float32 or not w.is_contiguous() or w.device != self.device:
                    w = w.to(device=self.device, dtype=t.float32).contiguous()
                name = prefix + field
                if self.obs_norm is not None and name in ("w0_pi", "w0_vf"):
                    # layer 0 behind the normaliser: the packed image of diag(rstd) W and the folded bias, straight into the bias copy
                    k, n = w.shape
                    b = self.params[dict(keys)["b0" + field[2:]]].detach()
                    if b.dtype != t.float32 or not b.is_contiguous() or b.device != self.device:
                        b = b.to(device=self.device, dtype=t.float32).contiguous()
                    bname = "b0" + field[2:]
                    if bname not in self.biases:
                        self.biases[bname] = t.empty_like(b)
                    mean, rstd = (self.obs_norm.mean, self.obs_norm.rstd) if int(k) == 160 else self._norm_tab
                    _lib.check(self.L.orr_policy_pack_norm(w.data_ptr(), int(k), int(n), mean.data_ptr(), rstd.data_ptr(), b.data_ptr(),
                                                           self.packed[name].data_ptr(), self.biases[bname].data_ptr(), self._stream()), self.L)
                    setattr(struct, field, self.packed[name].data_ptr())
                    setattr(struct, bname, self.biases[bname].data_ptr())
                    done.add(bname)
                elif name in done:
                    pass
                elif field.startswith("w"):
                    k, n = w.shape
                    _lib.check(self.L.orr_policy_pack(w.data_ptr(), int(k), int(n), self.packed[name].data_ptr(), self._stream()), self.L)
                    setattr(struct, field, self.packed[name].data_ptr())
                else:
                    if name not in self.biases:          # own copy (stays valid while the optimiser updates the original) at a fixed address,
                        self.biases[name] = t.empty_like(w)   # so that a captured forward pass can be replayed after a refresh
                    self.biases[name].copy_(w)
                    setattr(struct, field, self.biases[name].data_ptr())

    def prepare(self, noise, scaled, logp=None):
        """orr_gauss_prepare with this policy's log-std: scaled [n,12] = exp(log_std) * noise [n,12] and, when given, logp [n] = the
        log-probability of mean + scaled under the sampling policy.  One launch for any n (a whole rollout segment); scaled may be noise."""
        t = self.torch
        if self.log_std is None:
            raise ValueError("prepare() is for a policy with %s" % LOGSTD)
        n = noise.shape[0]
        for x, shape in ((noise, (n, 12)), (scaled, (n, 12)), (logp, (n,))):
            if x is not None and (x.dtype != t.float32 or not x.is_contiguous() or tuple(x.shape) != shape or x.device != self.device):
                raise ValueError("noise and scaled must be contiguous float32 [n,12] tensors and logp [n] on %s" % (self.device,))
        _lib.check(self.L.orr_gauss_prepare(noise.data_ptr(), self.log_std.data_ptr(), scaled.data_ptr(), logp.data_ptr() if logp is not None else None,
                                            int(n), self._stream()), self.L)
        return scaled

    def forward(self, obs, noise=None, want_mean=False, out_action=None, out_raw=None, out_value=None, priv=None, out_mean=None, want_value=True,
                hist=None, out_latent=None, scaled=False, critic_priv=None):
        """obs [N,160] float32 on the device; noise [N,12] standard normal or None (deterministic); priv [N,48] float32, the
        privileged observation, for a privileged critic (and only then).
        Returns (clipped action [N,12], raw action [N,12], value [N], mean [N,12] or None); the out_* tensors
        (contiguous float32 of those shapes, e.g. rows of a rollout buffer) are written in place when given (out_mean implies want_mean).
        want_value=False: no value is written and None is returned for it; a privileged actor's kernel then skips the critic.
        hist [N,512] float32 (history_push), for a history student and instead of priv: the encoder's estimate of the row feeds actor and
        critic (orr_policy_forward_history) and is written to out_latent [N,48] when that is given.
        critic_priv [N,48] float32, with hist only: the critic reads obs | critic_priv, the TRUE row, while the actor reads the estimate
        (orr_policy_forward_history_priv: the actor's outputs are orr_policy_forward_history's, the value orr_policy_forward_teacher's).
        scaled=True, for a policy with a learned log-std: `noise` already is exp(log_std) * noise (prepare(), e.g. once for a whole segment)."""
        t = self.torch
        if obs.dtype != t.float32 or not obs.is_contiguous() or obs.device != self.device or obs.dim() != 2 or obs.shape[1] != 160:
            raise ValueError("obs must be a contiguous float32 [N,160] tensor on %s" % (self.device,))
        n = obs.shape[0]
        if hist is not None:
            if priv is not None:
                raise ValueError("give priv or hist, not both")
            if not self.history:
                raise ValueError("hist is for a history student (model/enc_fc0/w:0) and for no other")
            if hist.dtype != t.float32 or not hist.is_contiguous() or tuple(hist.shape) != (n, _abi.HISTORY_DIM) or hist.device != self.device:
                raise ValueError("hist must be a contiguous float32 [N,%d] tensor on the same device" % _abi.HISTORY_DIM)
            if critic_priv is not None and (critic_priv.dtype != t.float32 or not critic_priv.is_contiguous() or critic_priv.device != self.device
                                            or tuple(critic_priv.shape) != (n, _abi.POLICY_PRIV_DIM)):
                raise ValueError("critic_priv must be a contiguous float32 [N,%d] tensor on the same device" % _abi.POLICY_PRIV_DIM)
        elif critic_priv is not None:
            raise ValueError("critic_priv goes with hist: the actor reads the encoder's estimate, the critic the true row")
        elif out_latent is not None:
            raise ValueError("out_latent belongs to hist")
        elif (priv is not None) != (self.priv_dim > 0):
            raise ValueError("priv is needed by a privileged critic (model/vf_fc0/w:0 with %d rows) and by no other" % (160 + _abi.POLICY_PRIV_DIM))
        if priv is not None and (priv.dtype != t.float32 or not priv.is_contiguous() or tuple(priv.shape) != (n, self.priv_dim)
                                 or priv.device != self.device):
            raise ValueError("priv must be a contiguous float32 [N,%d] tensor on the same device" % self.priv_dim)
        if noise is not None and (noise.dtype != t.float32 or not noise.is_contiguous() or tuple(noise.shape) != (n, 12)
                                  or noise.device != self.device):
            raise ValueError("noise must be a contiguous float32 [N,12] tensor on the same device")
        def out(x, shape):
            if x is None:
                return t.empty(shape, dtype=t.float32, device=self.device)
            if x.dtype != t.float32 or not x.is_contiguous() or tuple(x.shape) != shape or x.device != self.device:
                raise ValueError("output tensor must be contiguous float32 %s on %s" % (shape, self.device))
            return x
        if not want_value and out_value is not None:
            raise ValueError("out_value given with want_value=False")
        act, raw, val = out(out_action, (n, 12)), out(out_raw, (n, 12)), out(out_value, (n,)) if want_value else None
        mean = out(out_mean, (n, 12)) if (want_mean or out_mean is not None) else None
        std = self.std
        if self.log_std is not None:
            if noise is not None and not scaled:
                if n not in self._scaled:
                    self._scaled[n] = t.empty((n, 12), dtype=t.float32, device=self.device)
                noise = self.prepare(noise, self._scaled[n])
            std = 1.0
        elif scaled:
            raise ValueError("scaled=True is for a policy with %s" % LOGSTD)
        if hist is not None:
            latent = out(out_latent, (n, _abi.POLICY_PRIV_DIM)) if out_latent is not None else None
            if critic_priv is not None:
                _lib.check(self.L.orr_policy_forward_history_priv(C.byref(self.net), C.byref(self.enc), obs.data_ptr(), hist.data_ptr(),
                                                                  critic_priv.data_ptr(), int(n), noise.data_ptr() if noise is not None else None,
                                                                  std, self.clip, act.data_ptr(), raw.data_ptr(),
                                                                  val.data_ptr() if val is not None else None,
                                                                  mean.data_ptr() if mean is not None else None,
                                                                  latent.data_ptr() if latent is not None else None, self._stream()), self.L)
                return act, raw, val, mean
            _lib.check(self.L.orr_policy_forward_history(C.byref(self.net), C.byref(self.enc), obs.data_ptr(), hist.data_ptr(), int(n),
                                                         noise.data_ptr() if noise is not None else None, std, self.clip, act.data_ptr(),
                                                         raw.data_ptr(), val.data_ptr() if val is not None else None,
                                                         mean.data_ptr() if mean is not None else None,
                                                         latent.data_ptr() if latent is not None else None, self._stream()), self.L)
            return act, raw, val, mean
        if self.actor_priv_dim:
            _lib.check(self.L.orr_policy_forward_teacher(C.byref(self.net), obs.data_ptr(), priv.data_ptr(), int(n),
                                                         noise.data_ptr() if noise is not None else None, std, self.clip, act.data_ptr(),
                                                         raw.data_ptr(), val.data_ptr() if val is not None else None,
                                                         mean.data_ptr() if mean is not None else None, self._stream()), self.L)
            return act, raw, val, mean
        if priv is not None:
            _lib.check(self.L.orr_policy_forward_priv(C.byref(self.net), obs.data_ptr(), priv.data_ptr(), int(n),
                                                      noise.data_ptr() if noise is not None else None, std, self.clip, act.data_ptr(),
                                                      raw.data_ptr(), val.data_ptr() if val is not None else None, mean.data_ptr() if mean is not None else None,
                                                      self._stream()), self.L)
            return act, raw, val, mean
        _lib.check(self.L.orr_policy_forward(C.byref(self.net), obs.data_ptr(), int(n), noise.data_ptr() if noise is not None else None,
                                             std, self.clip, act.data_ptr(), raw.data_ptr(), val.data_ptr() if val is not None else None,
                                             mean.data_ptr() if mean is not None else None, self._stream()), self.L)
        return act, raw, val, mean


def history_push(obs, done, prev, out):
    """orr_history_push: out [N,512] = the sensor history after the step that produced obs [N,160] and done [N] (uint8 / bool; None: everybody
    starts an episode, prev may then be None too), prev [N,512] the one before it.  out may be prev (in place).  Returns out."""
    import torch
    n = obs.shape[0]
    for x, shape, name in ((obs, (n, 160), "obs"), (prev, (n, _abi.HISTORY_DIM), "prev"), (out, (n, _abi.HISTORY_DIM), "out")):
        if x is not None and (x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != shape or x.device != obs.device or not x.is_cuda):
            raise ValueError("%s must be a contiguous float32 %s tensor on the GPU" % (name, shape))
    if out is None or (done is not None and prev is None):
        raise ValueError("history_push needs out, and prev with done")
    if done is not None:
        if done.dtype == torch.bool:
            done = done.view(torch.uint8)
        if done.dtype != torch.uint8 or not done.is_contiguous() or tuple(done.shape) != (n,) or done.device != obs.device:
            raise ValueError("done must be a contiguous uint8 / bool [N] tensor on the same device")
    L = _lib.load()
    _lib.check(L.orr_history_push(obs.data_ptr(), done.data_ptr() if done is not None else None, prev.data_ptr() if prev is not None else None,
                                  out.data_ptr(), int(n), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)), L)
    return out
