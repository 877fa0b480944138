"""Batched policy inference on the device (SURVEY.md section 8f item 1 -- the caller side of the hot path).

The reference evaluates the policy once per robot with batch size 1 through a TF1 session
(agents/imitation_runners.py:88-92).  Here one batched MLP serves all robots of a GPU:
  pi: 160 -> 512 -> 256 -> 12, ReLU (run.py:101-105), fixed-variance diagonal Gaussian with std 0.125
  (agents/imitation_policies.py:44-51,96-107), optional value head vf: 160 -> 512 -> 256 -> 1.
Weights load from a stable-baselines zip (`parameters` npz inside the zip, keys `model/pi_fc0/w:0` ...;
stable_baselines/common/base_class.py:552-590) or from an npz with the same keys.
This is plain torch (hipBLASLt GEMMs): a dense contraction, but nowhere near the env step in cost.
"""
import io
import math
import zipfile

import numpy as np

PI_STD = 0.125  # imitation_policies.py:106 pi_init_std
PRIV_DIM = 48   # width of the privileged observation a privileged critic reads next to the 160 observation words (ppo.ActorCritic(priv_dim=48); no reference counterpart)


def _norm_key(k):
    return k.replace("__", "/").replace("_0", ":0") if "__" in k else k


# the statistics of an observation normaliser (ppo.ActorCritic(obs_norm=True)): <prefix>/count (int64), /mean, /var, /eps; no reference counterpart
NORM_PREFIXES = ("obs_norm", "priv_norm")
NORM_FIELDS = (("count", np.int64), ("mean", np.float32), ("var", np.float32), ("eps", np.float32))


def _as_loaded(k, v):
    """float32, but a normaliser's row count as the integer it is (it passes 2^24 within a few hundred iterations)."""
    return v.astype(np.int64) if k.endswith("_norm/count") else v.astype(np.float32)


def load_parameters(path):
    """dict name -> float32 array from a stable-baselines zip or an npz (a normaliser's obs_norm/count: int64)."""
    if zipfile.is_zipfile(path):
        with zipfile.ZipFile(path) as z:
            names = z.namelist()
            if "parameters" in names:            # stable-baselines model zip
                params = np.load(io.BytesIO(z.read("parameters")))
                return {k: _as_loaded(k, params[k]) for k in params.files}
    params = np.load(path)
    return {_norm_key(k): _as_loaded(_norm_key(k), params[k]) for k in params.files}


# variables of the reference's ImitationPolicy graph in the order stable-baselines saves them (parameter_list of the shipped
# zips; tests/golden/policy_parameter_list.json).  `model/q/*` is the action-value head stable-baselines attaches to every
# feed-forward policy (common/policies.py proba_distribution_from_latent); PPO1 never trains or reads it, but
# BaseRLModel.load_parameters(exact_match=True) (common/base_class.py:437-500) refuses a zip without it.
SB_PARAMETER_LIST = (("model/pi_fc0/w:0", (160, 512)), ("model/pi_fc0/b:0", (512,)), ("model/vf_fc0/w:0", (160, 512)),
                     ("model/vf_fc0/b:0", (512,)), ("model/pi_fc1/w:0", (512, 256)), ("model/pi_fc1/b:0", (256,)),
                     ("model/vf_fc1/w:0", (512, 256)), ("model/vf_fc1/b:0", (256,)), ("model/vf/w:0", (256, 1)),
                     ("model/vf/b:0", (1,)), ("model/pi/w:0", (256, 12)), ("model/pi/b:0", (12,)), ("model/q/w:0", (256, 12)),
                     ("model/q/b:0", (12,)))


# a history student's encoder (ppo.ActorCritic(history=16)); no reference counterpart
ENC_PARAMETER_LIST = (("model/enc_fc0/w:0", (512, 256)), ("model/enc_fc0/b:0", (256,)), ("model/enc_fc1/w:0", (256, PRIV_DIM)),
                      ("model/enc_fc1/b:0", (PRIV_DIM,)))


# the learned log-std of ppo.ActorCritic(learn_std=True).  The reference's graph declares this very variable (pi/logstd, [1, 12], filled with
# log(pi_init_std): agents/imitation_policies.py:48) but with trainable=False, which keeps it out of the zips it saves and loads
LOGSTD = "model/pi/logstd:0"
LOGSTD_PARAMETER = (LOGSTD, (1, 12))


def save_parameters_zip(path, params, data=None):
    """Write weights in the stable-baselines zip layout (`data` JSON, `parameter_list` JSON, `parameters` npz;
    stable_baselines/common/base_class.py:552-590) so that the reference's `agent.load_parameters(model_file)`
    (run.py:220-221, exact_match=True) can read a policy trained here: the FULL variable set of the reference graph in its
    saved order.  The unused q head is carried over when `params` holds one (a policy warm-started from a reference zip) and
    zero-filled otherwise.  `data` carries no pickled objects (load_parameters ignores it).  Variables the reference's list does not
    have - a history encoder's, a learned log-std (model/pi/logstd:0) - follow its fourteen names; such a zip loads here, not in the reference."""
    import json
    out = {}
    for name, shape in SB_PARAMETER_LIST:
        if name in params:
            v = np.asarray(params[name], dtype=np.float32)
            if name == "model/vf_fc0/w:0" and v.shape == (shape[0] + PRIV_DIM, shape[1]):
                pass       # a privileged critic (ppo.ActorCritic(priv_dim=48)), written in full: the actor part is what the reference can load
            elif name == "model/pi_fc0/w:0" and v.shape == (shape[0] + PRIV_DIM, shape[1]):
                pass       # a privileged actor (ppo.ActorCritic(actor_priv_dim=48)): a teacher, loadable here only; its distilled student is plain
            elif v.shape != shape:
                raise ValueError("%s has shape %s, the reference graph expects %s" % (name, v.shape, shape))
        elif name.startswith("model/q/"):
            v = np.zeros(shape, dtype=np.float32)
        else:
            raise ValueError("missing variable %s" % name)
        out[name] = v
    names = [n for n, _ in SB_PARAMETER_LIST]
    for name, shape in ENC_PARAMETER_LIST:       # a history student (ppo.ActorCritic(history=16)): behind the reference's list, loadable here only
        if ENC_PARAMETER_LIST[0][0] in params:
            v = np.asarray(params[name], dtype=np.float32)
            if v.shape != shape:
                raise ValueError("%s has shape %s, a history encoder has %s" % (name, v.shape, shape))
            out[name] = v
            names.append(name)
    name, shape = LOGSTD_PARAMETER               # a learned log-std (ppo.ActorCritic(learn_std=True)): likewise behind the list, loadable here only -
    if name in params:                           # the reference's exact_match load refuses a zip with a fifteenth name
        v = np.asarray(params[name], dtype=np.float32)
        if v.shape != shape:
            raise ValueError("%s has shape %s, a learned log-std has %s" % (name, v.shape, shape))
        out[name] = v
        names.append(name)
    for prefix in NORM_PREFIXES:                 # an observation normaliser's statistics (ppo.ActorCritic(obs_norm=True)): likewise behind the list.
        if prefix + "/count" in params:          # The nets of such a zip expect normalised inputs: the reference must not load it as a plain policy,
            for field, dtype in NORM_FIELDS:     # and with these names in the list its exact_match load refuses it (save_folded writes one it can run)
                if "%s/%s" % (prefix, field) in params:
                    out["%s/%s" % (prefix, field)] = np.asarray(params["%s/%s" % (prefix, field)], dtype=dtype)
                    names.append("%s/%s" % (prefix, field))
    buf = io.BytesIO()
    np.savez(buf, **out)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(data or {}))
        z.writestr("parameter_list", json.dumps(names))
        z.writestr("parameters", buf.getvalue())


NORM_EPS = 1e-2       # ppo.NORM_EPS: what a zip without <prefix>/eps was normalised with


def fold_norm(params):
    """The parameters of a model with an observation normaliser (its state_dict(): obs_norm/*, priv_norm/*) as those of the SAME function
    on raw inputs, without statistics: ((x - mean) * rstd) W + b = x (diag(rstd) W) + (b - (mean * rstd) W) for both layer 0s.
    rstd = 1 / (sqrt(var) + eps) as the record forms it (float64 on the float32 var, rounded once); the matrix is the float32 product
    rstd_i * W_ij (what orr_policy_pack_norm packs), the bias is summed in float64 and rounded once.  Rows 160.. of a 208-row matrix take
    priv_norm's statistics.  A dict without statistics comes back as a copy."""
    out = {k: np.asarray(v) for k, v in params.items() if not k.startswith(tuple(p + "/" for p in NORM_PREFIXES))}
    if "obs_norm/count" not in params:
        return out
    tab = {}
    for prefix in NORM_PREFIXES:
        if prefix + "/count" in params:
            var = np.asarray(params[prefix + "/var"], dtype=np.float32)
            eps = np.float32(np.asarray(params.get(prefix + "/eps", NORM_EPS)).reshape(-1)[0])
            tab[prefix] = (np.asarray(params[prefix + "/mean"], dtype=np.float32),
                           (1.0 / (np.sqrt(var.astype(np.float64)) + np.float64(eps))).astype(np.float32))
    for net in ("pi", "vf"):
        w = np.asarray(params["model/%s_fc0/w:0" % net], dtype=np.float32)
        b = np.asarray(params["model/%s_fc0/b:0" % net], dtype=np.float32)
        mean, rstd = tab["obs_norm"]
        if w.shape[0] > mean.shape[0]:
            if "priv_norm" not in tab:
                raise ValueError("model/%s_fc0/w:0 has %d rows and the dict no priv_norm/*" % (net, w.shape[0]))
            mean, rstd = np.concatenate((mean, tab["priv_norm"][0])), np.concatenate((rstd, tab["priv_norm"][1]))
        if w.shape[0] != mean.shape[0]:
            raise ValueError("model/%s_fc0/w:0 has %d rows, the statistics %d columns" % (net, w.shape[0], mean.shape[0]))
        out["model/%s_fc0/w:0" % net] = rstd[:, None] * w
        out["model/%s_fc0/b:0" % net] = (b.astype(np.float64) - (mean * rstd).astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
    return out


def save_folded(path, params, data=None):
    """save_parameters_zip of fold_norm(params): a zip with no statistics whose layer-0 matrices and biases carry the normaliser.  For a
    model without privileged rows that is a plain 160 -> 512 -> 256 -> 12 policy: MLPPolicy.from_file and the reference's run.py load it
    and run it on raw observations."""
    save_parameters_zip(path, fold_norm(params), data)


class MLPPolicy(object):
    def __init__(self, params, device, std=PI_STD):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.std = float(std)
        if "obs_norm/count" in params:           # a zip with a normaliser's statistics: the same function on raw observations
            params = fold_norm(params)
        g = lambda k: torch.tensor(params[k], dtype=torch.float32, device=self.device)
        self.pi = [(g("model/pi_fc0/w:0"), g("model/pi_fc0/b:0")), (g("model/pi_fc1/w:0"), g("model/pi_fc1/b:0")),
                   (g("model/pi/w:0"), g("model/pi/b:0"))]
        # a zip saved from a learn-std model: sample with its twelve stds instead of `std`
        self.log_std = g(LOGSTD).reshape(1, 12) if LOGSTD in params else None
        self.learn_std = self.log_std is not None      # as ppo.ActorCritic says it: whoever forms a log-probability asks this one attribute
        self.vf = None
        if "model/vf_fc0/w:0" in params:
            self.vf = [(g("model/vf_fc0/w:0"), g("model/vf_fc0/b:0")), (g("model/vf_fc1/w:0"), g("model/vf_fc1/b:0")),
                       (g("model/vf/w:0"), g("model/vf/b:0"))]

    @classmethod
    def from_file(cls, path, device, std=PI_STD):
        return cls(load_parameters(path), device, std)

    def _mlp(self, layers, x):
        t = self.torch
        h = t.relu(t.addmm(layers[0][1], x, layers[0][0]))
        h = t.relu(t.addmm(layers[1][1], h, layers[1][0]))
        return t.addmm(layers[2][1], h, layers[2][0])

    def mean(self, obs):
        return self._mlp(self.pi, obs)

    def value(self, obs):
        if self.vf is None:
            return self.torch.zeros(obs.shape[0], device=obs.device)
        return self._mlp(self.vf, obs)[:, 0]

    def act(self, obs, deterministic=False, generator=None):
        """-> (clipped action [N,12] for env.step, unclipped action, value [N]).  Clip = action space +-2 pi
        (imitation_runners.py:140-143)."""
        t = self.torch
        mu = self.mean(obs)
        std = self.std if self.log_std is None else self.log_std.exp()
        a = mu if deterministic else mu + std * t.randn(mu.shape, device=mu.device, generator=generator)
        return t.clamp(a, -2.0 * math.pi, 2.0 * math.pi), a, self.value(obs)

    def log_prob(self, obs, actions):
        t = self.torch
        mu = self.mean(obs)
        if self.log_std is not None:
            z = (actions - mu) * t.exp(-self.log_std)
            return (-0.5 * z * z - self.log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
        var = self.std * self.std
        return (-0.5 * ((actions - mu) ** 2) / var - 0.5 * math.log(2.0 * math.pi * var)).sum(dim=1)
