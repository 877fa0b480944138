"""The recurrent student on the bf16 matrix cores (csrc/orr_recurrent_bf16.hip) against STEP-WISE float64 references on the kernel's own float32
operands, rounded to bf16 in numpy with integer arithmetic: a whole-sequence reference would put elements across rounding boundaries.
Figures measured on an MI355X are in profiles/gru_bf16.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_recurrent import (CASES, F, G, H, SENTINEL, Z, _forward, _frame, _guarded, _inputs, _pads_untouched, _raw_args, _segment, _student,
                                      _weights)

pytestmark = pytest.mark.gpu

KEYS = ("model/gru_x/w:0", "model/gru_x/b:0", "model/gru_h/w:0", "model/gru_h/b:0", "model/gru_out/w:0", "model/gru_out/b:0")


def _rne(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _w(dtype):
    """wx, bx, wh, bh, wo, bo: the float32 weights the device holds, the matrices rounded to bf16."""
    f32 = [_weights()[k].astype(np.float32) for k in KEYS]
    return [(_rne(a) if a.ndim == 2 else a).astype(dtype) for a in f32]


def _step(x, hp, dtype):
    """One step from the float32 frame x and float32 h': rounded operands into the contractions, the unrounded h' into the combine."""
    wx, bx, wh, bh, _, _ = _w(dtype)
    sig = lambda a: 1 / (1 + np.exp(-a))   # noqa: E731
    gx, gh = _rne(x).astype(dtype) @ wx, _rne(hp).astype(dtype) @ wh
    r, u = sig((gx[:, :H] + gh[:, :H] + bx[:H]) + bh[:H]), sig((gx[:, H:2 * H] + gh[:, H:2 * H] + bx[H:2 * H]) + bh[H:2 * H])
    q = gh[:, 2 * H:] + bh[2 * H:]
    c = np.tanh((gx[:, 2 * H:] + bx[2 * H:]) + r * q)
    return (1 - u) * c + u * hp.astype(dtype), np.stack((r, u, c, q), axis=1)


def _latent(hid, dtype):
    _, _, _, _, wo, bo = _w(dtype)
    return _rne(hid).astype(dtype) @ wo + bo


def _bptt(saved, hprev, starts, g_latent, g_h, dtype):
    """g_x, g_h of every step, dh carried in `dtype`.  g_h: the float32 rows whose rounded values go into dh_{t-1} (the kernel's own; None: this
    function's, as float32)."""
    wht, wot = _w(dtype)[2].T, _w(dtype)[4].T
    T = len(starts)
    out_x, out_h = [None] * T, [None] * T
    dh = _rne(g_latent[T - 1]).astype(dtype) @ wot
    for t in range(T - 1, -1, -1):
        r, u, c, q = (saved[t][:, k].astype(dtype) for k in range(4))
        du, dc = dh * (hprev[t].astype(dtype) - c), dh * (1 - u)
        dcp, dup = dc * (1 - c * c), du * u * (1 - u)
        drp, gc = dcp * q * r * (1 - r), r * dcp
        out_x[t], out_h[t] = np.concatenate((drp, dup, dcp), axis=1), np.concatenate((drp, dup, gc), axis=1)
        if t > 0:
            carried = u * dh + _rne(out_h[t].astype(np.float32) if g_h is None else g_h[t]).astype(dtype) @ wht
            dh = np.where(starts[t][:, None] != 0, dtype(0), carried) + _rne(g_latent[t - 1]).astype(dtype) @ wot
    return np.stack(out_x), np.stack(out_h)


@functools.lru_cache(maxsize=None)
def _tolerances():
    """8 x the largest float32-vs-float64 difference of the two step-wise recipes on the (6, 33) inputs, from the references alone: the operands
    are the float64 chain's own values as float32.  -> (forward, backward)"""
    obs, starts, h0 = _inputs(6, 33)
    h, fwd, hps, svs = h0, 0.0, [], []
    for t in range(6):
        x, hp = _frame(obs[t]), np.where(starts[t][:, None] != 0, np.float32(0), h)
        (h32, s32), (h64, s64) = _step(x, hp, np.float32), _step(x, hp, np.float64)
        h = h64.astype(np.float32)
        fwd = max(fwd, np.abs(h32 - h64).max(), np.abs(s32 - s64).max(), np.abs(_latent(h, np.float32) - _latent(h, np.float64)).max())
        hps.append(hp), svs.append(s64.astype(np.float32))
    g_latent = np.random.default_rng(5).normal(0, 1, (6, 33, Z)).astype(np.float32)
    a, b = _bptt(svs, hps, starts, g_latent, None, np.float32), _bptt(svs, hps, starts, g_latent, None, np.float64)
    return 8.0 * float(fwd), 8.0 * max(float(np.abs(x - y).max()) for x, y in zip(a, b))


def _encoder(dev):
    import torch
    from openroborl_amd import policy_hip
    return policy_hip.GruEncoder({k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in _weights().items()}, dev, bf16=True)


@pytest.mark.parametrize("with_h0", [True, False])
@pytest.mark.parametrize("T,n", CASES)
def test_forward_matches_stepwise_float64(T, n, with_h0):
    import torch
    dev = torch.device("cuda:0")
    obs, starts, h0 = _inputs(T, n)
    h0 = h0 if with_h0 else None
    got = _forward(_encoder(dev), dev, obs, starts, h0)                 # guarded outputs: the pads are checked there
    tol, worst = _tolerances()[0], 0.0
    assert np.array_equal(got["frames"], _frame(obs))
    assert np.array_equal(got["hprev"][0], np.where(starts[0][:, None] != 0, np.float32(0), np.zeros((n, H), np.float32) if h0 is None else h0))
    assert np.array_equal(got["hprev"][1:], np.where(starts[1:][:, :, None] != 0, np.float32(0), got["hid"][:-1]))
    for t in range(T):
        h, s = _step(got["frames"][t], got["hprev"][t], np.float64)
        for name, a, b in (("hid", got["hid"][t], h), ("saved", got["saved"][t], s), ("latent", got["latent"][t], _latent(got["hid"][t], np.float64))):
            err = np.abs(a - b).max()
            worst = max(worst, err)
            assert err < tol, (name, t, err, tol)
    print("T=%d n=%d h0=%s: largest error %.3e, tolerance %.3e" % (T, n, with_h0, worst, tol))


@pytest.mark.parametrize("T,n", [(3, 16), (6, 33)])
def test_backward_matches_stepwise_float64(T, n):
    import torch
    from openroborl_amd import _abi, _lib
    dev = torch.device("cuda:0")
    L = _lib.load()
    obs, starts, h0 = _inputs(T, n)
    fwd = _forward(_encoder(dev), dev, obs, starts, h0)
    g_latent = np.random.default_rng(5).normal(0, 1, (T, n, Z)).astype(np.float32)
    images = []
    for key, shape in (("model/gru_h/w:0", (G, H)), ("model/gru_out/w:0", (Z, H))):
        src = torch.from_numpy(_weights()[key].astype(np.float32)).to(dev)
        images.append(torch.empty(int(L.orr_gru_packed_bf16_size(*shape)), dtype=torch.bfloat16, device=dev))
        _lib.check(L.orr_gru_pack_bf16(src.data_ptr(), src.shape[0], src.shape[1], 1, images[-1].data_ptr(), None), L)
    rows = _abi.gru_backward_rows(n)
    bufs = {"g_x": _guarded((T, n, G), dev), "g_h": _guarded((T, n, G), dev), "partials": _guarded((2, rows, G), dev)}
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (g_latent, fwd["saved"], fwd["hprev"], starts)]
    _lib.check(L.orr_gru_backward_bf16(C.byref(_abi.OrrGruTransposed(images[0].data_ptr(), images[1].data_ptr())), *(x.data_ptr() for x in ins), T, n,
                                       *(bufs[k][1].data_ptr() for k in ("g_x", "g_h", "partials")), None), L)
    torch.cuda.synchronize()
    assert all(_pads_untouched(full) for full, _ in bufs.values())
    got = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    want_x, want_h = _bptt(fwd["saved"], fwd["hprev"], starts, g_latent, got["g_h"], np.float64)
    tol = _tolerances()[1]
    err = max(np.abs(got["g_x"] - want_x).max(), np.abs(got["g_h"] - want_h).max())
    print("T=%d n=%d: g_x / g_h error %.3e, tolerance %.3e" % (T, n, err, tol))
    assert err < tol
    for k, name in enumerate(("g_x", "g_h")):                 # the bias sums against the kernel's own rows, by the same rule on a sequential sum
        rows64 = got[name].reshape(T * n, G).astype(np.float64)
        bound = 8.0 * np.abs(np.cumsum(got[name].reshape(T * n, G), axis=0, dtype=np.float32)[-1] - rows64.sum(0)).max() / np.abs(rows64.sum(0)).max()
        rel = np.abs(got["partials"][k].astype(np.float64).sum(0) - rows64.sum(0)).max() / np.abs(rows64.sum(0)).max()
        print("bias sums of %s: relative error %.3e, bound %.3e" % (name, rel, bound))
        assert rel < bound


def test_chaining_determinism_and_optional_outputs():
    import torch
    dev = torch.device("cuda:0")
    T, n = 6, 33
    obs, starts, h0 = _inputs(T, n)
    enc = _encoder(dev)
    whole, again = _forward(enc, dev, obs, starts, h0), _forward(enc, dev, obs, starts, h0)
    assert all(np.array_equal(whole[k], again[k]) for k in whole)
    bare, only_latent = _forward(enc, dev, obs, starts, h0, names=()), _forward(enc, dev, obs, starts, h0, names=("latent",))
    assert np.array_equal(bare["hid"], whole["hid"]) and all(np.array_equal(only_latent[k], whole[k]) for k in only_latent)
    h, o, s = torch.from_numpy(h0).to(dev), torch.from_numpy(obs).to(dev), torch.from_numpy(starts).to(dev)
    z = torch.empty((1, n, Z), device=dev)
    for t in range(T):                                                                    # six steps in place: hid is h0
        enc.forward(o[t:t + 1], s[t:t + 1], h, hid=h.view(1, n, H), latent=z)
        assert np.array_equal(h.cpu().numpy(), whole["hid"][t]) and np.array_equal(z[0].cpu().numpy(), whole["latent"][t])


LEARNER_GRADIENT_BOUND = 1.53e-2       # 4 x the 3.811e-3 measured on an MI355X (profiles/gru_bf16.txt), under bf16_gemm.txt's ceiling of 5e-2


def test_learner_gradient_and_graph_replay():
    import torch
    from openroborl_amd import history, learner_hip
    dev = torch.device("cuda:0")
    T, N, m = 4, 48, 16
    model = _student(dev, 4)
    obs, starts, h0, target = _segment(dev, T, N, 0)
    rows = slice(m, 2 * m)                                     # the second minibatch of whole robots
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items() if k.startswith("model/gru_")}
    _, z = history.encode_seq(p64, obs[:, rows].cpu().double(), starts[:, rows].cpu(), h0[rows].cpu().double())
    ((z - target[:, rows].cpu().double()) ** 2).sum(dim=-1).mean().backward()
    learner = learner_hip.FusedDistillRecurrent(model, lr=1e-4, minibatch=T * m, use_graph=False, bf16_gemm=True)
    learner.T, learner.minibatch = T, m
    P = learner._plan(N, m)
    with torch.no_grad():
        P["obs"].copy_(obs), P["starts"].copy_(starts.view(torch.uint8)), P["h0"].copy_(h0), P["target"].copy_(target)
        P["perm"].copy_(torch.arange(N, device=dev))
        learner._minibatch(P, 1)
    got = np.concatenate([learner.g[k].detach().cpu().numpy().ravel() for k in sorted(p64)]).astype(np.float64)
    want = np.concatenate([p64[k].grad.numpy().ravel() for k in sorted(p64)])
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("flat gradient, norm-wise relative error against unrounded float64 autograd: %.3e" % err)
    assert err < LEARNER_GRADIENT_BOUND
    models = [_student(dev, 2), _student(dev, 2)]
    for model, graph in zip(models, (False, True)):
        fused = learner_hip.FusedDistillRecurrent(model, lr=1e-4, minibatch=T * m, use_graph=graph, bf16_gemm=True)
        for it in range(2):
            fused.update(obs, starts, h0, target, epochs=2, generator=torch.Generator(device=dev).manual_seed(10 + it))
    assert all(torch.equal(models[0].p[k], models[1].p[k]) for k in models[0].p)


REFUSALS = [("forward", {"obs": None}), ("forward", {"wh": +2}), ("forward", {"T": 0}), ("forward", {"hprev": "hid"}), ("backward", {"g_x": None}),
            ("backward", {"wht": +2}), ("backward", {"T": 0}), ("backward", {"g_h": "g_x"}), ("pack", {"hid": None}), ("pack", {"hid": +2})]


@pytest.mark.parametrize("entry,change", REFUSALS)
def test_entry_points_refuse(entry, change):
    """None: a null pointer; an integer: that many bytes off (a misaligned image for wh / wht); a name: the other buffer's address (an overlap).
    The refusals come before any launch, so the image pointers only have to be aligned: the f32 encoder's serve."""
    import torch
    from openroborl_amd import _abi
    dev = torch.device("cuda:0")
    L, keep, p = _raw_args(dev)
    enc, encT = _abi.OrrGruEncoder.from_buffer_copy(keep["enc"].enc), _abi.OrrGruTransposed(keep["wt"].data_ptr(), keep["wt"].data_ptr())
    for k, v in change.items():
        if k in ("wh", "wht"):
            setattr(enc if k == "wh" else encT, k, getattr(enc if k == "wh" else encT, k) + v)
        else:
            p[k] = v if (v is None or k in ("T", "n")) else (p[v] if isinstance(v, str) else p[k] + v)
    if entry == "forward":
        rc = L.orr_gru_forward_bf16(C.byref(enc), p["obs"], p["starts"], p["h0"], p["T"], p["n"], p["hid"], p["latent"], p["frames"], p["hprev"], p["saved"], None)
    elif entry == "backward":
        rc = L.orr_gru_backward_bf16(C.byref(encT), p["g_latent"], p["saved"], p["hprev"], p["starts"], p["T"], p["n"], p["g_x"], p["g_h"], p["partials"], None)
    else:
        rc = L.orr_gru_pack_bf16(p["h0"], 17, H, 1, p["hid"], None)       # `hid` as the image's buffer
    torch.cuda.synchronize()
    assert rc < 0 and L.orr_last_error()
    assert all(bool((full == SENTINEL).all()) for full, _ in keep["bufs"].values())


def test_train_accepts_the_flag_and_still_refuses_the_mlp_flags(tmp_path):
    import json
    from tests import gpu_kit
    gpu_kit.train_refuses(["--distill", "x.zip", "--recurrent", "--hip-forward", "--num-robot", "64", "--iters", "1"], "--recurrent has kernels of its own")
    teacher, student, log_path = str(tmp_path / "teacher.zip"), str(tmp_path / "student.zip"), str(tmp_path / "log.json")
    common = ["--num-robot", "64", "--horizon", "8", "--push", "0.05,0.2,0.5"]
    gpu_kit.run_train("--privileged-actor", "--iters", "1", "--save", teacher, *common)
    gpu_kit.run_train("--distill", teacher, "--recurrent", "--bf16-gemm", "--iters", "3", "--save", student, "--log", log_path, *common)
    log = json.load(open(log_path))
    assert log[-1]["iter"] == 2 and all(np.isfinite(rec["latent_loss"]) and rec["latent_loss"] > 0.0 for rec in log)
    rec = json.loads(gpu_kit.run_train("--eval", student, "--bf16-gemm", "--num-robot", "16").strip().splitlines()[-1])
    assert rec["robots"] == 16 and np.isfinite(rec["return_mean"])
