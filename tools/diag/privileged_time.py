"""The privileged critic's two kernels against what they sit next to, 4096 robots, same process, alternated (the protocol of
tools/diag/variant_time.py: medians of 5 x 300 back-to-back launches, every candidate sees the same clocks; the 300 launches are one
captured graph, so that no host time sits between them):
python tools/diag/privileged_time.py [--alt-policy-lib PATH] [--sections forward,history,row,head,history_priv,latent]

  forward   orr_policy_forward_priv, orr_policy_forward_teacher and orr_policy_forward_teacher with value = NULL (the labelling call of
            distillation: no critic) against orr_policy_forward, random weights; with --alt-policy-lib also orr_policy_forward_priv of a
            second build of csrc/orr_policy.hip (e.g. -DORR_POLICY_PRIV_SPLIT=0: the critic's layer 0 at pipeline depth 1 instead of
            12 + 1 k-groups), loaded next to the shipped library and run on the same packed weights
  history   orr_policy_forward_history (a history student: the encoder 512 -> 256 -> 48 in front of the teacher's pass) against
            orr_policy_forward_teacher, each with and without a value buffer, and orr_history_push per launch (out of place, no resets)
  row       orr_privileged_obs with contact and push outputs bound against the env step of the same env (train mode, randomiser, pushes
            at prob 0.02)
  head      orr_history_student_head at m = 16384 (a history student's action loss: forward through the frozen actor, both losses, backward
            to the latent, one launch) against the same mathematics composed from the older pieces on the same inputs: three torch GEMMs
            with bias / ReLU epilogues, orr_distill_head, orr_head_backward, two torch GEMMs with orr_relu_backward between them,
            orr_regress_head and the sum of the two gradients; and against orr_regress_head alone (the latent loss without the action loss)
  history_priv  orr_policy_forward_history_priv (a history policy with an asymmetric critic: the critic's layer 0 reads the true row) against
            orr_policy_forward_history, each with and without a value buffer; the MFMA counts are the same
  latent    orr_latent_backward at m = 16384 (PPO on a history policy: the gradient from the actor's layer 0 into the latent, the latent loss,
            the column sums) against the same mathematics composed from torch.mm, orr_regress_head, an add and a column sum"""
import argparse
import ctypes as C
import sys

import torch

sys.path.insert(0, '.')
from openroborl_amd import _abi, policy_hip, ppo  # noqa: E402
from openroborl_amd.env import VecQuadrupedEnv  # noqa: E402

N, WARMUP, ROUNDS, LAUNCHES = 4096, 300, 5, 300

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--alt-policy-lib", default="")
ap.add_argument("--sections", default="forward,history,row,head,history_priv,latent")
args = ap.parse_args()
sections = args.sections.split(",")
dev = torch.device("cuda", 0)


def timed(graph):
    """ms per launch of a graph of LAUNCHES back-to-back launches (no host time between them: the row's kernel is shorter than a Python call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def report(names, fns):
    graphs = []
    for fn in fns:
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(LAUNCHES):
                fn()
        gr.replay()
        graphs.append(gr)
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(ROUNDS):
        for j, gr in enumerate(graphs):
            ms[j].append(timed(gr))
    med = [sorted(m)[ROUNDS // 2] for m in ms]
    for name, m, mid in zip(names, ms, med):
        print("%-52s %.4f ms (median of %d x %d back-to-back launches; all: %s)" % (name, mid, ROUNDS, LAUNCHES, " ".join("%.4f" % x for x in m)))
    for name, mid in zip(names[1:], med[1:]):
        print("%s against %s: %+.2f %% (ratio %.4f)" % (name, names[0], 100.0 * (mid / med[0] - 1.0), mid / med[0]))
    return med


# ---- forward ----
model = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM)
plain = {k: v.detach().clone() for k, v in model.p.items()}
plain["model/vf_fc0/w:0"] = plain["model/vf_fc0/w:0"][:160].contiguous()
fp, f0 = policy_hip.FusedActorCritic(model.p, dev, std=0.125), policy_hip.FusedActorCritic(plain, dev, std=0.125)
g = torch.Generator(device=dev).manual_seed(0)
obs, priv, noise = (torch.randn(N, c, device=dev, generator=g) for c in (160, _abi.POLICY_PRIV_DIM, 12))
act, raw, val = torch.empty(N, 12, device=dev), torch.empty(N, 12, device=dev), torch.empty(N, device=dev)
teacher = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM, actor_priv_dim=_abi.POLICY_PRIV_DIM)
ft = policy_hip.FusedActorCritic(teacher.p, dev, std=0.125)
mean = torch.empty(N, 12, device=dev)
names = ["orr_policy_forward", "orr_policy_forward_priv", "orr_policy_forward_teacher", "orr_policy_forward_teacher, value = NULL"]
fns = [lambda: f0.forward(obs, noise, out_action=act, out_raw=raw, out_value=val),
       lambda: fp.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, priv=priv),
       lambda: ft.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, priv=priv),
       lambda: ft.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, priv=priv)]
if args.alt_policy_lib:
    alt = C.CDLL(args.alt_policy_lib)
    alt.orr_policy_forward_priv.restype = C.c_int32
    alt.orr_policy_forward_priv.argtypes = fp.L.orr_policy_forward_priv.argtypes
    val_alt = torch.empty(N, device=dev)

    def run_alt():
        rc = alt.orr_policy_forward_priv(C.byref(fp.net), obs.data_ptr(), priv.data_ptr(), N, noise.data_ptr(), 0.125, 6.2831853, act.data_ptr(),
                                         raw.data_ptr(), val_alt.data_ptr(), None, fp._stream())
        assert rc == 0
    names.append("orr_policy_forward_priv, --alt-policy-lib")
    fns.append(run_alt)
if "forward" in sections:
    med = report(names, fns)
    # MFMAs per wave: 1728 plain, 1824 with the critic's 13th k-group pair (+96), 1920 with the actor's too (+96); 992 without the critic
    print("orr_policy_forward_teacher against orr_policy_forward_priv: %+.2f %% (the MFMA counts give %+.2f %%)" % (100.0 * (med[2] / med[1] - 1.0), 100.0 * 96 / 1824))
    print("orr_policy_forward_teacher, value = NULL against orr_policy_forward_teacher: ratio %.4f (the MFMA counts give %.4f)" % (med[3] / med[2], 992.0 / 1920.0))
    if args.alt_policy_lib:
        fns[1](); run_alt(); torch.cuda.synchronize()
        print("the two builds' values are equal bit for bit: %s" % bool(torch.equal(val, val_alt)))

# ---- history ----
if "history" in sections:
    student = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM, actor_priv_dim=_abi.POLICY_PRIV_DIM, history=_abi.HISTORY_STEPS)
    fh = policy_hip.FusedActorCritic(student.p, dev, std=0.125)
    hist, hist2 = torch.randn(N, _abi.HISTORY_DIM, device=dev, generator=g), torch.empty(N, _abi.HISTORY_DIM, device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    med = report(["orr_policy_forward_teacher", "orr_policy_forward_teacher, value = NULL", "orr_policy_forward_history", "orr_policy_forward_history, value = NULL",
                  "orr_history_push"],
                 [fns[2], fns[3], lambda: fh.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, hist=hist),
                  lambda: fh.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, hist=hist),
                  lambda: policy_hip.history_push(obs, done, hist, hist2)])
    # MFMAs per wave: the encoder adds 512 (layer 0) + 64 (layer 1, on three of the four waves) to the teacher's 1920, or 992 without the critic
    print("orr_policy_forward_history against orr_policy_forward_teacher: ratio %.4f (the MFMA counts give %.4f)" % (med[2] / med[0], (1920.0 + 576.0) / 1920.0))
    print("the same with value = NULL: ratio %.4f (the MFMA counts give %.4f)" % (med[3] / med[1], (992.0 + 576.0) / 992.0))

# ---- row ----
if "row" in sections:
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=N, mode="train", auto_reset=True, seed=7, contact_outputs=True,
                          push=dict(prob=0.02, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True)
    o = env.reset()
    a = torch.empty(N, 12, device=dev)
    for k in range(WARMUP):
        env.stress_actions(o, torch.randn(N, 12, device=dev, generator=g) * 0.125, a)
        o, r, d, _ = env.step(a)
    rows = torch.empty(N, _abi.PRIV_DIM, device=dev)
    report(["env step (push variant, contact + push outputs)", "orr_privileged_obs"],
           [lambda: env.step_into(a, env.obs, env.reward, env.done), lambda: env.privileged_obs(out=rows, done=env.done)])
    env.close()

# ---- head ----
if "head" in sections:
    from openroborl_amd import _lib  # noqa: E402
    M, Z = 16384, _abi.POLICY_PRIV_DIM
    L = ft.L
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)   # noqa: E731
    w = {k: v.detach() for k, v in teacher.p.items()}
    w0, b0, w1, b1, w2, b2 = (w["model/pi%s/%s:0" % (s, x)] for s in ("_fc0", "_fc1", "") for x in ("w", "b"))
    w2t_pad = torch.zeros(16, 256, device=dev)
    w2t_pad[:12] = w2.t()
    packed = []
    for src in (w2t_pad, w1.t().contiguous(), w0[160:].t().contiguous()):
        out = torch.empty(int(L.orr_policy_packed_size(src.shape[0], src.shape[1])), device=dev)
        _lib.check(L.orr_policy_pack(src.data_ptr(), src.shape[0], src.shape[1], out.data_ptr(), st()), L)
        packed.append(out)
    xo, z, tm, tp = (torch.randn(M, c, device=dev, generator=g) for c in (160, Z, 12, Z))
    g_z, hp = torch.empty(M, Z, device=dev), torch.empty(50 * _abi.student_head_rows(M), device=dev)
    a_c, l_c = 1.0, 0.5

    def fused_head():
        _lib.check(L.orr_history_student_head(C.byref(ft.net), packed[0].data_ptr(), packed[1].data_ptr(), packed[2].data_ptr(), xo.data_ptr(), z.data_ptr(),
                                              tm.data_ptr(), tp.data_ptr(), M, a_c, l_c, g_z.data_ptr(), None, hp.data_ptr(), st()), L)
    # the composition: what the parent commit's pieces need for the same g_z (coefficients folded into two elementwise launches at the end)
    xin, h1, h2, y = (torch.empty(M, c, device=dev) for c in (160 + Z, 512, 256, 12))
    g_y, gz2, gh1, gin, g_lat, g_ref = (torch.empty(M, c, device=dev) for c in (12, 256, 512, Z, Z, Z))
    gb12, gb48, stats = torch.empty(12, device=dev), torch.empty(Z, device=dev), torch.empty(2, device=dev)
    ws, ws2, ws1 = (torch.empty(int(L.orr_learner_workspace_floats(M, c)), device=dev) for c in (64, 256, 512))
    w1t, w0zt = w1.t(), w0[160:].t()

    def composed():
        torch.cat((xo, z), dim=1, out=xin)
        torch._addmm_activation(b0, xin, w0, out=h1)
        torch._addmm_activation(b1, h1, w1, out=h2)
        torch.addmm(b2, h2, w2, out=y)
        _lib.check(L.orr_distill_head(y.data_ptr(), tm.data_ptr(), M, g_y.data_ptr(), gb12.data_ptr(), stats.data_ptr(), ws.data_ptr(), st()), L)
        _lib.check(L.orr_head_backward(g_y.data_ptr(), 12, w2.data_ptr(), h2.data_ptr(), M, 256, gz2.data_ptr(), None, None, ws2.data_ptr(), st()), L)
        torch.mm(gz2, w1t, out=gh1)
        _lib.check(L.orr_relu_backward(gh1.data_ptr(), h1.data_ptr(), M, 512, None, ws1.data_ptr(), st()), L)
        torch.mm(gh1, w0zt, out=gin)
        _lib.check(L.orr_regress_head(z.data_ptr(), tp.data_ptr(), M, Z, g_lat.data_ptr(), gb48.data_ptr(), stats[1:].data_ptr(), ws.data_ptr(), st()), L)
        torch.add(gin * a_c, g_lat, alpha=l_c, out=g_ref)

    def regress_alone():
        _lib.check(L.orr_regress_head(z.data_ptr(), tp.data_ptr(), M, Z, g_lat.data_ptr(), gb48.data_ptr(), stats[1:].data_ptr(), ws.data_ptr(), st()), L)
    fused_head(); composed(); torch.cuda.synchronize()
    scale = float(g_ref.abs().max())
    print("m = %d: the fused launch and the composition agree to %.2e of the gradient's scale" % (M, float((g_z - g_ref).abs().max()) / scale))
    med = report(["the composition (5 GEMMs + 5 launches + 3 elementwise)", "orr_history_student_head", "orr_regress_head alone"], [composed, fused_head, regress_alone])
    # MFMAs per wave and tile of 16 rows: 416 + 512 + 64 forward, 16 + 512 + 128 backward = 1648; the teacher's full forward pass 1920
    print("orr_history_student_head: %d workgroups of 1648 MFMAs per wave in %.4f ms; orr_policy_forward_teacher: 256 workgroups of 1920 (section forward)"
          % (M // 16, med[1]))

# ---- history_priv ----
if "history_priv" in sections:
    student = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM, actor_priv_dim=_abi.POLICY_PRIV_DIM, history=_abi.HISTORY_STEPS)
    fh = policy_hip.FusedActorCritic(student.p, dev, std=0.125)
    hist = torch.randn(N, _abi.HISTORY_DIM, device=dev, generator=g)
    med = report(["orr_policy_forward_history", "orr_policy_forward_history_priv", "orr_policy_forward_history, value = NULL",
                  "orr_policy_forward_history_priv, value = NULL"],
                 [lambda: fh.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, hist=hist),
                  lambda: fh.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, hist=hist, critic_priv=priv),
                  lambda: fh.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, hist=hist),
                  lambda: fh.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, hist=hist, critic_priv=priv)])
    # MFMAs per wave: 2496 in both; the asymmetric critic's layer 0 is three layer<> calls (10 + 2 + 1 k-groups) instead of two (12 + 1), and
    # the tile is 48 words wider (a 3 KB load of the true row)
    print("orr_policy_forward_history_priv against orr_policy_forward_history: ratio %.4f (the MFMA counts give 1.0000)" % (med[1] / med[0]))
    print("the same with value = NULL: ratio %.4f (the same code but the kernel's LDS, 112.2 -> 115.2 KB)" % (med[3] / med[2]))

# ---- latent ----
if "latent" in sections:
    from openroborl_amd import _lib  # noqa: E402,F811
    M, Z = 16384, _abi.POLICY_PRIV_DIM
    L = ft.L
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)   # noqa: E731
    w0z = teacher.p["model/pi_fc0/w:0"].detach()[160:]                    # [48][512]
    w0zt = w0z.t().contiguous()
    packed = torch.empty(int(L.orr_policy_packed_size(512, Z)), device=dev)
    _lib.check(L.orr_policy_pack(w0zt.data_ptr(), 512, Z, packed.data_ptr(), st()), L)
    g0 = torch.randn(M, 512, device=dev, generator=g) * (torch.rand(M, 512, device=dev, generator=g) < 0.5) / M
    z, tp = (torch.randn(M, Z, device=dev, generator=g) for _ in range(2))
    rows = _abi.latent_backward_rows(M)
    g_z, lp, gb, loss = torch.empty(M, Z, device=dev), torch.empty(49 * rows, device=dev), torch.empty(Z, device=dev), torch.empty(1, device=dev)
    jobs = (_abi.OrrColsumJob * 2)(_abi.OrrColsumJob(lp.data_ptr(), gb.data_ptr(), rows, Z), _abi.OrrColsumJob(lp.data_ptr() + 4 * Z * rows, loss.data_ptr(), rows, 1))
    coef = 0.5

    def fused_latent():
        _lib.check(L.orr_latent_backward(g0.data_ptr(), packed.data_ptr(), z.data_ptr(), tp.data_ptr(), M, coef, g_z.data_ptr(), lp.data_ptr(), st()), L)
        _lib.check(L.orr_colsum_finish(jobs, 2, st()), L)

    def kernel_alone():
        _lib.check(L.orr_latent_backward(g0.data_ptr(), packed.data_ptr(), z.data_ptr(), tp.data_ptr(), M, coef, g_z.data_ptr(), lp.data_ptr(), st()), L)
    gin, g_lat, g_ref, gb_ref, gb48, stat = (torch.empty(s, device=dev) for s in ((M, Z), (M, Z), (M, Z), (Z,), (Z,), (1,)))
    ws = torch.empty(int(L.orr_learner_workspace_floats(M, 64)), device=dev)
    w0z_t = w0z.t()

    def composed():          # the library GEMM (N = 48), the latent loss head, the sum of the two gradients, and a column sum in torch's order
        torch.mm(g0, w0z_t, out=gin)
        _lib.check(L.orr_regress_head(z.data_ptr(), tp.data_ptr(), M, Z, g_lat.data_ptr(), gb48.data_ptr(), stat.data_ptr(), ws.data_ptr(), st()), L)
        torch.add(gin, g_lat, alpha=coef, out=g_ref)
        torch.sum(g_ref, dim=0, out=gb_ref)
    fused_latent(); composed(); torch.cuda.synchronize()
    scale = float(g_ref.abs().max())
    print("m = %d: orr_latent_backward and the composition agree to %.2e of the gradient's scale, the column sums to %.2e, the loss to %.2e"
          % (M, float((g_z - g_ref).abs().max()) / scale, float((gb - gb_ref).abs().max()) / float(gb_ref.abs().max()), abs(loss.item() - stat.item()) / stat.item()))
    report(["the composition (torch.mm + orr_regress_head + add + column sum)", "orr_latent_backward + orr_colsum_finish", "orr_latent_backward alone"],
           [composed, fused_latent, kernel_alone])
