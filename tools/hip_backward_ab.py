"""orr_wgrad / orr_dgrad_relu against the library calls they replace (development aid, GPU box), alternated in one process at the learners'
shapes: the 16-way bmm + its finish against orr_wgrad + its finish; mm + orr_relu_backward + finish against orr_dgrad_relu + finish.
Prints per shape the median and the range over the rounds of the mean time of a launch sequence, and the largest difference of the results.

usage:  python tools/hip_backward_ab.py [m=16384] [rounds=7] [reps=100] [bf16]
        bf16: a third column, orr_wgrad_bf16 / orr_dgrad_relu_bf16 + their finish
"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from openroborl_amd import _abi, _lib  # noqa: E402

BF16 = "bf16" in sys.argv
sys.argv = [a for a in sys.argv if a != "bf16"]
m, rounds, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 16384), (2, 7), (3, 100)))
dev = torch.device("cuda", 0)
L = _lib.load()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
f = lambda *shape: torch.randn(*shape, device=dev)   # noqa: E731


def job(p, o, r, c):
    return (_abi.OrrColsumJob * 1)(_abi.OrrColsumJob(p.data_ptr(), o.data_ptr(), r, c))


def ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def compare(name, old, new, outs, new_bf16):
    fns = (old, new, new_bf16) if BF16 else (old, new)
    for fn in fns:
        for _ in range(10):
            fn()
    a, b, c = ([o.clone() for o in outs(fn)] for fn in (old, new, new_bf16 if BF16 else new))
    t = {"library": [], "hip": [], "bf16": []}
    for _ in range(rounds):
        for key, fn in zip(("library", "hip", "bf16"), fns):
            t[key].append(ms(fn))
    rel = lambda p, q: max((x - y).abs().max().item() / (x.abs().max().item() + 1e-30) for x, y in zip(p, q))   # noqa: E731
    line = ("%-28s library %6.1f us (%.1f .. %.1f)   hip %6.1f us (%.1f .. %.1f)   largest difference %.1e of the largest entry"
            % (name, statistics.median(t["library"]), min(t["library"]), max(t["library"]), statistics.median(t["hip"]), min(t["hip"]),
               max(t["hip"]), rel(a, b)))
    if BF16:
        line += "   bf16 %6.1f us (%.1f .. %.1f)   %.1e" % (statistics.median(t["bf16"]), min(t["bf16"]), max(t["bf16"]), rel(a, c))
    print(line)


for k, n in ((160, 512), (208, 512), (512, 256), (256, 48)):
    x, g, gw = f(m, k), f(m, n), f(k, n)
    S, Sb = L.orr_wgrad_slices(m, k, n), L.orr_wgrad_bf16_slices(m, k, n)
    p_old, p_new, p_bf = f(16, k, n), f(S, k, n), f(Sb, k, n)
    j_old, j_new, j_bf = job(p_old, gw, 16, k * n), job(p_new, gw, S, k * n), job(p_bf, gw, Sb, k * n)

    def old():
        torch.bmm(x.view(16, m // 16, k).transpose(1, 2), g.view(16, m // 16, n), out=p_old)
        L.orr_colsum_finish(j_old, 1, st)

    def new():
        _lib.check(L.orr_wgrad(x.data_ptr(), k, g.data_ptr(), n, m, p_new.data_ptr(), st), L)
        L.orr_colsum_finish(j_new, 1, st)

    def new_bf16():
        _lib.check(L.orr_wgrad_bf16(x.data_ptr(), k, g.data_ptr(), n, m, p_bf.data_ptr(), st), L)
        L.orr_colsum_finish(j_bf, 1, st)

    def outs(fn):
        fn()
        return [gw]
    compare("wgrad %d x %d x %d, S = %d" % (m, k, n, S), old, new, outs, new_bf16)

for n, k in ((256, 512), (48, 256)):
    gz, w, h, gh, gb = f(m, n), f(k, n), torch.relu(f(m, k)), f(m, k), f(k)
    r_old, r_new = L.orr_learner_partial_rows(m), L.orr_dgrad_partial_rows(m)
    ws_old, ws_new = f(r_old, k), f(r_new, k)
    j_old, j_new = job(ws_old, gb, r_old, k), job(ws_new, gb, r_new, k)

    def old():
        torch.mm(gz, w.t(), out=gh)
        _lib.check(L.orr_relu_backward(gh.data_ptr(), h.data_ptr(), m, k, None, ws_old.data_ptr(), st), L)
        L.orr_colsum_finish(j_old, 1, st)

    def new():
        _lib.check(L.orr_dgrad_relu(gz.data_ptr(), w.data_ptr(), h.data_ptr(), m, n, k, gh.data_ptr(), ws_new.data_ptr(), st), L)
        L.orr_colsum_finish(j_new, 1, st)

    def new_bf16():
        _lib.check(L.orr_dgrad_relu_bf16(gz.data_ptr(), w.data_ptr(), h.data_ptr(), m, n, k, gh.data_ptr(), ws_new.data_ptr(), st), L)
        L.orr_colsum_finish(j_new, 1, st)

    def outs(fn):
        fn()
        return [gh, gb]
    compare("dgrad %d x %d x %d" % (m, n, k), old, new, outs, new_bf16)
