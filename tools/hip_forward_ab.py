"""orr_dense_forward against the library calls it replaces (development aid, GPU box), alternated in one process at the learners' shapes:
layer 0 at 160 -> 512 and 208 -> 512 with the index_select gathers (and the cat) on the library side and the row tables on the other,
the hidden layer 512 -> 256, the output layers 256 -> 12 and 256 -> 1, and the encoder chain 512 -> 256 -> 48 (its gather on both sides).
Prints per shape the median and the range over the rounds of the mean time of a launch sequence, and the largest difference of the results.

usage:  python tools/hip_forward_ab.py [m=16384] [rounds=7] [reps=100] [bf16]
        bf16: a third column, orr_dense_forward_bf16 (the layers of a fan-out that is a multiple of 16; the others run the f32 kernel)
"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from openroborl_amd import _lib  # noqa: E402

BF16 = "bf16" in sys.argv
sys.argv = [a for a in sys.argv if a != "bf16"]
m, rounds, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 16384), (2, 7), (3, 100)))
dev = torch.device("cuda", 0)
L = _lib.load()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
f = lambda *shape: torch.randn(*shape, device=dev)   # noqa: E731
B = 8 * m                                            # the rows an update gathers a minibatch from (train.py: 4096 robots x 32 steps)
idx = torch.randperm(B, device=dev)[:m]


def dense(xa, ra, xb, rb, w, b, relu, y, x_out, bf16=False):
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    entry = L.orr_dense_forward_bf16 if bf16 and w.shape[1] % 16 == 0 else L.orr_dense_forward
    _lib.check(entry(xa.data_ptr(), xa.shape[1], ptr(ra), ptr(xb), 0 if xb is None else xb.shape[1], ptr(rb), m, w.data_ptr(),
                                   b.data_ptr(), w.shape[1], relu, y.data_ptr(), ptr(x_out), st), L)


def ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def compare(name, old, new, outs_old, outs_new):
    for fn in (old, new):
        for _ in range(10):
            fn()
    for _ in range(10 if BF16 else 0):
        new(True)
    t = {"library": [], "hip": [], "bf16": []}
    for _ in range(rounds):
        t["library"].append(ms(old))
        t["hip"].append(ms(new))
        if BF16:
            t["bf16"].append(ms(lambda: new(True)))
    new()
    diff = max((x - y).abs().max().item() / (x.abs().max().item() + 1e-30) for x, y in zip(outs_old, outs_new))
    line = ("%-34s library %6.1f us (%.1f .. %.1f)   hip %6.1f us (%.1f .. %.1f)   largest difference %.1e of the largest entry"
            % (name, statistics.median(t["library"]), min(t["library"]), max(t["library"]), statistics.median(t["hip"]), min(t["hip"]),
               max(t["hip"]), diff))
    if BF16:
        new(True)
        diff = max((x - y).abs().max().item() / (x.abs().max().item() + 1e-30) for x, y in zip(outs_old, outs_new))
        line += "   bf16 %6.1f us (%.1f .. %.1f)   %.1e" % (statistics.median(t["bf16"]), min(t["bf16"]), max(t["bf16"]), diff)
    print(line)


# layer 0 behind the minibatch's gathers: obs alone, and obs | priv through a cat
for kb in (0, 48):
    obs, priv, w, b = f(B, 160), f(B, 48), f(160 + kb, 512) * 0.1, f(512)
    x, xp, xv, x_new = f(m, 160), f(m, 48), f(m, 208), f(m, 160 + kb)
    y_old, y_new = f(m, 512), f(m, 512)

    def old():
        torch.index_select(obs, 0, idx, out=x)
        if kb:
            torch.index_select(priv, 0, idx, out=xp)
            torch.cat((x, xp), dim=1, out=xv)
        torch._addmm_activation(b, xv if kb else x, w, out=y_old)

    def new(bf16=False):
        dense(obs, idx, priv if kb else None, idx if kb else None, w, b, 1, y_new, x_new, bf16)
    compare("gather + %d -> 512, ReLU" % (160 + kb), old, new, [y_old, xv if kb else x], [y_new, x_new])

for k, n, relu in ((512, 256, 1), (256, 12, 0), (256, 1, 0)):
    x, w, b, y_old, y_new = f(m, k), f(k, n) * 0.1, f(n), f(m, n), f(m, n)

    def old():
        if relu:
            torch._addmm_activation(b, x, w, out=y_old)
        else:
            torch.addmm(b, x, w, out=y_old)

    def new(bf16=False):
        dense(x, None, None, None, w, b, relu, y_new, None, bf16)
    compare("%d -> %d%s" % (k, n, ", ReLU" if relu else ""), old, new, [y_old], [y_new])

hist, w0, b0, w1, b1 = f(B, 512), f(512, 256) * 0.1, f(256), f(256, 48) * 0.1, f(48)
xh_old, xh_new, he_old, he_new, z_old, z_new = f(m, 512), f(m, 512), f(m, 256), f(m, 256), f(m, 48), f(m, 48)


def enc_old():
    torch.index_select(hist, 0, idx, out=xh_old)
    torch._addmm_activation(b0, xh_old, w0, out=he_old)
    torch.addmm(b1, he_old, w1, out=z_old)


def enc_new(bf16=False):
    dense(hist, idx, None, None, w0, b0, 1, he_new, xh_new, bf16)
    dense(he_new, None, None, None, w1, b1, 0, z_new, None, bf16)


compare("gather + 512 -> 256 -> 48", enc_old, enc_new, [z_old, xh_old], [z_new, xh_new])
