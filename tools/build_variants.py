#!/usr/bin/env python3
"""Build differently compiled copies of the library for tools/ab_variants.sh (development aid; build container).

usage: python tools/build_variants.py name=[main|w2|both]:flag,flag,... [name=...]      ("base=main:" = the shipped flags)
The flags replace / extend one of the two flag sets of the env kernels' units (openroborl_amd/_lib.py: UNITS): main = HIPCC_FLAGS
(orr_kernels.hip: the one-wave step kernel, ILP scheduler, and the friction-anchor and clip-set units, which share its flags);
w2 = HIPCC_FLAGS_W2 (orr_kernels_w2.hip: the two-waves-per-SIMD step kernel); the other set keeps its shipped flags.
A flag set that names an -amdgpu-sched-strategy replaces the unit's own; "nosched" removes it; -O1/-O2/-O3/-Os replace -O2.
Example: python tools/build_variants.py base=main: w2ilp=w2:-mllvm,-amdgpu-sched-strategy=iterative-ilp w2o3=w2:-O3
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openroborl_amd import _lib  # noqa: E402


def apply(base, extra):
    base = [f for f in base if f != "-shared"]
    extra = list(extra)

    def drop_sched(fl):
        for k, f in enumerate(fl):
            if "amdgpu-sched-strategy" in f:
                del fl[k - 1:k + 1]
                return
    if any("amdgpu-sched-strategy" in f for f in extra) or "nosched" in extra:
        drop_sched(base)
    if "nosched" in extra:
        extra.remove("nosched")
    if any(f in ("-O1", "-O2", "-O3", "-Os") for f in extra):
        base = [f for f in base if f != "-O2"]
    return base + extra


SHIPPED = (list(_lib.HIPCC_FLAGS), list(_lib.HIPCC_FLAGS_W2))
for spec in sys.argv[1:]:
    name, _, rest = spec.partition("=")
    tu, _, fl = rest.partition(":")
    extra = [f for f in fl.split(",") if f]
    # the unit table refers to these two lists: change them in place, and _lib.build() compiles and links ALL units with them
    _lib.HIPCC_FLAGS[:] = apply(SHIPPED[0], extra if tu in ("main", "both") else [])
    _lib.HIPCC_FLAGS_W2[:] = apply(SHIPPED[1], extra if tu in ("w2", "both") else [])
    out = _lib.build(out_path=os.path.join(ROOT, "openroborl_amd", "lib_var_%s.so" % name))
    print("built", out, tu, " ".join(extra))
