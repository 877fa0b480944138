"""Compile-only (no GPU): the env step kernels end without a device-wide cache write-back.

The launch tally is one packed 64-bit word (orr_env_kernels.h, end of orr_step_kernel), so no wave needs a fence between its counter
updates.  A `__threadfence()` compiles to `buffer_wbl2` (+ an L2 invalidate and waits) on gfx950; it cost 7 % of the 4096-robot launch.
Checked in the full env step (MODE 0) and its parity replay (MODE 2) of every translation unit that holds them.
"""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

from openroborl_amd import _lib

UNITS = [(src, flags) for _, src, flags, _ in _lib.ENV_UNITS]


def kernel_bodies(asm):
    """{symbol: instructions} of every orr_step_kernel instantiation in a device assembly listing"""
    lines = asm.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z15orr_step_kernel\S*):", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith("s_endpgm"))
            out[m.group(1)] = [t.split(";")[0].strip() for t in lines[i:end + 1]]
    return out


def compile_unit(src, flags, out_dir):
    out = os.path.join(out_dir, os.path.basename(src) + ".s")
    f = [x for x in flags if x not in ("-shared", "-fPIC")]
    subprocess.check_call([_lib.HIPCC] + f + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
    with open(out) as fh:
        return fh.read()


def front_end_compiles(src, defs):
    """`src` with the extra defines through the device compiler's front end only (syntax, templates, static_asserts); the completed process"""
    base = [f for f in _lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-fsyntax-only", "-Wno-unused-command-line-argument"]
    return subprocess.run([_lib.HIPCC] + base + defs + [src], capture_output=True, text=True)


def assert_no_cache_writeback(bodies, what=""):
    for sym, body in bodies.items():
        bad = [t for t in body if t.startswith("buffer_wbl2") or t.startswith("buffer_inv")]
        assert not bad, (what, sym, bad[:4])


def test_no_cache_writeback_in_step_kernels():
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(len(UNITS)) as ex:
        asms = list(ex.map(lambda u: compile_unit(u[0], u[1], d), UNITS))
    checked = []
    for (src, _), asm in zip(UNITS, asms):
        bodies = {sym: body for sym, body in kernel_bodies(asm).items() if int(re.match(r"_Z15orr_step_kernelILi(\d+)E", sym).group(1)) in (0, 2)}
        checked += [(os.path.basename(src), sym) for sym in bodies]
        assert_no_cache_writeback(bodies, os.path.basename(src))
    # MODE 0 in all four units (one-wave, two-wave, friction anchors, clip sets), MODE 2 in the main and the clip-set units
    assert len(checked) == 6, checked
