"""Builder + ctypes loader of the variant rule's host probe (tests/host_probe/orr_variant_probe.cpp) -- test infrastructure only.

The probe wraps csrc/orr_variants.h, the pure rule by which the C-ABI chooses the instantiation of the env kernels that an entry point
launches.  It is plain C++ without device code: no GPU, no offload, about a second to compile.  The library goes where the caller
says (the tests: pytest's temporary directory); it is no part of libopenroborl_hip.so.
"""
import ctypes as C
import os
import subprocess

from openroborl_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_probe", "orr_variant_probe.cpp")
FEATURES = ("anchors", "clips", "noise", "terms", "contacts", "actuator", "sensor", "randomizer", "push", "two_wave")   # orr::Features, in order
ENTRIES = ("orr_step", "orr_reset", "orr_debug_physics", "orr_debug_replay_step", "orr_debug_replay_reset")           # orr::Entry, in order

_probe = None


def compile_command(out):
    return [_lib.HIPCC, "-x", "c++", "-std=c++17", "-shared", "-fPIC", "-I", _lib.CSRC, "-o", out, SRC]


class Probe:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        L.orrv_entry_name.restype = L.orrv_variant_name.restype = C.c_char_p
        L.orrv_choose.argtypes = [C.c_uint, C.c_int]
        L.orrv_message.argtypes = [C.c_uint, C.c_int, C.c_char_p, C.c_int]
        assert tuple(L.orrv_entry_name(e).decode() for e in range(L.orrv_num_entries())) == ENTRIES
        self.variants = tuple(L.orrv_variant_name(v).decode() for v in range(L.orrv_num_variants()))

    @staticmethod
    def mask(features):
        return sum(1 << FEATURES.index(f) for f in set(features))

    def choose(self, features, entry):
        """(variant name, message) for a set of feature names (or a mask) at the entry point `entry` (a name of ENTRIES); the message
        is None unless the variant is kRefused."""
        mask = features if isinstance(features, int) else self.mask(features)
        e = ENTRIES.index(entry)
        name = self.L.orrv_variant_name(self.L.orrv_choose(mask, e)).decode()
        buf = C.create_string_buffer(512)
        n = self.L.orrv_message(mask, e, buf, len(buf))
        assert (n > 0) == (name == "kRefused") and n < len(buf) and len(buf.value) == n
        return name, (buf.value.decode() if n else None)


def lib(tmp_path_factory):
    """The probe, compiled once per process into a directory of pytest's tmp_path_factory."""
    global _probe
    if _probe is None:
        out = str(tmp_path_factory.mktemp("variant_probe") / "liborr_variant_probe.so")
        subprocess.check_call(compile_command(out))
        _probe = Probe(out)
    return _probe
