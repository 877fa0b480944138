"""Child process of tests/test_gpu_substep_stages.py: loads the -DORR_STAGE_DUMP build of the library (tools/dev_build.py; a process can
load one build only, and ORR_LIB_PATH has to be set before it does), dumps the stages of every bucket of tests/stage_refs.py with both
step units' code (ORR_STEP_WAVES_PER_EU = 1, 2) and both friction-anchor forms, and writes the dumps to the .npz named on the command
line.  Every launch is checked; the first error ends the process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dev_build  # noqa: E402

L = dev_build.load(*dev_build.STAGE_DUMP)          # before anything loads the library
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openroborl_amd import _lib  # noqa: E402
from openroborl_amd.env import VecQuadrupedEnv  # noqa: E402
from tests import gpu_kit  # noqa: E402
from tests import stage_refs as SR  # noqa: E402

L.orr_debug_stage_words.restype = L.orr_debug_stage_dump.restype = __import__("ctypes").c_int32
assert L.orr_debug_stage_words() == SR.WORDS, (L.orr_debug_stage_words(), SR.WORDS)
# one robot of a bucket alone, seven of it, and one record in all four places of a wave: (bucket, robot)
SMALL = (("warm", "mini_cheetah"), ("limit_inside", "laikago"))


def dump(inp, anchor, room=None):
    """-> [room, WORDS] float32: the stages of the bucket's robots; the buffer is pre-filled with NaN and has room for `room` robots"""
    n = len(inp.st)
    room = room or n
    env = VecQuadrupedEnv(num_robot=n, **inp.env_kwargs(anchor))
    assert bool(env.L.orr_debug_stage_words() == SR.WORDS)
    for k in ("sim_dt", "contact_margin", "contact_erp", "limit_activation", "warmstart_factor", "plane_friction", "friction_erp", "gravity_z"):
        assert getattr(env.cfg, k) == getattr(inp.cfg, k), k
    gpu_kit.push_state(env, inp.st)
    before = env.state.clone()
    tau = torch.tensor(inp.tau, dtype=torch.float32, device=env.device).contiguous()
    out = torch.full((room * SR.WORDS,), float("nan"), dtype=torch.float32, device=env.device)
    # bad arguments are refused: a missing buffer, a buffer too small for the batch
    assert L.orr_debug_stage_dump(env.h, None, out.data_ptr(), out.numel(), env._stream()) != 0
    assert L.orr_debug_stage_dump(env.h, tau.data_ptr(), None, out.numel(), env._stream()) != 0
    assert L.orr_debug_stage_dump(env.h, tau.data_ptr(), out.data_ptr(), n * SR.WORDS - 1, env._stream()) != 0
    assert L.orr_debug_stage_dump(None, tau.data_ptr(), out.data_ptr(), out.numel(), env._stream()) != 0
    _lib.check(L.orr_debug_stage_dump(env.h, tau.data_ptr(), out.data_ptr(), out.numel(), env._stream()), L)
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), before.view(torch.int32)), "the dump changed the records"
    res = out.cpu().numpy().reshape(room, SR.WORDS)
    env.close()
    return res


def main(path):
    out = {}
    for wpe in (1, 2):
        os.environ["ORR_STEP_WAVES_PER_EU"] = str(wpe)       # read by orr_create: which unit's kernel the handle runs
        for anchor in (False, True):
            for bucket, robot in SR.cases():
                if bucket == "anchor" and not anchor:
                    continue                                 # its models carry the anchor: there is no plain form of it
                out["%s/%s/w%d/a%d" % (bucket, robot, wpe, anchor)] = dump(SR.inputs(bucket, robot), anchor)
        for bucket, robot in SMALL:
            inp = SR.inputs(bucket, robot)
            out["seven/%s/%s/w%d" % (bucket, robot, wpe)] = dump(inp.subset(list(range(7))), False, room=8)
            out["one/%s/%s/w%d" % (bucket, robot, wpe)] = dump(inp.subset([5]), False, room=4)
            out["places/%s/%s/w%d" % (bucket, robot, wpe)] = dump(inp.subset([9, 9, 9, 9]), False)
        print("unit w%d dumped" % wpe, flush=True)
    np.savez(path, **out)
    print("STAGE DUMP OK", len(out))


if __name__ == "__main__":
    main(sys.argv[1])
