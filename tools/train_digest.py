"""A digest of what train.py computes in every mode, to compare two checkouts (development aid, GPU box): a fixed list of train.py runs as
child processes, one at a time, and for each one line with a SHA-256 over its --log records without "sec" (--eval: the printed record) and
one over every array of each zip it saved, in sorted key order.

usage:  python tools/train_digest.py [--train PATH/train.py] [--dump DIR]
        --train: another checkout's train.py (the package it imports is the one on PYTHONPATH, else its own directory's)
        --dump:  also write each case's records without "sec" to DIR/<case>.json
The tool stops at the first child that does not exit 0.  Equal code gives equal lines where the run is reproducible; diff two outputs.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openroborl_amd import policy as pol  # noqa: E402

SHAPE = "--num-robot 64 --horizon 8 --iters 12 --seed 3"        # records at iterations 0, 10 and 11
PUSH = "--push 0.05,0.2,0.5"
# (name, flags, the zips it saves): every file name is relative to the run's own temporary directory, later cases read earlier ones' zips
CASES = [
    ("defaults", "", ()),
    ("learn-std-controls", "--learn-std --ent-coef 0.01 --max-grad-norm 0.5 --lr-schedule linear --kl-target 0.01", ()),
    ("critic-obs-norm", "--privileged-critic --obs-norm --obs-norm-freeze-after 5 %s --save normed.zip --save-folded folded.zip" % PUSH,
     ("normed.zip", "folded.zip")),
    ("clips-shaping", "--motion-file laikago_pace.txt --motion-file laikago_backwards_pace.txt --clip-curriculum 0.1,0.1 --reward-terms "
     "--contact-outputs --reward-shaping torque=1e-4,failure=1 --reward-shaping-ramp 4 --init-std 1.0", ()),
    ("teacher", "--privileged-actor %s --save teacher.zip" % PUSH, ("teacher.zip",)),
    ("distill", "--distill teacher.zip --distill-beta 0.5 --distill-beta-iters 6 --save plain.zip", ("plain.zip",)),
    ("distill-history", "--distill teacher.zip --history --distill-action-coef 0.5 --distill-latent-coef 0.5 --save student.zip", ("student.zip",)),
    ("history-ppo-tuned", "--history-ppo --model-file student.zip --latent-coef 0.5 --save tuned.zip", ("tuned.zip",)),
    ("history-ppo-kl-stop", "--history-ppo --learn-std --kl-stop 0.05 --reward-shaping failure=1", ()),
    ("torch-policy-learner", "--torch-policy --torch-learner", ()),
    ("history-ppo-torch", "--history-ppo --torch-learner", ()),
    ("distill-torch", "--distill teacher.zip --torch-learner", ()),
    ("eval", "--eval tuned.zip --num-robot 16", ()),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", default=os.path.join(ROOT, "train.py"))
    ap.add_argument("--dump", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per child")
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        for name, flags, zips in CASES:
            argv = flags.split() if name == "eval" else SHAPE.split() + flags.split() + ["--log", "log.json"]
            r = subprocess.run([sys.executable, os.path.abspath(a.train)] + argv, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               timeout=a.timeout)
            if r.returncode != 0:
                sys.exit("%s: exit status %d\n%s" % (name, r.returncode, r.stdout.decode()[-3000:]))
            if name == "eval":
                recs = [json.loads(r.stdout.decode().strip().splitlines()[-1])]
            else:
                with open(os.path.join(work, "log.json")) as f:
                    recs = [{k: v for k, v in rec.items() if k != "sec"} for rec in json.load(f)]
            h = hashlib.sha256()
            for z in zips:
                w = pol.load_parameters(os.path.join(work, z))
                for k in sorted(w):
                    h.update(k.encode() + np.asarray(w[k]).tobytes())
            print("%-22s log %s  zips %s" % (name, hashlib.sha256(json.dumps(recs).encode()).hexdigest(), h.hexdigest() if zips else "-"), flush=True)
            if a.dump:
                with open(os.path.join(a.dump, name + ".json"), "w") as f:
                    json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
