#!/usr/bin/env python3
"""End-to-end motion-imitation training on the device: env (HIP kernels) + batched policy + GAE + PPO, nothing
leaves the GPU.  Counterpart of `python3 OpenRoboRL/run.py --task imitation_learning_laikago` in train mode
(run.py:186-237), restricted to what SURVEY.md section 8f lists as "next" rows.

  python train.py --task imitation_learning_laikago --iters 200
  python train.py --task imitation_learning_laikago --iters 200 --learn-std --ent-coef 0.01   (a learned exploration width, entropy / KL / clip fraction in the log)
  python train.py --task imitation_learning_laikago --iters 200 --max-grad-norm 0.5 --lr-schedule linear --kl-target 0.01   (update controls on the device)
  python train.py --task imitation_learning_laikago --iters 200 --obs-norm --save normed.zip --save-folded plain.zip   (running observation normalisation, folded into layer 0)
  python train.py --task imitation_learning_laikago --iters 200 --privileged-critic --push 0.02,0.2,0.5   (asymmetric actor-critic)
  python train.py --task imitation_learning_laikago --iters 200 --privileged-actor --push 0.02,0.2,0.5 --save teacher.zip   (a teacher)
  python train.py --task imitation_learning_laikago --iters 200 --distill teacher.zip --push 0.02,0.2,0.5 --save student.zip   (its student)
  python train.py --task imitation_learning_laikago --iters 200 --distill teacher.zip --history --push 0.02,0.2,0.5 --save student.zip   (a history student)
  python train.py --task imitation_learning_laikago --iters 200 --history-ppo --model-file student.zip --push 0.02,0.2,0.5 --save tuned.zip   (PPO on it)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def control_args(ap):
    """The flags of the update controls (learner_hip: orr_update_control + orr_adam_step_ctl; --torch-learner: ppo._UpdateControl)."""
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global gradient norm to X before every optimiser step (torch.nn.utils.clip_grad_norm_'s formula); with any of "
                         "these flags a step whose gradient is not finite is skipped and counted instead of taken")
    ap.add_argument("--lr-schedule", choices=("constant", "linear"), default="constant",
                    help="linear: lr * max(1 - it / iters, 0), the reference's schedule='linear' (agents/ppo_imitation.py:296-299), set once per "
                         "iteration on the device: the captured update is not captured again")
    ap.add_argument("--kl-stop", type=float, default=None, metavar="X",
                    help="PPO: stop the rest of an update once a minibatch's approx_kl exceeds X (that minibatch's step included)")
    ap.add_argument("--kl-target", type=float, default=None, metavar="X",
                    help="PPO: KL-adaptive learning rate, per step: approx_kl > 2 X: lr / 1.5; 0 < approx_kl < X / 2: lr * 1.5")
    ap.add_argument("--kl-lr-bounds", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="--kl-target: the adaptive learning rate stays within [LO, HI] times --lr (default 0.01 10)")


def control_kwargs(args, kl=True):
    """The learners' keywords for the flags of control_args; no flag, no keyword.  kl: a PPO learner (the distillation learners have no KL)."""
    if not kl and (args.kl_stop is not None or args.kl_target is not None):
        raise SystemExit("train.py: --kl-stop / --kl-target belong to PPO; the distillation learners have no KL")
    if args.kl_lr_bounds is not None and args.kl_target is None:
        raise SystemExit("train.py: --kl-lr-bounds belongs to --kl-target")
    kw = {}
    if args.max_grad_norm is not None:
        kw["max_grad_norm"] = args.max_grad_norm
    if args.kl_stop is not None:
        kw["kl_stop"] = args.kl_stop
    if args.kl_target is not None:
        kw["kl_target"] = args.kl_target
        if args.kl_lr_bounds is not None:
            kw["kl_lr_bounds"] = tuple(args.kl_lr_bounds)
    if args.lr_schedule != "constant" and not args.torch_learner:
        kw["device_lr"] = True
    return kw


def control_on(args):
    return (args.max_grad_norm is not None or args.kl_stop is not None or args.kl_target is not None or args.lr_schedule != "constant")


def lr_mult(args, it):
    """--lr-schedule: the multiplier of --lr in iteration `it` (linear: the reference's max(1 - it / iters, 0))."""
    return max(1.0 - it / float(args.iters), 0.0) if args.lr_schedule == "linear" else 1.0


def control_record(learner):
    """What the log line gains when the control path is on; reads and clears the learner's counters (one sync per logged record)."""
    c = learner.control_stats()
    return {"grad_norm": round(c["grad_norm_mean"], 5), "grad_norm_max": round(c["grad_norm_max"], 5), "clipped": c["clipped"],
            "skipped_nonfinite": c["skipped_nonfinite"], "skipped_kl": c["skipped_kl"], "lr_mult": round(c["lr_mult"] * c["kl_lr_mult"], 6)}


def reward_shaping_arg(text):
    """--reward-shaping: "torque=1e-4,work=1e-3,failure=1,floor=0" -> the dict of env_spec.reward_shaping_spec (which validates it)."""
    from openroborl_amd import env_spec
    out = {}
    for item in text.split(","):
        key, sep, value = item.partition("=")
        try:
            out[key.strip()] = float(value)
        except ValueError:
            sep = ""
        if not sep:
            raise argparse.ArgumentTypeError("expected NAME=VALUE[,NAME=VALUE...] with the names %s, got %r" % (", ".join(env_spec.SHAPING_KEYS), item))
    try:
        env_spec.reward_shaping_spec(out)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return out


def shaping_ramp(args, env, it):
    """--reward-shaping-ramp: the weights' scale in iteration `it`, 0 -> 1 linearly over the first ITERS iterations; one setter call per
    iteration until it stands at 1.  The shaping kernel reads the weights in device memory: the captured rollout is not captured again."""
    if args.reward_shaping is not None and args.reward_shaping_ramp > 0 and it <= args.reward_shaping_ramp:
        env.set_reward_shaping(args.reward_shaping, scale=min(it / float(args.reward_shaping_ramp), 1.0))


def shaping_record(args, env, log_it):
    """--reward-shaping: {name: mean per step} over the episodes THIS rank finished since the totals were cleared (None without the flag
    or when the record is not logged), read and cleared where the episode log is."""
    if args.reward_shaping is None:
        return None
    out = {k: round(v, 6) for k, v in env.reward_shaping_stats().items()} if log_it else None
    env.clear_shaping_totals()
    return out


def obs_norm_check(args, world):
    """--obs-norm and its flags against the modes that have no normaliser; SystemExit with the reason."""
    if not args.obs_norm:
        if args.obs_norm_freeze_after is not None or args.save_folded:
            raise SystemExit("train.py: --obs-norm-freeze-after / --save-folded belong to --obs-norm")
        return
    if world > 1:
        raise SystemExit("train.py: --obs-norm runs on one rank: every rank would keep the statistics of its own shard and the replicas would "
                         "no longer be one policy (merging the records over ranks is not built)")
    if args.distill or args.history or args.history_ppo:
        raise SystemExit("train.py: --obs-norm belongs to PPO on a plain, privileged-critic or privileged-actor policy; the history and "
                         "distillation learners have no normaliser")
    if args.obs_norm_freeze_after is not None and args.obs_norm_freeze_after < 0:
        raise SystemExit("train.py: --obs-norm-freeze-after must not be negative")


def obs_norm_record(model):
    """What the log line gains with --obs-norm: the rows behind the statistics and the range of 1 / (sqrt(var) + eps) (one device read)."""
    rstd = model.obs_norm.rstd
    return {"obs_norm_count": model.obs_norm.count, "obs_rstd_min": round(float(rstd.min()), 4), "obs_rstd_max": round(float(rstd.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="imitation_learning_laikago")
    ap.add_argument("--num-robot", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--model-file", default="")
    ap.add_argument("--motion-file", action="append", default=None,
                    help="reference motion clip (repeatable; overrides the task YAML's motion_file): several = the clip set every reset "
                         "draws the episode's clip from (ImitationTask's ref_motion_filenames)")
    ap.add_argument("--clip-time", type=float, nargs=2, metavar=("MIN", "MAX"), default=None,
                    help="switch to a newly drawn clip of the set every U(MIN, MAX) seconds of motion time, mid-episode (ImitationTask's "
                         "clip_time_min / clip_time_max; overrides the task YAML's; default: never)")
    ap.add_argument("--clip-weights", type=float, nargs="+", metavar="W", default=None,
                    help="one weight per --motion-file: every reset and mid-episode switch draws clip k with probability W_k / sum W "
                         "(overrides the task YAML's clip_weights; default: uniform)")
    ap.add_argument("--clip-curriculum", type=clip_curriculum_arg, default=None, metavar="ALPHA,EPS[,METRIC]",
                    help="failure-adaptive clip sampling on the device: once per iteration the logged episodes' scores (METRIC: length, the "
                         "default, against the task's final episode step limit; return or step_reward against 1 per step) move a running "
                         "score per clip with weight ALPHA, and clip k is drawn with probability (1 - EPS) (1 - score_k) / sum + EPS / n.  "
                         "Logged records gain \"clip_prob\".  One rank")
    ap.add_argument("--perturb-init-state-prob", type=float, default=None,
                    help="probability that a reset starts the robot on a Gaussian-perturbed copy of the reference state (ImitationTask's "
                         "perturb_init_state_prob; overrides the task YAML's; default: 0)")
    ap.add_argument("--tar-obs-noise", type=float, default=None,
                    help="standard deviation (rad) of the noise on the heading the target observations are expressed in (ImitationTask's "
                         "tar_obs_noise[0]; overrides the task YAML's; default: none)")
    ap.add_argument("--sensor-noise", type=sensor_noise_arg, default=None, metavar="A,V,T,R,D",
                    help="standard deviations of the sensor noise: motor angle (rad), motor velocity, motor torque, base roll / pitch / yaw (rad) "
                         "and their rates (rad/s), the reference robot's _observation_noise_stdev; velocity and torque are accepted and have no "
                         "consumer (default: none)")
    ap.add_argument("--push", type=push_arg, default=None, metavar="PROB,LO,HI[,Z,ANG[,GRACE]]",
                    help="external pushes while training: probability of a velocity kick per robot and env step, its horizontal speed range "
                         "(m/s), optionally the vertical bound (m/s) and the angular bound per axis (rad/s), optionally the env steps at "
                         "the start of an episode without kicks; overrides the task YAML's `push` (default: none; never in --eval)")
    ap.add_argument("--reward-shaping", type=reward_shaping_arg, default=None, metavar="NAME=W[,NAME=W...]",
                    help="penalties taken off the imitation reward on the device, inside the captured rollout: weights for torque (mean square "
                         "torque over the motors, (N m)^2), work (J), action_rate, action_accel (squared first and second differences of the "
                         "actions), impact (sum of the legs' peak normal forces, N) and failure (1 at a fall, not at a time limit), and floor, "
                         "the smallest shaped reward (default: none).  Every learner trains on the shaped reward; the return columns stay the "
                         "imitation return, and every logged record gains \"shaping\": {name: mean per step} over the episodes THIS rank finished")
    ap.add_argument("--reward-shaping-ramp", type=int, default=0, metavar="ITERS",
                    help="--reward-shaping: scale the weights from 0 to 1 linearly over the first ITERS iterations (default: full weights from the start)")
    ap.add_argument("--reward-terms", action="store_true",
                    help="also output the five unweighted terms of the imitation reward on the device (pose, velocity, end effector, root pose, "
                         "root velocity): every logged record gains \"reward_terms\": {name: mean per step} over the episodes THIS rank finished "
                         "in the segment (rank-local, unlike the gathered episode means); --eval: over each robot's episode")
    ap.add_argument("--contact-outputs", action="store_true",
                    help="also output the foot contact impulses on the device: every logged record gains \"gait\": {\"duty\": [4], \"normal_force\": [4]} "
                         "(per leg: stance steps / steps, mean normal force in N) over the episodes THIS rank finished in the segment (rank-local); "
                         "--eval: over each robot's episode")
    ap.add_argument("--privileged-critic", action="store_true",
                    help="asymmetric actor-critic: the value net also reads the simulator's privileged observation (env.privileged_obs: true base "
                         "twist and gravity direction, the episode's randomised parameters, foot contacts and forces, the step's push), the actor "
                         "keeps the 160 observation words.  Binds the contact outputs, and the push outputs with --push.  --save then writes the "
                         "full critic under the usual names (model/vf_fc0/w:0 with 208 rows): the actor part is what the reference can load, "
                         "--eval of such a zip works here")
    ap.add_argument("--privileged-actor", action="store_true",
                    help="a teacher policy: the actor reads the privileged observation as well (implies --privileged-critic; model/pi_fc0/w:0 "
                         "with 208 rows too), trained with PPO.  --save writes a zip that loads here (--eval, --distill) and not in the "
                         "reference; --distill turns it into a deployable 160-input policy")
    ap.add_argument("--distill", default="", metavar="TEACHER.zip",
                    help="train a plain student by distillation instead of PPO (DAgger): every segment is collected with the student's actions "
                         "and labelled with the teacher's mean on (observation, privileged observation), then regressed on for --epochs "
                         "(learner_hip.FusedDistill; --torch-learner: ppo.Distill).  The log carries distill_loss; --save writes a plain "
                         "[160, 512] actor.  One rank")
    ap.add_argument("--history", action="store_true",
                    help="--distill: the student keeps the teacher's actor and critic and gains an encoder over the last 16 steps of its own "
                         "sensors (IMU, last action, motor angles: 512 words), trained to estimate the privileged observation from them "
                         "(learner_hip.FusedDistillHistory; --torch-learner: ppo.DistillHistory).  The log carries latent_loss; --save writes "
                         "the teacher's variables + model/enc_*, a zip that loads here (--eval) and not in the reference")
    ap.add_argument("--history-ppo", action="store_true",
                    help="PPO on a history policy (RMA's third phase, or one-stage training): the actor reads its observation and the encoder's "
                         "estimate from the last 16 steps of its own sensors, the critic reads the simulator's TRUE privileged observation, and "
                         "actor, critic and encoder all train (learner_hip.FusedPPOHistory; --torch-learner: ppo.PPOHistory).  --model-file: a "
                         "history student's zip is fine-tuned, a teacher's zip (--privileged-actor) gets a fresh encoder, none: fresh weights.  "
                         "The environment is --privileged-actor's.  The log carries latent_loss; --save writes a history zip that --eval runs")
    ap.add_argument("--latent-coef", type=float, default=0.0, metavar="C",
                    help="--history-ppo: weight of the auxiliary estimation loss, the squared error of the encoder's output against the "
                         "privileged observation (default 0: the encoder is trained by the PPO gradient through the actor alone)")
    ap.add_argument("--distill-action-coef", type=float, default=0.0, metavar="C",
                    help="--distill --history: weight of the action loss, the squared error of the student's actor output on (observation, "
                         "encoder output) against the teacher's mean, its gradient flowing through the frozen actor into the encoder "
                         "(orr_history_student_head).  The log then carries action_loss next to latent_loss.  Default 0: the latent regression alone")
    ap.add_argument("--distill-latent-coef", type=float, default=1.0, metavar="C",
                    help="--distill --history: weight of the latent regression (default 1)")
    ap.add_argument("--distill-beta", type=float, default=0.0,
                    help="--distill: the share of robots that are stepped with the teacher's action instead of the student's (default 0)")
    ap.add_argument("--distill-beta-iters", type=int, default=0, help="--distill: decay --distill-beta linearly to 0 over this many iterations (0: constant)")
    ap.add_argument("--learn-std", action="store_true",
                    help="train a state-independent log-std of the twelve actions with PPO (model/pi/logstd:0, on the device) instead of "
                         "sampling with a fixed std.  The log gains entropy, approx_kl, clip_fraction and the smallest and largest std; "
                         "--save writes the variable behind the reference's list: a zip that loads here and not in the reference")
    ap.add_argument("--ent-coef", type=float, default=0.0, metavar="C", help="--learn-std: weight of the entropy bonus, loss - C * H (default 0)")
    ap.add_argument("--init-std", type=float, default=0.125, metavar="S",
                    help="the std of the action noise; with --learn-std where log-std starts (default 0.125, the reference's pi_init_std)")
    ap.add_argument("--log-std-bounds", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="--learn-std: log-std is clamped to [LO, HI] after every optimiser step (default log 0.01, log 1)")
    ap.add_argument("--obs-norm", action="store_true",
                    help="running mean / std normalisation of the network inputs (the 160 observation words; with --privileged-critic / "
                         "--privileged-actor the 48 privileged ones too), on the device: the statistics are frozen from the start of a rollout to "
                         "the end of its update, then the segment is merged into them (one pass) and folded into the packed layer 0 of the fused "
                         "forward pass, which runs on raw observations as before.  One extra segment before the first iteration seeds them.  "
                         "The log gains obs_norm_count, obs_rstd_min, obs_rstd_max; --save writes the statistics next to the weights (loads here: "
                         "--eval, --model-file).  One rank")
    ap.add_argument("--obs-norm-freeze-after", type=int, default=None, metavar="ITERS", help="--obs-norm: no update of the statistics after this many iterations")
    ap.add_argument("--save-folded", default="", metavar="PATH",
                    help="--obs-norm: also write a zip WITHOUT statistics whose layer-0 matrices and biases carry the normaliser: the same "
                         "function on raw observations; for a plain policy a zip the reference's run.py loads")
    control_args(ap)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default="")
    ap.add_argument("--save", default="", help="write the trained weights as a stable-baselines style zip (with --privileged-critic: see there)")
    ap.add_argument("--torch-policy", action="store_true", help="rollout policy through plain torch instead of the fused HIP kernel")
    ap.add_argument("--torch-learner", action="store_true",
                    help="PPO update through autograd + torch.optim.Adam (ppo.PPO, the fp32 reference) instead of the hand-written backward "
                         "replayed as a hipGraph (learner_hip.FusedPPO)")
    ap.add_argument("--eval", default="", help="evaluate a policy zip instead of training: deterministic actions, test mode "
                                                 "(no randomiser, full-length episodes), like `run.py --mode test`")
    ap.add_argument("--legacy-gae-index", action="store_true",
                    help="reproduce the reference's neighbouring-robot episode-start index in the GAE recursion (ppo_imitation.py:88); "
                         "only for curve-by-curve comparisons with the reference at num_robot > 1")
    ap.add_argument("--mpi-adam", action="store_true",
                    help="the reference's MpiAdam arithmetic (stable_baselines/common/mpi_adam.py:53-58: epsilon outside the bias correction, i.e. "
                         "NOT scaled by sqrt(1 - beta2^t)) instead of torch.optim.Adam's; with adam_epsilon 1e-5 (run.py:118) the reference's "
                         "effective epsilon is ~30x larger in the first steps.  Default off: the recorded training runs used torch's form")
    ap.add_argument("--sync-check-every", type=int, default=100, help="replica consistency check (MpiAdam.check_synced, mpi_adam.py:47-48: every 100 updates)")
    ap.add_argument("--tune-gemms", action="store_true", help="let PyTorch's TunableOp pick the learner's GEMM kernels (graph-replayed learner: 16.8 -> 16.3 ms per iteration after ~3 s of tuning)")
    args = ap.parse_args()

    import torch
    from openroborl_amd import dist as odist, policy as pol, ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv

    if args.tune_gemms:
        torch.cuda.tunable.enable(True)
    if args.eval:
        return evaluate(args, torch, pol, ppo, VecQuadrupedEnv)
    if args.history_ppo and (args.distill or args.history or args.privileged_critic or args.privileged_actor):
        raise SystemExit("train.py: --history-ppo is a mode of its own; not with --distill / --history / --privileged-critic / --privileged-actor")
    if args.latent_coef != 0.0 and not args.history_ppo:
        raise SystemExit("train.py: --latent-coef belongs to --history-ppo")
    if not args.latent_coef >= 0.0:
        raise SystemExit("train.py: --latent-coef must not be negative")
    args.privileged_critic = args.privileged_critic or args.privileged_actor
    if args.distill and (args.privileged_critic or args.torch_policy):
        raise SystemExit("train.py: --distill trains a plain student with the fused rollout; not with --privileged-critic / --privileged-actor / --torch-policy")
    if args.history and not args.distill:
        raise SystemExit("train.py: --history belongs to --distill (PPO on a history policy is --history-ppo)")
    if (args.distill_action_coef != 0.0 or args.distill_latent_coef != 1.0) and not args.history:
        raise SystemExit("train.py: --distill-action-coef / --distill-latent-coef belong to --distill --history")
    if args.distill_action_coef < 0.0 or args.distill_latent_coef < 0.0:
        raise SystemExit("train.py: --distill-action-coef / --distill-latent-coef must not be negative")
    if args.learn_std and args.distill:
        raise SystemExit("train.py: --learn-std belongs to PPO; the distillation learners neither read nor train a log-std")
    if (args.ent_coef != 0.0 or args.log_std_bounds is not None) and not args.learn_std:
        raise SystemExit("train.py: --ent-coef / --log-std-bounds belong to --learn-std")
    if args.reward_shaping_ramp and args.reward_shaping is None:
        raise SystemExit("train.py: --reward-shaping-ramp belongs to --reward-shaping")
    if args.reward_shaping_ramp < 0:
        raise SystemExit("train.py: --reward-shaping-ramp must not be negative")
    privileged = args.privileged_critic or bool(args.distill) or args.history_ppo       # somebody reads env.privileged_obs
    rank, world, local = odist.init_from_env()
    obs_norm_check(args, world)
    if args.clip_curriculum is not None and world > 1:
        raise SystemExit("train.py: --clip-curriculum runs on one rank: each rank would adapt to its own episodes and the shards would no "
                         "longer draw what one env draws (merging the statistics over ranks is not built)")
    if args.distill and world > 1:
        raise SystemExit("train.py: --distill runs on one rank")
    # ORR_BENCH_SINGLE_DEVICE=1 (+ ORR_DIST_BACKEND=gloo): several ranks rehearsed on a one-GPU box (tests), never a measurement
    dev = torch.device("cuda", 0 if os.environ.get("ORR_BENCH_SINGLE_DEVICE") else local)
    torch.cuda.set_device(dev)
    env = VecQuadrupedEnv(task_name=args.task, num_robot=args.num_robot, mode="train", auto_reset=True, seed=args.seed,
                          device=dev, num_procs=world, robot_index_offset=rank * args.num_robot, motion_file=args.motion_file,
                          perturb_init_state_prob=args.perturb_init_state_prob, tar_obs_noise=args.tar_obs_noise,
                          reward_terms=args.reward_terms, contact_outputs=args.contact_outputs or privileged,
                          observation_noise_stdev=args.sensor_noise, push=args.push,
                          push_outputs=privileged and args.push is not None, reward_shaping=args.reward_shaping,
                          **clip_time_kwargs(args), **clip_draw_kwargs(args))     # (bound here, before the rollout graph is captured)
    if args.clip_curriculum is not None and not env.multi_clip:
        raise SystemExit("train.py: --clip-curriculum needs several --motion-file")
    if args.history:
        return distill(args, torch, pol, ppo, rollout, odist, env, history_student(args, torch, pol, ppo, dev), dev)
    params = pol.load_parameters(args.model_file) if args.model_file else None     # run.py:220-221
    if args.history_ppo and params is not None and "model/enc_fc0/w:0" not in params:
        # a teacher's zip: its nets + a fresh encoder (the rule of --distill --history); the log-std, if any, is the teacher's
        model = history_student(args, torch, pol, ppo, dev, path=args.model_file, fused=False, std=args.init_std, learn_std=args.learn_std)
    else:
        # same seed -> identical replicas.  (--model-file: the critic's width is the file's)
        wide = args.privileged_actor or args.history_ppo
        model = ppo.ActorCritic(dev, params=params, seed=args.seed, priv_dim=pol.PRIV_DIM if args.privileged_critic or wide else 0,
                                actor_priv_dim=pol.PRIV_DIM if wide else 0, std=args.init_std, learn_std=args.learn_std,
                                history=ppo.HISTORY_STEPS if args.history_ppo else 0, obs_norm=args.obs_norm)
    if (model.obs_norm is not None) != args.obs_norm:
        raise SystemExit("train.py: --model-file has %s, --obs-norm says otherwise" % ("a normaliser's statistics" if model.obs_norm is not None else "no statistics"))
    if model.learn_std != args.learn_std and not args.distill:
        raise SystemExit("train.py: --model-file has %s, --learn-std says otherwise" % ("a learned log-std" if model.learn_std else "no log-std"))
    if args.history_ppo:
        return history_ppo(args, torch, pol, ppo, rollout, odist, env, model, dev, rank, world)
    if bool(model.priv_dim) != args.privileged_critic:
        raise SystemExit("train.py: --model-file has a %s critic, --privileged-critic says otherwise" % ("privileged" if model.priv_dim else "plain"))
    if bool(model.actor_priv_dim) != args.privileged_actor:
        raise SystemExit("train.py: --model-file has a %s actor, --privileged-actor says otherwise" % ("privileged" if model.actor_priv_dim else "plain"))
    if not args.torch_policy:
        model.enable_fused()
    if args.distill:
        return distill(args, torch, pol, ppo, rollout, odist, env, model, dev)
    # --learn-std: the entropy bonus and the clamp; without it no keyword at all, the learners' defaults
    entropy = dict(ent_coef=args.ent_coef, log_std_bounds=tuple(args.log_std_bounds or ppo.LOG_STD_BOUNDS)) if args.learn_std else {}
    if args.torch_learner:
        learner = ppo.PPO(model, lr=args.lr, minibatch=args.minibatch, **entropy, **control_kwargs(args))
    else:
        from openroborl_amd import learner_hip
        # equal minibatches only (static buffers of the graph-replayed update): the largest size <= --minibatch that divides the
        # segment, e.g. --num-robot 1000 x horizon 32 = 32000 samples run as 2 x 16000 instead of failing on 16384
        mb = learner_hip.FusedPPO.fit_minibatch(args.num_robot * args.horizon, args.minibatch)
        if mb != min(args.minibatch, args.num_robot * args.horizon) and rank == 0:
            print("train.py: minibatch %d -> %d (must divide the %d samples of a segment)" % (args.minibatch, mb, args.num_robot * args.horizon),
                  file=sys.stderr)
        if mb < 256 and args.num_robot * args.horizon >= 4096:
            raise SystemExit("train.py: %d samples per segment have no divisor between 256 and %d; pick another --num-robot / --horizon "
                             "or use --torch-learner (handles a short last minibatch)" % (args.num_robot * args.horizon, args.minibatch))
        learner = learner_hip.FusedPPO(model, lr=args.lr, minibatch=mb, mpi_adam_epsilon=args.mpi_adam, **entropy, **control_kwargs(args))
        learner.sync()                                        # MpiAdam.sync before training (ppo_imitation.py:274)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed * 1000 + rank)
    obs = env.reset()
    t0 = time.time()
    samples = 0
    log = []
    first_starts = None                   # episode_starts of a segment's first step = the last step's done flags of the previous segment
    priv = None                           # --privileged-critic: the privileged observation that belongs to `obs` (None: right after the reset)
    # static rollout buffers + the segment replayed as one hipGraph (fused policy only); --torch-policy keeps the eager collector
    collector = None if args.torch_policy else rollout.GraphRollout(env, model, args.horizon)

    def merge_segment(buf):
        """--obs-norm: the segment into the statistics, and the fold into the fused layer 0 at the next refresh; after the update, never before"""
        T, n = buf["rewards"].shape
        model.update_obs_norm(buf["obs"].reshape(T * n, -1), *((buf["priv"].reshape(T * n, -1),) if model.priv_norm is not None else ()))
        model.mark_updated()
    if args.obs_norm and model.obs_norm.count == 0:
        # one segment whose only use is to seed the statistics: the policy never acts, and the learner never learns, on the identity
        buf = (collector.collect(obs, generator=gen, priv=priv) if collector
               else rollout.collect_rollout(env, model, args.horizon, obs=obs, generator=gen, priv=priv))
        obs, priv, first_starts = buf["last_obs"], buf.get("last_priv"), buf["dones"][-1].clone()
        merge_segment(buf)
        odist.gather_env_episodes(env, args.horizon)       # its episodes are not the first iteration's
    for it in range(args.iters):
        shaping_ramp(args, env, it)
        buf = (collector.collect(obs, generator=gen, priv=priv) if collector
               else rollout.collect_rollout(env, model, args.horizon, obs=obs, generator=gen, priv=priv))
        obs = buf["last_obs"]
        priv = buf.get("last_priv")
        with torch.no_grad():
            boot = model.value(obs, priv)
        # bootstrap with the critic at the segment end (the reference uses 0 there, imitation_runners.py:98-100;
        # with 32-step segments that bias would dominate)
        adv, ret = rollout.gae_fused(buf["rewards"], buf["vpred"], buf["dones"], 0.95, 0.95, bootstrap=boot, normalize=True, eps=1e-8,
                                     legacy_gae_index=args.legacy_gae_index, first_starts=first_starts)
        first_starts = buf["dones"][-1].clone()               # the collector's buffers are overwritten by the next segment
        T, n = buf["rewards"].shape
        if args.lr_schedule != "constant":
            learner.set_lr_mult(lr_mult(args, it))
        losses = learner.update(buf["obs"].reshape(T * n, -1), buf["actions"].reshape(T * n, -1), adv.reshape(-1),
                                ret.reshape(-1), old_logp=buf["logp"].reshape(-1) if "logp" in buf else None,
                                epochs=args.epochs, generator=gen, priv=buf["priv"].reshape(T * n, -1) if model.priv_dim else None)
        surr, vf = losses[0], losses[1]      # --learn-std: three more, ppo.STAT_NAMES
        if args.obs_norm and (args.obs_norm_freeze_after is None or it < args.obs_norm_freeze_after):
            merge_segment(buf)
        samples += T * n * world
        # (> 1 rank, or ORR_FORCE_DIST=1: the one-rank rehearsal of the several-ranks path on RCCL runs the check too)
        if (world > 1 or os.environ.get("ORR_FORCE_DIST", "0") == "1") and args.sync_check_every > 0 and it % args.sync_check_every == args.sync_check_every - 1 and hasattr(learner, "check_synced"):
            learner.check_synced()                            # like MpiAdam every 100 updates (mpi_adam.py:47-48)
        log_it = rank == 0 and (it % 10 == 0 or it == args.iters - 1)
        # this rank's episodes of the segment by clip (read before the gather below clears the log)
        by_clip = env.episode_returns_by_clip() if log_it and env.multi_clip else None
        by_term = env.episode_reward_terms() if log_it and args.reward_terms else None     # likewise; rank-local
        gait = env.episode_gait() if log_it and args.contact_outputs else None             # likewise
        shaping = shaping_record(args, env, log_it)                                        # likewise, and cleared where the log is
        if args.clip_curriculum is not None:
            env.clip_curriculum_update()                       # one launch on the log as it stands, before the gather clears it; no sync
        stats = odist.gather_env_episodes(env, args.horizon)   # means come from the exact per-rank sums, not the truncated list
        if log_it:
            rec = {"iter": it, "samples": samples, "sec": round(time.time() - t0, 2),
                   "mean_step_reward": round(float(buf["rewards"].mean()), 4),
                   "ep_len_mean": round(stats.mean_length, 1), "ep_ret_mean": round(stats.mean_return, 2),
                   "episodes": stats.sums[0], "episodes_unlogged": stats[3] - max(stats.sums[0] - int(stats[0].numel()), 0),
                   "max_ep_steps": int(env.field_int("MAX_EP_STEPS").max()), "surr": round(float(surr), 4), "vf": round(float(vf), 4)}
            if args.learn_std:           # the twelve stds: one device read per logged record
                std = model.std
                rec.update({k: round(float(v), 6) for k, v in zip(ppo.STAT_NAMES[2:], losses[2:])})
                rec.update({"std_min": round(float(std.min()), 5), "std_max": round(float(std.max()), 5)})
            if control_on(args):
                rec.update(control_record(learner))
            if args.obs_norm:
                rec.update(obs_norm_record(model))
            if by_clip is not None:
                rec["ep_ret_mean_by_clip"] = {clip_name(env, c): round(r, 2) for c, (r, _) in sorted(by_clip.items())}
            if args.clip_curriculum is not None or args.clip_weights is not None:
                rec["clip_prob"] = clip_prob_record(env)
            if by_term is not None:
                rec["reward_terms"] = {k: round(v, 4) for k, v in by_term.items()}
            if gait is not None:
                rec["gait"] = {k: [round(x, 3) for x in v] for k, v in gait.items()}
            if shaping is not None:
                rec["shaping"] = shaping
            log.append(rec)
            print(json.dumps(rec), flush=True)
    if rank == 0 and args.save:
        pol.save_parameters_zip(args.save, model.state_dict())
    if rank == 0 and args.save_folded:
        pol.save_folded(args.save_folded, model.state_dict())
    if rank == 0 and args.log:
        with open(args.log, "w") as f:
            json.dump(log, f, indent=1)
    env.close()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def history_student(args, torch, pol, ppo, dev, path=None, fused=True, **model_kw):
    """--distill TEACHER.zip --history: the teacher's parameters + a fresh encoder (seeded by --seed), on the fused path.  --history-ppo with a
    teacher's --model-file (`path`): the same rule, the model's std arguments in model_kw."""
    params = pol.load_parameters(path or args.distill)
    if any(k.startswith(pol.NORM_PREFIXES) for k in params):
        # the teacher's layer 0 expects normalised inputs, and a history policy has no normaliser: copying its weights would run them on raw
        # observations and on the encoder's raw estimate, without a word
        raise SystemExit("train.py: %s is a teacher trained with --obs-norm; a history policy with an observation normaliser is not built "
                         "(the encoder's frames are a subset of the observation): train the teacher without --obs-norm"
                         % (path or args.distill))
    if np.shape(params["model/pi_fc0/w:0"])[0] != 160 + pol.PRIV_DIM:
        raise SystemExit("train.py: %s needs a teacher with a privileged actor (--privileged-actor)" % ("--history-ppo --model-file" if path else "--history"))
    student = ppo.ActorCritic(dev, seed=args.seed, priv_dim=pol.PRIV_DIM, actor_priv_dim=pol.PRIV_DIM, history=ppo.HISTORY_STEPS, **model_kw)
    with torch.no_grad():
        for k, v in params.items():
            if k.startswith("model/enc_"):
                continue                     # a history student as the teacher: its actor and critic, a fresh encoder all the same
            if k in student.p:
                student.p[k].copy_(torch.as_tensor(v))
            else:
                student.extra[k] = np.asarray(v, dtype=np.float32).copy()
    return student.enable_fused() if fused else student


def history_ppo(args, torch, pol, ppo, rollout, odist, env, model, dev, rank, world):
    """--history-ppo: PPO on a history policy.  The collector hands hist[k] to the actor and priv[k], the true row, to the critic
    (critic_priv=True), the bootstrap is the critic on the last true row, and the learner trains actor, critic and encoder."""
    if not model.history:
        raise SystemExit("train.py: --history-ppo could not make a history policy of --model-file")
    if not args.torch_policy:
        model.enable_fused()
    B = args.num_robot * args.horizon
    entropy = dict(ent_coef=args.ent_coef, log_std_bounds=tuple(args.log_std_bounds or ppo.LOG_STD_BOUNDS)) if args.learn_std else {}
    if args.torch_learner:
        learner = ppo.PPOHistory(model, lr=args.lr, minibatch=args.minibatch, latent_coef=args.latent_coef, **entropy, **control_kwargs(args))
    else:
        from openroborl_amd import learner_hip
        mb = learner_hip.FusedPPOHistory.fit_minibatch(B, args.minibatch)
        if mb < 256 and B >= 4096:
            raise SystemExit("train.py: %d samples per segment have no divisor between 256 and %d; pick another --num-robot / --horizon "
                             "or use --torch-learner (handles a short last minibatch)" % (B, args.minibatch))
        learner = learner_hip.FusedPPOHistory(model, lr=args.lr, minibatch=mb, mpi_adam_epsilon=args.mpi_adam, latent_coef=args.latent_coef, **entropy,
                                              **control_kwargs(args))
        learner.sync()
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed * 1000 + rank)
    collector = None if args.torch_policy else rollout.GraphRollout(env, model, args.horizon, critic_priv=True)
    obs, priv, hist, first_starts = env.reset(), None, None, None
    t0, samples, log = time.time(), 0, []
    for it in range(args.iters):
        shaping_ramp(args, env, it)
        buf = (collector.collect(obs, generator=gen, priv=priv, hist=hist) if collector
               else rollout.collect_rollout(env, model, args.horizon, obs=obs, generator=gen, priv=priv, hist=hist, critic_priv=True))
        obs, priv, hist = buf["last_obs"], buf["last_priv"], buf["last_hist"]
        with torch.no_grad():
            boot = model.value(obs, priv)
        adv, ret = rollout.gae_fused(buf["rewards"], buf["vpred"], buf["dones"], 0.95, 0.95, bootstrap=boot, normalize=True, eps=1e-8,
                                     legacy_gae_index=args.legacy_gae_index, first_starts=first_starts)
        first_starts = buf["dones"][-1].clone()
        if args.lr_schedule != "constant":
            learner.set_lr_mult(lr_mult(args, it))
        losses = learner.update(buf["obs"].reshape(B, -1), buf["hist"].reshape(B, -1), buf["priv"].reshape(B, -1), buf["actions"].reshape(B, -1),
                                adv.reshape(-1), ret.reshape(-1), old_logp=buf["logp"].reshape(-1) if "logp" in buf else None,
                                epochs=args.epochs, generator=gen)
        samples += B * world
        if (world > 1 or os.environ.get("ORR_FORCE_DIST", "0") == "1") and args.sync_check_every > 0 and it % args.sync_check_every == args.sync_check_every - 1 and hasattr(learner, "check_synced"):
            learner.check_synced()
        if args.clip_curriculum is not None:
            env.clip_curriculum_update()
        shaping = shaping_record(args, env, rank == 0 and (it % 10 == 0 or it == args.iters - 1))
        stats = odist.gather_env_episodes(env, args.horizon)
        if rank == 0 and (it % 10 == 0 or it == args.iters - 1):
            rec = {"iter": it, "samples": samples, "sec": round(time.time() - t0, 2), "mean_step_reward": round(float(buf["rewards"].mean()), 4),
                   "ep_len_mean": round(stats.mean_length, 1), "ep_ret_mean": round(stats.mean_return, 2), "episodes": stats.sums[0],
                   "surr": round(float(losses[0]), 4), "vf": round(float(losses[1]), 4), "latent_loss": round(float(losses[-1]), 6)}
            if args.learn_std:
                std = model.std
                rec.update({k: round(float(v), 6) for k, v in zip(ppo.STAT_NAMES[2:], losses[2:5])})
                rec.update({"std_min": round(float(std.min()), 5), "std_max": round(float(std.max()), 5)})
            if control_on(args):
                rec.update(control_record(learner))
            if shaping is not None:
                rec["shaping"] = shaping
            log.append(rec)
            print(json.dumps(rec), flush=True)
    if rank == 0 and args.save:
        pol.save_parameters_zip(args.save, model.state_dict())
    if rank == 0 and args.log:
        with open(args.log, "w") as f:
            json.dump(log, f, indent=1)
    env.close()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def distill(args, torch, pol, ppo, rollout, odist, env, student, dev):
    """--distill TEACHER.zip: DAgger on the device.  Each iteration collects a segment in which the student drives (all robots but the
    share --distill-beta, which the teacher drives) and the teacher labels every visited state, then regresses the student's mean on the labels.
    --history: the student reads its sensor history, and its encoder's output is regressed on the segment's privileged observations instead."""
    teacher_params = {k: v for k, v in pol.load_parameters(args.distill).items() if not k.startswith("model/enc_")}
    teacher = ppo.ActorCritic(dev, params=teacher_params).enable_fused()
    B = args.num_robot * args.horizon
    loss_name = "latent_loss" if args.history else "distill_loss"
    coefs = dict(action_coef=args.distill_action_coef, latent_coef=args.distill_latent_coef) if args.history else {}
    with_actions = args.history and (args.distill_action_coef != 0.0 or args.distill_latent_coef != 1.0)      # the log carries both losses
    if args.torch_learner:
        learner = (ppo.DistillHistory if args.history else ppo.Distill)(student, lr=args.lr, minibatch=args.minibatch, **coefs,
                                                                        **control_kwargs(args, kl=False))
    else:
        from openroborl_amd import learner_hip
        cls = learner_hip.FusedDistillHistory if args.history else learner_hip.FusedDistill
        learner = cls(student, lr=args.lr, minibatch=cls.fit_minibatch(B, args.minibatch), **coefs, **control_kwargs(args, kl=False))
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed * 1000)
    collector = rollout.GraphRollout(env, student, args.horizon, teacher=teacher)
    obs, priv, hist = env.reset(), None, None
    t0, samples, log = time.time(), 0, []
    for it in range(args.iters):
        beta = args.distill_beta * (max(0.0, 1.0 - it / float(args.distill_beta_iters)) if args.distill_beta_iters > 0 else 1.0)
        driven = int(round(beta * args.num_robot))
        shaping_ramp(args, env, it)
        collector.teacher_mask.zero_()
        collector.teacher_mask[:driven] = 1
        buf = collector.collect(obs, generator=gen, priv=priv, hist=hist)
        obs, priv, hist = buf["last_obs"], buf["last_priv"], buf.get("last_hist")
        if args.lr_schedule != "constant":
            learner.set_lr_mult(lr_mult(args, it))
        if args.history and args.distill_action_coef > 0.0:
            loss = learner.update(buf["hist"].reshape(B, -1), buf["priv"].reshape(B, -1), epochs=args.epochs, generator=gen,
                                  obs=buf["obs"].reshape(B, -1), target_mean=buf["teacher_mean"].reshape(B, 12))
        elif args.history:
            loss = learner.update(buf["hist"].reshape(B, -1), buf["priv"].reshape(B, -1), epochs=args.epochs, generator=gen)
        else:
            loss = learner.update(buf["obs"].reshape(B, -1), buf["teacher_mean"].reshape(B, 12), epochs=args.epochs, generator=gen)
        samples += B
        if args.clip_curriculum is not None:
            env.clip_curriculum_update()
        shaping = shaping_record(args, env, it % 10 == 0 or it == args.iters - 1)
        stats = odist.gather_env_episodes(env, args.horizon)
        if it % 10 == 0 or it == args.iters - 1:
            rec = {"iter": it, "samples": samples, "sec": round(time.time() - t0, 2), "mean_step_reward": round(float(buf["rewards"].mean()), 4),
                   "ep_len_mean": round(stats.mean_length, 1), "ep_ret_mean": round(stats.mean_return, 2), "episodes": stats.sums[0],
                   loss_name: round(float(loss), 6), "teacher_driven": driven}
            if with_actions:             # loss_name then holds the latent regression's own loss, as it does without the action loss
                rec.update({"latent_loss": round(learner.last_latent_loss, 6), "action_loss": round(learner.last_action_loss, 6),
                            "total_loss": round(float(loss), 6)})
            if control_on(args):
                rec.update(control_record(learner))
            if shaping is not None:
                rec["shaping"] = shaping
            log.append(rec)
            print(json.dumps(rec), flush=True)
    if args.save:
        pol.save_parameters_zip(args.save, student.state_dict())
    if args.log:
        with open(args.log, "w") as f:
            json.dump(log, f, indent=1)
    env.close()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def sensor_noise_arg(text):
    """--sensor-noise a,v,t,r,d -> five floats (validated by the env: openroborl_amd.env.sensor_noise_spec)."""
    parts = text.split(",")
    if len(parts) != 5:
        raise argparse.ArgumentTypeError("five comma-separated numbers: motor angle, motor velocity, motor torque, base rpy, base rpy rate")
    try:
        return [float(x) for x in parts]
    except ValueError:
        raise argparse.ArgumentTypeError("not a number in %r" % (text,))


def push_arg(text):
    """--push prob,lo,hi[,z,ang[,grace]] -> the env's push dict (validated by the env: openroborl_amd.env.push_spec)."""
    parts = text.split(",")
    if len(parts) not in (3, 5, 6):
        raise argparse.ArgumentTypeError("prob,lo,hi or prob,lo,hi,z,ang or prob,lo,hi,z,ang,grace")
    try:
        v = [float(x) for x in parts[:5]]
        push = dict(prob=v[0], lin_vel=(v[1], v[2]))
        if len(parts) >= 5:
            push.update(lin_vel_z=v[3], ang_vel=v[4])
        if len(parts) == 6:
            push["grace_steps"] = int(parts[5])
    except ValueError:
        raise argparse.ArgumentTypeError("not a number in %r" % (text,))
    return push


def clip_curriculum_arg(s):
    """ALPHA,EPS[,METRIC] -> the env's clip_curriculum dict; the refs are the env's defaults (env_spec.clip_curriculum_spec)."""
    parts = s.split(",")
    if len(parts) not in (2, 3):
        raise argparse.ArgumentTypeError("expected ALPHA,EPS[,METRIC], got %r" % (s,))
    try:
        cur = {"alpha": float(parts[0]), "eps": float(parts[1])}
    except ValueError:
        raise argparse.ArgumentTypeError("expected ALPHA,EPS[,METRIC] with two numbers, got %r" % (s,))
    cur["metric"] = parts[2] if len(parts) == 3 else "length"
    if cur["metric"] not in ("length", "return", "step_reward"):
        raise argparse.ArgumentTypeError("METRIC is length, return or step_reward, not %r" % (cur["metric"],))
    return cur


def clip_draw_kwargs(args):
    """--clip-weights / --clip-curriculum -> the env's clip_weights / clip_curriculum (nothing given: the task YAML's weights, no
    curriculum)."""
    kw = {}
    if args.clip_weights is not None:
        kw["clip_weights"] = list(args.clip_weights)
    if args.clip_curriculum is not None:
        kw["clip_curriculum"] = dict(args.clip_curriculum)
    return kw


def clip_prob_record(env):
    """{clip name: probability} of the clip draws as the device holds them (one sync; logged iterations only)."""
    out = {}
    for name, p in env.clip_probabilities().items():
        for c, x in zip(env.clip_sets[name], p):
            out[clip_name(env, c)] = round(float(x), 6)
    return out


def clip_time_kwargs(args):
    """--clip-time MIN MAX -> the env's clip_time_min / clip_time_max (nothing given: the task YAML's, else no switching)."""
    return {} if args.clip_time is None else dict(clip_time_min=args.clip_time[0], clip_time_max=args.clip_time[1])


def clip_name(env, clip_id):
    """'<id>:<file name>' of a clip of the env (ids keep a file listed twice apart)."""
    return "%d:%s" % (clip_id, os.path.splitext(os.path.basename(env.clips[clip_id].path))[0])


def evaluate(args, torch, pol, ppo, VecQuadrupedEnv):
    """run.py:151-183 (test): one full episode per robot with the policy mean; prints return / length statistics."""
    dev = torch.device("cuda", 0)
    n = min(args.num_robot, 1024)
    env = VecQuadrupedEnv(task_name=args.task, num_robot=n, mode="test", auto_reset=False, seed=args.seed, device=dev,
                          motion_file=args.motion_file, reward_terms=args.reward_terms, contact_outputs=args.contact_outputs,
                          observation_noise_stdev=args.sensor_noise, **clip_time_kwargs(args))
    model = ppo.ActorCritic(dev, params=pol.load_parameters(args.eval))
    if not args.torch_policy:
        model.enable_fused()
    if model.actor_priv_dim and not model.history and not args.contact_outputs:
        env.bind_contact_outputs(True)           # a teacher's actor reads the contact words of the row, as it did in training
    obs = env.reset()
    # a zip with a privileged critic (--privileged-critic): the fused forward pass takes the privileged observation; only the actor's output is used
    # here.  A teacher's zip (--privileged-actor): the row goes to the actor every step.  A student's zip (--distill) is a plain policy.
    # A history student's zip (--distill --history): no row at all; its sensor history is kept in place, one push per step
    priv = env.privileged_obs(done=None) if model.priv_dim and not model.history else None
    hist = None
    if model.history:
        from openroborl_amd import policy_hip
        hist = policy_hip.history_push(obs, None, None, torch.empty((n, ppo.HISTORY_DIM), device=dev))
    clip_ids = env.active_clip_ids()             # the clip each robot's episode plays
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    ret = torch.zeros(n, device=dev)
    length = torch.zeros(n, device=dev)
    term_sum = torch.zeros(len(env.TERM_NAMES), dtype=torch.float64, device=dev)      # --reward-terms: over every robot's steps up to its first done
    stance = torch.zeros(4, dtype=torch.float64, device=dev)       # --contact-outputs: per leg, likewise
    normal = torch.zeros(4, dtype=torch.float64, device=dev)
    limit = int(env.field_int("MAX_EP_STEPS").max())
    for _ in range(limit):
        act, _, _ = model.act(obs, priv, deterministic=True, hist=hist)
        obs, rew, done, _ = env.step(act)
        if priv is not None:
            env.privileged_obs(out=priv, done=done)
        if hist is not None:
            policy_hip.history_push(obs, done, hist, hist)
        ret += rew * alive
        if args.reward_terms:
            term_sum += (env.reward_terms * alive[:, None]).sum(0)
        if args.contact_outputs:
            stance += (env.foot_contact() & alive[:, None]).sum(0).double()
            normal += (env.contact_out.view(n, 4, 4)[:, :, 0] * alive[:, None]).sum(0).double()
        length += alive.float()
        alive &= ~done.bool()
        if not bool(alive.any()):
            break
    rec = {"policy": args.eval, "task": args.task, "robots": n, "episode_limit": limit,
           "return_mean": round(float(ret.mean()), 2), "return_min": round(float(ret.min()), 2),
           "length_mean": round(float(length.mean()), 1), "full_length_fraction": round(float((length >= limit).float().mean()), 3),
           "reward_per_step": round(float((ret / length).mean()), 3)}
    if env.multi_clip:       # finish rate (full-length episodes) and robots per clip
        full = (length >= limit).cpu().numpy()
        cid = clip_ids.cpu().numpy()
        rec["full_length_fraction_by_clip"] = {clip_name(env, int(c)): round(float(full[cid == c].mean()), 3) for c in np.unique(cid)}
        rec["robots_by_clip"] = {clip_name(env, int(c)): int((cid == c).sum()) for c in np.unique(cid)}
    if args.reward_terms:
        rec["reward_terms"] = {k: round(float(v), 4) for k, v in zip(env.TERM_NAMES, (term_sum / length.sum()).tolist())}
    if args.contact_outputs:
        steps = float(length.sum())
        rec["gait"] = {"duty": [round(x / steps, 3) for x in stance.tolist()],
                       "normal_force": [round(x / (steps * env.env_time_step), 3) for x in normal.tolist()]}
    print(json.dumps(rec))
    env.close()


if __name__ == "__main__":
    main()
