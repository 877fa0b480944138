"""What tests/test_actuator_cpu.py and tests/test_gpu_actuator.py share: a sub-step driver in Python on top of the CPU oracle's probes
(step_robot's loop, oracle/orr_oracle.c, with MotorModel's torque clip added: the oracle itself has no torque limit), the reduction of its
per-sub-step torques and motor rates to the layout of act_dev / act_ep_dev, and the floor rule of tests/contact_lib.py per column.

The driver starts from a pre-step record and the step's filtered target (the record's ACTION, XHIST, YHIST and LAST_ACTION after the
oracle's own orc_step on a copy) and repeats action_repeat times: orc_ctrl_obs_probe, map_pi + lerp + the +-max_angle_change clip, the PD
law with the record's STRENGTH, the clip to the limits, orc_physics_substep, orc_receive_obs_probe.  The model values go through
oracle_lib.dec32 as the oracle's own do.  Without limits it reproduces orc_step's rigid state, LAMBDA and trace torques exactly
(tests/test_actuator_cpu.py)."""
import ctypes as C

import numpy as np

from tests import contact_lib as cl
from tests import oracle_lib as ol
from tests.gpu_kit import MIXED

LEG_LIMITS = np.array([20.0, 30.0, 40.0] * 4)            # abduction / hip / knee of each leg, motor order, N m
F32_SHARE, DEVICE_SHARE = cl.F32_SHARE, cl.DEVICE_SHARE   # shares of the motor steps that may lie over the cell bound
ULP = cl.ULP
COLUMNS = ("S1", "PK", "S2", "W")
RIGID = ("POS", "QUAT", "LINVEL", "ANGVEL", "Q", "QD")
TWO_PI = 2.0 * 3.14159265358979323846


def limits_of(robot_type, per_type=None):
    """[n, 12] limits: LEG_LIMITS for every robot, or {type id: [12]} (+inf where a type is missing)"""
    robot_type = np.asarray(robot_type)
    out = np.full((len(robot_type), 12), np.inf)
    for i, t in enumerate(robot_type):
        out[i] = LEG_LIMITS if per_type is None else per_type.get(int(t), np.full(12, np.inf))
    return out


def mixed_limits():
    """the torque_limits keyword that gives every robot of a MIXED batch LEG_LIMITS"""
    return {name: [float(x) for x in LEG_LIMITS] for name in MIXED}


def map_pi(a):
    """orc_map_pi elementwise, in a's own number format"""
    dt = a.dtype.type
    m = np.fmod(a, dt(TWO_PI))
    pi = dt(TWO_PI / 2)
    return np.where(m >= pi, m - dt(TWO_PI), np.where(m < -pi, m + dt(TWO_PI), m)).astype(dt)


class SubstepDriver(object):
    """An OracleEnv (float64, or the float32 parity build) driven sub-step by sub-step from Python"""

    def __init__(self, cfg, models, clips, n, robot_type, clip_id, f32=False):
        self.orc = ol.OracleEnv(cfg, models, clips, n, robot_type=robot_type, clip_id=clip_id, f32="parity" if f32 else False)
        L, dt = self.orc.L, self.orc.dt
        rp = C.POINTER(C.c_float if f32 else C.c_double)
        L.orc_physics_substep.restype = C.c_int
        L.orc_physics_substep.argtypes = [C.c_void_p, rp, rp]
        L.orc_ctrl_obs_probe.argtypes = [C.c_void_p, rp, rp]
        L.orc_receive_obs_probe.argtypes = [C.c_void_p, rp]
        self.n, self.rep, self.dt, self.lay, self.rp = n, int(cfg.action_repeat), dt, self.orc.lay, rp
        robot_type = np.broadcast_to(np.asarray(robot_type, dtype=np.int32), (n,))
        tab = {}
        for t in set(int(x) for x in robot_type):
            m = models[t]
            tab[t] = {k: ol.dec32(m[k]).astype(dt) for k in ("kp", "kd", "motor_offset", "motor_dir")}
            tab[t]["jom"] = np.asarray(m["joint_of_motor"], dtype=np.int64)
        self.kp, self.kd, self.off, self.dir = (np.stack([tab[int(t)][k] for t in robot_type]) for k in ("kp", "kd", "motor_offset", "motor_dir"))
        self.jom = np.stack([tab[int(t)]["jom"] for t in robot_type])
        self.mac = dt(ol.dec32(cfg.max_angle_change))

    def step_from(self, state64, counters, act, limits=None):
        """One env step of every robot from the given records (float64 layout) and counters.  limits: [n, 12] N m or None.  -> dict:
        tau, qd [n, action_repeat, 12] (motor order; the torque that went into the physics and the motor rate after each sub-step), raw
        (the strength-scaled PD torque before the clip),
        qm [n, action_repeat + 1, 12] (the motor angle before the first and after every sub-step), rigid [n, 37] and lam [n, 12] after
        the last sub-step, orc = the record after the oracle's own, unlimited orc_step - all in the build's number format."""
        o, lay, dt, n, rep = self.orc, self.lay, self.dt, self.n, self.rep
        pre = np.ascontiguousarray(state64.astype(dt))
        o.state[:] = pre
        o.counters[:] = counters
        o.step(act)
        post = o.state.copy()
        o.counters[:] = counters
        W = pre.copy()
        for name in ("LAST_ACTION", "XHIST", "YHIST", "ACTION"):
            W[:, lay.sl(name)] = post[:, lay.sl(name)]
        lim = None if limits is None else np.asarray(limits, dtype=np.float64).astype(dt)
        Q, QD = lay.sl("Q").start, lay.sl("QD").start
        rows = np.arange(n)[:, None]
        strength, target = W[:, lay.sl("STRENGTH")].copy(), W[:, lay.sl("ACTION")].copy()
        sac, fv, sc = lay.sl("STATE_ACTION_COUNTER").start, lay.sl("FILTER_VALID").start, lay.sl("STEP_COUNTER").start
        co, tau_in = np.zeros((n, 19), dtype=dt), np.zeros((n, 12), dtype=dt)
        pW, pco, ptau = self.row_pointers(W), self.row_pointers(co), self.row_pointers(tau_in)      # one pointer object per row, made once
        h, probe, substep, receive = o.h, o.L.orc_ctrl_obs_probe, o.L.orc_physics_substep, o.L.orc_receive_obs_probe
        taus, qds, qms = np.zeros((n, rep, 12), dtype=dt), np.zeros((n, rep, 12), dtype=dt), np.zeros((n, rep + 1, 12), dtype=dt)
        raws = np.zeros((n, rep, 12), dtype=dt)
        qms[:, 0] = (W[rows, Q + self.jom] - self.off) * self.dir
        for sub in range(rep):
            lerp = dt(sub + 1) / dt(rep)
            for i in range(n):
                probe(h, pW[i], pco[i])
            cur = map_pi(co[:, :12])
            prev = np.where(W[:, fv:fv + 1] != 0, W[:, lay.sl("FILTER_ACTION")], cur)
            cmd = prev + lerp * (target - prev)
            lo, hi = cur - self.mac, cur + self.mac
            cmd = np.where(cmd < lo, lo, np.where(cmd > hi, hi, cmd))
            qm = (W[rows, Q + self.jom] - self.off) * self.dir
            qdm = W[rows, QD + self.jom] * self.dir
            tau = -1 * (self.kp * (qm - cmd)) - self.kd * (qdm - dt(0.0)) + dt(0.0)      # orc_motor_torque
            tau = strength * tau
            raws[:, sub] = tau
            if lim is not None:                                                          # minitaur_motor.py:166-171: strength first, then the clip
                tau = np.where(tau > lim, lim, np.where(tau < -lim, -lim, tau))
            assert tau.dtype == dt
            tau_in[:] = tau
            W[:, sac] += 1
            if sub == rep - 1:
                W[:, lay.sl("FILTER_ACTION")] = target
                W[:, fv] = 1
                W[:, sc] += 1
            for i in range(n):
                substep(h, pW[i], ptau[i])
                receive(h, pW[i])
            taus[:, sub] = tau
            qds[:, sub] = W[rows, QD + self.jom] * self.dir
            qms[:, sub + 1] = (W[rows, Q + self.jom] - self.off) * self.dir
        return {"tau": taus, "raw": raws, "qd": qds, "qm": qms, "rigid": rigid_of(lay, W), "lam": W[:, lay.sl("LAMBDA")].copy(), "orc": post}

    def row_pointers(self, a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == self.dt
        return [C.cast(a.ctypes.data + i * a.strides[0], self.rp) for i in range(a.shape[0])]

    def close(self):
        self.orc.close()


def rigid_of(lay, st):
    """[n, 37]: POS QUAT LINVEL ANGVEL Q QD of records [n, stride]"""
    return np.concatenate([st[:, lay.sl(k)] for k in RIGID], axis=1)


def reduce_substeps(tau, qd, sim_dt):
    """tau, qd [n, action_repeat, 12] -> [n, 12, 4] in act_dev's layout: sum tau, max |tau|, sum tau^2, sim_dt sum tau qd, added in
    sub-step order from 0 in the inputs' own number format, the work scaled once at the end (the device's order)"""
    tau, qd = np.asarray(tau), np.asarray(qd)
    dt = tau.dtype.type
    out = np.zeros((tau.shape[0], 12, 4), dtype=tau.dtype)
    for s in range(tau.shape[1]):
        out[:, :, 0] = out[:, :, 0] + tau[:, s]
        out[:, :, 1] = np.maximum(out[:, :, 1], np.abs(tau[:, s]))
        out[:, :, 2] = out[:, :, 2] + tau[:, s] * tau[:, s]
        out[:, :, 3] = out[:, :, 3] + tau[:, s] * qd[:, s]
    out[:, :, 3] = out[:, :, 3] * dt(sim_dt)
    return out


def episode_row(step_rows, limits):
    """step_rows [steps, n, 12, 4] of one episode, limits [n, 12] -> [n, 4] in act_ep_dev's layout, float64: the work and the sum of
    squares over steps and motors, the largest |tau|, the number of steps in which some motor's peak equalled its limit"""
    r = np.asarray(step_rows, dtype=np.float64)
    sat = (r[..., 1] == np.asarray(limits, dtype=np.float64)[None]).any(axis=-1)
    return np.stack([r[..., 3].sum(axis=(0, 2)), r[..., 2].sum(axis=(0, 2)), r[..., 1].max(axis=(0, 2)), sat.sum(axis=0).astype(np.float64)], axis=1)


def floor_rule(ref, f32, dev=None):
    """contact_lib.floor_rule's rule for one column: ref, f32 (, dev) [...] cells of the float64 reference, of the float32 parity build
    and of the device, every step started from the same record; every cell is live.  q = the 99th percentile of |f32 - ref|; cell bound
    = 4 q + 2^-22 max(1, |ref|).  -> dict: q, cells, the share of cells over the bound for f32 and for dev, the bound array, dev's
    worst cell"""
    ref, f32 = np.asarray(ref, dtype=np.float64), np.asarray(f32, dtype=np.float64)
    q = float(np.percentile(np.abs(f32 - ref), 99))
    bound = 4.0 * q + ULP * np.maximum(1.0, np.abs(ref))
    out = {"q": q, "cells": int(ref.size), "bound": bound, "top": float(np.abs(ref).max()),
           "f32_share": float((np.abs(f32 - ref) > bound).sum()) / ref.size}
    if dev is not None:
        err = np.abs(np.asarray(dev, dtype=np.float64) - ref)
        out["dev_share"] = float((err > bound).sum()) / ref.size
        k = np.unravel_index(np.argmax(err), err.shape)
        out["dev_worst"] = (float(err[k]), float(ref[k]), tuple(int(x) for x in k))
    return out


def describe(r):
    s = "q99 %.3e | cells %d | largest |ref| %.4g | float32 oracle over the bound %.3f %%" % (r["q"], r["cells"], r["top"], 100 * r["f32_share"])
    if "dev_share" in r:
        s += " | device over the bound %.3f %%, worst cell |d| %.3e at ref %.5g %s" % ((100 * r["dev_share"],) + r["dev_worst"])
    return s
