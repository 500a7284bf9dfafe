"""Seeded synthetic jobs for Optimizer::InertialOptimization (openmavis_amd/inertial_init.py, tests/inertial_ref.py).

A smooth body trajectory in a gravity-aligned frame (an arc with a pitch wobble and a vertical oscillation), seen from a
map whose world frame is rotated by a planted Rwg (gravity direction) and, for a mono job, shrunk by a planted scale;
IMU samples of the exact specific force / angular rate plus white noise and planted constant biases; keyframe poses with
small noise.  The records are preintegrated on the CPU by the preintegration restatement of oracle/oracle.py
(oracle.preintegrate), so nothing here needs a GPU.

make_job(K, seed, mode, mono, priorG, priorA, breaks=(), isolated=()) returns the job dict of
inertial_init.InertialOptimizer / tests/inertial_ref.py:
    Rwb [K][9], twb [K][3], vel [K][3] float64; old_bg [K][3] float32; kf1, kf2 [E] int32; preint [E][292] float32;
    bg0, ba0 [3], Rwg [9], scale float64; mode, mono; priorG, priorA float32
plus the planted truth (truth_*), the IMU samples (meas, start, bias: a synth_imu-style batch) and the calibration.
breaks: keyframes that are "bad" (the edge into them is not built: the chain splits there); isolated: keyframes with
no edge at all.  shuffle: the keyframes (and edges) in a random order."""
import os
import sys

import numpy as np

from . import imu
from .inertial_init import FULL, BIAS, GS, initial_guess

GRAV = float(np.float32(9.81))


def _oracle():
    try:
        import oracle
    except ImportError:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        import oracle
    return oracle


def _traj(t, ph):
    """(R [n][3][3], p, v [n][3]) of the body in the gravity-aligned frame at times t."""
    t = np.asarray(t, np.float64)
    yaw, pitch = 0.8 * t + ph[0], 0.08 * np.sin(1.3 * t + ph[1])
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    z, o = np.zeros_like(t), np.ones_like(t)
    Rz = np.stack([cy, -sy, z, sy, cy, z, z, z, o], -1).reshape(-1, 3, 3)
    Ry = np.stack([cp, z, sp, z, o, z, -sp, z, cp], -1).reshape(-1, 3, 3)
    r = 1.0 / 0.8
    p = np.stack([r * np.sin(yaw), r * (1 - np.cos(yaw)), 0.5 * np.sin(2.5 * t + ph[2])], -1)
    v = np.stack([np.cos(yaw), np.sin(yaw), 1.25 * np.cos(2.5 * t + ph[2])], -1)
    return Rz @ Ry, p, v


def _log(R):
    w = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1) / 2
    th = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    s = np.sin(th)
    return np.where((th < 1e-12)[:, None], w, w * (th / np.where(s == 0, 1, s))[:, None])


def _exp(w):
    d = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if d < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + W * np.sin(d) / d + W @ W * (1 - np.cos(d)) / (d * d)


def make_job(K, seed, mode=FULL, mono=False, priorG=1e2, priorA=1e5, breaks=(), isolated=(), shuffle=False, freq=100.0,
             scale_true=1.1, bias_true=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    h = 1.0 / freq
    n_steps = rng.integers(8, 17, size=max(K - 1, 0))
    kf_t = np.concatenate([[0.0], np.cumsum(n_steps * h)]) + float(rng.uniform(0, 5))
    ph = rng.uniform(0, 2 * np.pi, 3)
    if bias_true is None:
        bg_t = rng.normal(0, 1.0, 3)
        bg_t *= rng.uniform(0.02, 0.03) / np.linalg.norm(bg_t)
        ba_t = rng.normal(0, 0.05, 3)
    else:
        bg_t, ba_t = np.asarray(bias_true[0], np.float64), np.asarray(bias_true[1], np.float64)
    Rwg_t = _exp(rng.normal(0, 0.4, 3) * np.array([1, 1, 0]))
    if mode == BIAS:   # a map that is already gravity-aligned (the overload fixes Rwg = I, scale = 1)
        Rwg_t = np.eye(3)
    s_t = float(scale_true) if mono and mode != BIAS else 1.0
    # the bias the records are integrated with (the keyframes' current estimate)
    if mode == FULL:
        bias0 = np.zeros(6, np.float32)
    else:
        bias0 = np.concatenate([ba_t + rng.normal(0, 5e-3, 3), bg_t + rng.normal(0, 2e-3, 3)]).astype(np.float32)
    cal = imu.Calib(1.7e-4, 2.0e-3, 1.9e-5, 3.0e-3, freq)
    noise_g, noise_a = 1.7e-4 * np.sqrt(freq), 2.0e-3 * np.sqrt(freq)
    # edges: keyframe k - 1 -> k for every k that is not bad and not next to an isolated keyframe
    drop = set(int(b) for b in breaks) | set(int(i) for i in isolated) | set(int(i) + 1 for i in isolated)
    kf2 = np.array([k for k in range(1, K) if k not in drop], np.int32)
    kf1 = kf2 - 1
    meas, start = [], [0]
    for k in kf2:
        t = kf_t[k - 1] + h * np.arange(n_steps[k - 1] + 1)
        R, _, v = _traj(t, ph)
        w = _log(np.swapaxes(R[:-1], 1, 2) @ R[1:]) / h
        a = np.einsum("nji,nj->ni", R[:-1], (v[1:] - v[:-1]) / h + np.array([0, 0, GRAV]))
        n = len(w)
        m = np.concatenate([a + ba_t + rng.normal(0, noise_a, (n, 3)), w + bg_t + rng.normal(0, noise_g, (n, 3)),
                            np.full((n, 1), h)], 1)
        meas.append(m)
        start.append(start[-1] + n)
    E = len(kf2)
    batch = dict(meas=np.concatenate(meas).astype(np.float32) if E else np.zeros((0, 7), np.float32),
                 start=np.array(start, np.int32), bias=np.tile(bias0, (E, 1)).astype(np.float32))
    if E:
        rec, _ = _oracle().preintegrate(batch, cal.Cov, cal.CovWalk)
    else:
        rec = np.zeros((0, imu.PREINT_FLOATS), np.float32)
    R, p, v = _traj(kf_t, ph)
    Rn = np.stack([_exp(rng.normal(0, 5e-5, 3)) for _ in range(K)]) if K else np.zeros((0, 3, 3))
    Rwb = Rwg_t.T @ R @ Rn                      # the map's world: gravity = Rwg_t (0, 0, -G)
    twb = (p @ Rwg_t) / s_t + rng.normal(0, 5e-5, (K, 3))
    vel_t = (v @ Rwg_t) / s_t
    # the keyframes' old gyro bias: the records' own, or (about half) one near the planted bias: both flag values
    old_bg = np.tile(bias0[3:], (K, 1)).astype(np.float32)
    near = rng.uniform(0, 1, K) < 0.5
    old_bg[near] = (bg_t + rng.normal(0, 3e-4, (int(near.sum()), 3))).astype(np.float32)
    job = dict(Rwb=Rwb.reshape(K, 9), twb=twb, old_bg=old_bg, kf1=kf1, kf2=kf2, preint=rec,
               bg0=bias0[3:].astype(np.float64), ba0=bias0[:3].astype(np.float64), mode=int(mode), mono=int(bool(mono)),
               priorG=np.float32(priorG), priorA=np.float32(priorA), truth_bg=bg_t, truth_ba=ba_t, truth_Rwg=Rwg_t.T,
               truth_scale=s_t, truth_vel=vel_t, meas=batch["meas"], start=batch["start"], bias=batch["bias"], calib=cal)
    g = initial_guess(job)
    job["vel"] = g["vel"]
    if mode == FULL:
        job["Rwg"], job["scale"] = g["Rwg"].reshape(9), 1.0
    else:   # a map that is already initialised: a start near the truth (GS); BIAS does not read Rwg and scale
        job["Rwg"] = (Rwg_t.T @ _exp(rng.normal(0, 0.02, 3) * np.array([1, 1, 0]))).reshape(9)
        job["scale"] = s_t * float(np.exp(rng.normal(0, 0.03)))
        job["vel"] = (vel_t + rng.normal(0, 2e-3, (K, 3))).astype(np.float32).astype(np.float64)
    if shuffle and K > 1:
        perm = rng.permutation(K)          # new index of keyframe k is inv[k]
        inv = np.empty(K, np.int64)
        inv[perm] = np.arange(K)
        for key in ("Rwb", "twb", "old_bg", "vel", "truth_vel"):
            job[key] = np.ascontiguousarray(np.asarray(job[key])[perm])
        eo = rng.permutation(E)
        job["kf1"], job["kf2"] = inv[kf1[eo]].astype(np.int32), inv[kf2[eo]].astype(np.int32)
        job["preint"] = np.ascontiguousarray(rec[eo])
        job["edge_perm"] = eo
    return job


def make_jobs(Ks, seed=1, modes=(FULL,), monos=(False,), priors=((1e2, 1e5),), **kw):
    """One job per entry of Ks, the other settings cycled."""
    return [make_job(int(K), seed + 17 * i, modes[i % len(modes)], monos[i % len(monos)], *priors[i % len(priors)], **kw)
            for i, K in enumerate(Ks)]
