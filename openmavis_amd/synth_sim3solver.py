"""Seeded synthetic jobs for Sim3Solver (src/Sim3Solver.cc): per job a planted similarity S12 between the camera frames
of two keyframes of different maps, N correspondences of which a chosen share are inliers (camera-2 points carried by
S12 into camera 1, plus 3-D noise of about half a pixel at their depth) and the rest gross outliers (an unrelated point
in front of camera 1).  World positions come from the camera-frame points through random keyframe poses, so the
constructor's Riw Xw + tiw has real work to do; octaves 0-7 per side give thresholds 9.210 * sigma2 whose truncation
to an integer matters; index1 is a sorted subset of 0 .. mN1-1 with mN1 > N (holes: unmatched / bad map points).

make_jobs(ns, ...) returns a list of job dicts (the layout of tests/sim3_ref.py and openmavis_amd.sim3solver) with the
truth added: R12, t12, s12, inlier [N]."""
import numpy as np

from . import synth
from .synth_sim3 import _rot

PINHOLE = np.array([380.0, 380.0, 360.0, 270.0, 0, 0, 0, 0], np.float32)
WIDTH, HEIGHT = 720, 540


def level_sigma2(nlevels=8, scale_factor=1.2):
    """mvLevelSigma2 as ORBextractor builds it: float mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor, squared."""
    sf = [np.float32(1.0)]
    for _ in range(1, nlevels):
        sf.append(np.float32(np.float64(sf[-1]) * scale_factor))
    return np.array([s * s for s in sf], np.float32)


def _camera(model):
    if model == 1:
        return PINHOLE.copy()
    return synth.hilti_rig(1)[0][0].astype(np.float32)


def _rays(model, cam, rng, n):
    u, v = rng.uniform(40, WIDTH - 40, n), rng.uniform(40, HEIGHT - 40, n)
    return synth.pinhole_unproject(cam[:4], u, v) if model == 1 else synth.kb8_unproject(cam, u, v)


def _pose12(rng):
    T = synth.random_pose(rng)
    return T[:12].astype(np.float32)   # Rcw row-major, tcw


def make_job(n, seed, inlier_share=0.6, model1=0, model2=0, fix_scale=False, holes=0.3):
    rng = np.random.Generator(np.random.PCG64(seed))
    cam1, cam2 = _camera(model1), _camera(model2)
    R12 = _rot(rng, 0.3)
    s12 = 1.0 if fix_scale else rng.uniform(0.7, 1.4)
    t12 = rng.uniform(-0.5, 0.5, 3)
    depth = rng.uniform(2.0, 15.0, n)
    X2 = _rays(model2, cam2, rng, n) * depth[:, None]
    X1 = s12 * X2 @ R12.T + t12
    X1 += rng.normal(0, 1, (n, 3)) * (np.linalg.norm(X1, axis=1) * 0.5 / float(cam1[0]))[:, None]
    inlier = rng.random(n) < inlier_share
    if n >= 3:
        inlier[rng.choice(n, 3, replace=False)] = True
    n_out = int((~inlier).sum())
    X1[~inlier] = _rays(model1, cam1, rng, n_out) * rng.uniform(2.0, 15.0, n_out)[:, None]
    pose1, pose2 = _pose12(rng), _pose12(rng)
    Xw = []
    for X, p in ((X1, pose1), (X2, pose2)):
        R, t = p[:9].reshape(3, 3).astype(np.float64), p[9:].astype(np.float64)
        Xw.append(((X - t) @ R).astype(np.float32))   # Rwc (X - tcw)
    mn1 = n + max(1, int(round(holes * n))) if holes > 0 else n
    index1 = np.sort(rng.choice(mn1, n, replace=False)).astype(np.int32)
    s2 = level_sigma2()
    return dict(Xw1=Xw[0], Xw2=Xw[1], sigma2_1=s2[rng.integers(0, 8, n)], sigma2_2=s2[rng.integers(0, 8, n)],
                index1=index1, mN1=int(mn1), pose1=pose1, pose2=pose2, cam1=cam1, cam2=cam2, model1=int(model1),
                model2=int(model2), fix_scale=bool(fix_scale), R12=R12, t12=t12, s12=float(s12), inlier=inlier)


def make_jobs(ns, seed=1, inlier_share=0.6, models=(0, 0), fix_scale=False, holes=0.3):
    """One job per entry of `ns` (ragged N), seeds seed, seed + 1, ...; models = (model1, model2) for every job or a list
    of such pairs."""
    pairs = [models] * len(ns) if isinstance(models[0], int) else list(models)
    return [make_job(n, seed + j, inlier_share, pairs[j][0], pairs[j][1], fix_scale, holes) for j, n in enumerate(ns)]
