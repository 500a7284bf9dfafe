"""Seeded synthetic jobs for Optimizer::OptimizeSim3 (src/Optimizer.cc:2460-2726), built on synth_sim3solver.make_job:
a planted similarity S12 between the camera frames of two keyframes, N matched map-point pairs of which a share are
gross outliers (an unrelated point in front of camera 1), keypoints = the projections of the camera-frame points plus
0.7 px of noise on both sides, octaves 0-7 per side (mvInvLevelSigma2), and a start value that is the planted similarity
disturbed like a RANSAC result (a few hundredths of a radian, of a unit and of the scale).  Options: a share of entries
without a KF2 keypoint (i2 < 0 under bAllPoints: obs2 is then the projection of P3D2c and the level the map point's
track level) and a share of points behind camera 2 (P3D2c.z < 0: no edge, the match stays).

make_job(n, ...) returns the job dict of openmavis_amd.optimizer.Sim3Optimizer / tests/optsim3_ref.py with the truth
added: R12, t12, s12, inlier [N] (false for the gross outliers), behind [N]."""
import numpy as np

from . import synth, synth_sim3solver as ss
from .synth_ba import cam_project
from .synth_sim3 import _rot


def _cam_frame(pose, Xw):
    p = np.asarray(pose, np.float64)
    return np.asarray(Xw, np.float64) @ p[:9].reshape(3, 3).T + p[9:]


def make_job(n, seed, outlier_share=0.2, model1=0, model2=0, fix_scale=False, no_kp2_share=0.0, behind_share=0.0,
             th2=10.0, noise_px=0.7):
    base = ss.make_job(n, seed, 1.0 - outlier_share, model1, model2, fix_scale)
    rng = np.random.Generator(np.random.PCG64(seed + 7919))
    Xw1, Xw2 = base["Xw1"].copy(), base["Xw2"].copy()
    behind = rng.random(n) < behind_share
    if behind.any():   # the camera-2 point mirrored through the camera centre: z < 0
        p2 = base["pose2"].astype(np.float64)
        Xc = -_cam_frame(p2, Xw2[behind])
        Xw2[behind] = ((Xc - p2[9:]) @ p2[:9].reshape(3, 3)).astype(np.float32)
    with np.errstate(all="ignore"):
        obs1 = cam_project(base["cam1"].astype(np.float64), _cam_frame(base["pose1"], Xw1), model1 == 1)
        obs2 = cam_project(base["cam2"].astype(np.float64), _cam_frame(base["pose2"], Xw2), model2 == 1)
    obs1, obs2 = obs1 + rng.normal(0, noise_px, (n, 2)), obs2 + rng.normal(0, noise_px, (n, 2))
    has_kp2 = ~(rng.random(n) < no_kp2_share)
    obs2[~has_kp2] = 0.0   # ignored: the optimiser projects P3D2c
    inv2 = (np.float32(1.0) / ss.level_sigma2()).astype(np.float32)
    dR = _rot(rng, 0.02)
    s0 = 1.0 if fix_scale else base["s12"] * (1.0 + rng.normal(0, 0.01))
    return dict(index1=base["index1"], mN1=base["mN1"], Xw1=Xw1, Xw2=Xw2, obs1=obs1.astype(np.float32),
                inv_sigma2_1=inv2[rng.integers(0, 8, n)], has_kp2=has_kp2, obs2=obs2.astype(np.float32),
                inv_sigma2_2=inv2[rng.integers(0, 8, n)], pose1=base["pose1"], pose2=base["pose2"], cam1=base["cam1"],
                cam2=base["cam2"], model1=int(model1), model2=int(model2), fix_scale=bool(fix_scale),
                th2=np.float32(th2), q=synth.quat_from_R(dR @ base["R12"]), t=base["t12"] + rng.normal(0, 0.02, 3),
                s=float(s0), R12=base["R12"], t12=base["t12"], s12=base["s12"], inlier=base["inlier"] & ~behind,
                behind=behind)


def make_jobs(ns, seed=1, models=(0, 0), fix_scale=False, **kw):
    """One job per entry of `ns` (ragged N), seeds seed, seed + 1, ...; models = (model1, model2) for every job or a list
    of such pairs; fix_scale one value or one per job."""
    pairs = [models] * len(ns) if isinstance(models[0], int) else list(models)
    fix = [fix_scale] * len(ns) if isinstance(fix_scale, (bool, int)) else list(fix_scale)
    return [make_job(n, seed + j, model1=pairs[j][0], model2=pairs[j][1], fix_scale=fix[j], **kw)
            for j, n in enumerate(ns)]
