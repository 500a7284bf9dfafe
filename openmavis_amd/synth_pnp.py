"""Seeded synthetic jobs for MLPnPsolver (src/MLPnPsolver.cpp): per job a planted camera pose Tcw, N map points seen by
a KannalaBrandt8 or Pinhole camera, Gaussian pixel noise and a chosen share of gross outliers (an unrelated pixel).
Scenes: "general" (points at depth U(depth) m along random pixel rays), "centred" (the same with the world origin at the
centre of the cloud, the well-conditioned choice), "planar" (world z = 0 exactly, so that the planarity matrix has an
exact zero row and FullPivHouseholderQR reports rank 2; close to the camera, because the planar branch's translation
scale as the reference writes it is off by a factor that its Gauss-Newton corrects only within the 5.0 step bound), "rank1" (every world point a multiple
of one direction: rank 1, the 12-column branch; the pose is then not observable) and "identity" (general, Tcw = I:
rot2rodrigues gives w == 0 where the linear stage returns the identity to the last bit).  Octaves 0-7 give the
thresholds sigma2 * th2; index is a sorted subset of 0 .. mN-1 with mN > N (holes: entries without a map point).

make_jobs(ns, ...) returns job dicts (the layout of tests/mlpnp_ref.py and openmavis_amd.pnpsolver) with the truth
added: Rcw, tcw, inlier [N]."""
import numpy as np

from . import synth
from .synth_sim3 import _rot
from .synth_sim3solver import HEIGHT, PINHOLE, WIDTH, level_sigma2


def camera(model):
    return PINHOLE.copy() if model == 1 else synth.hilti_rig(1)[0][0].astype(np.float32)


def project(model, k, X):
    """GeometricCamera::project for [n][3] points in float64."""
    k, X = np.asarray(k, np.float64), np.asarray(X, np.float64)
    if model == 1:
        return np.stack([k[0] * X[:, 0] / X[:, 2] + k[2], k[1] * X[:, 1] / X[:, 2] + k[3]], 1)
    th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
    psi = np.arctan2(X[:, 1], X[:, 0])
    r = th + k[4] * th ** 3 + k[5] * th ** 5 + k[6] * th ** 7 + k[7] * th ** 9
    return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def make_job(n, seed, model=0, scene="general", noise_px=0.5, outlier_share=0.0, holes=0.3, depth=(2.0, 15.0)):
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = camera(model)
    if scene == "identity":
        R, t = np.eye(3), np.zeros(3)
    else:
        R, t = _rot(rng, 0.6), rng.uniform(-1.0, 1.0, 3)
    if scene == "planar":
        Xw = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1)
        t = 0.3 * t + np.array([0.0, 0.0, 2.5])
    elif scene == "rank1":
        d = np.array([0.12, -0.2, 1.0]) / np.linalg.norm([0.12, -0.2, 1.0])
        Xw = rng.uniform(3.0, 12.0, n)[:, None] * d[None, :]
        R, t = _rot(rng, 0.2), rng.uniform(-0.3, 0.3, 3)
    else:
        u, v = rng.uniform(40, WIDTH - 40, n), rng.uniform(40, HEIGHT - 40, n)
        ray = synth.pinhole_unproject(cam[:4], u, v) if model == 1 else synth.kb8_unproject(cam, u, v)
        Xc = ray * rng.uniform(depth[0], depth[1], n)[:, None]
        if scene == "centred":
            t = Xc.mean(0) + 0.1 * t
        Xw = (Xc - t) @ R        # Rwc (Xc - tcw)
    Xw = Xw.astype(np.float32)
    P = project(model, cam, Xw.astype(np.float64) @ R.T + t)
    P = P + rng.normal(0, noise_px, P.shape) if noise_px > 0 else P
    inlier = rng.random(n) >= outlier_share
    if n >= 6:
        inlier[rng.choice(n, 6, replace=False)] = True
    n_out = int((~inlier).sum())
    P[~inlier] = np.stack([rng.uniform(20, WIDTH - 20, n_out), rng.uniform(20, HEIGHT - 20, n_out)], 1)
    mn = n + max(1, int(round(holes * n))) if holes > 0 else n
    index = np.sort(rng.choice(mn, n, replace=False)).astype(np.int32)
    octave = rng.integers(0, 8, n)
    return dict(P2D=P.astype(np.float32), sigma2=level_sigma2()[octave], octave=octave.astype(np.int32), Xw=Xw,
                index=index, mN=int(mn), cam=cam, model=int(model), Rcw=R, tcw=t, inlier=inlier, scene=scene)


def make_jobs(ns, seed=1, models=0, scenes="general", noise_px=0.5, outlier_share=0.0, holes=0.3, depth=(2.0, 15.0)):
    """One job per entry of `ns` (ragged N), seeds seed, seed + 1, ...; models / scenes: one value or one per job."""
    ms = [models] * len(ns) if isinstance(models, int) else list(models)
    sc = [scenes] * len(ns) if isinstance(scenes, str) else list(scenes)
    return [make_job(n, seed + j, ms[j], sc[j], noise_px, outlier_share, holes, depth) for j, n in enumerate(ns)]
