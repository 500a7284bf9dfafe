"""Seeded synthetic windows for the visual bundle adjustment (Optimizer::LocalBundleAdjustment's graph).

Keyframes on synth_ba's trajectory with its Hilti rig; the state is camera 0's Tcw as (q (x y z w), t) and the constant
transforms camera c <- camera 0 (mTrl / mTsll / mTsrl).  The first `n_opt` keyframes (newest first) are optimisable, the
rest fixed.  Each point is seen from `views` consecutive keyframes in up to two cameras each; observations are the exact
projection + N(0, obs_noise); a fraction of camera 0's observations become stereo observations (u, v, u_R) of
g2o::EdgeStereoSE3ProjectXYZ's pinhole.  Options plant what the outlier test has to find: gross outliers, and KannalaBrandt8
edges on points slightly behind their camera (theta > 90 deg) whose observation is the exact projection, so that only the
depth flags them.  Points seen from fixed keyframes only and points without edges exercise the solver's corners.
"""
import numpy as np

from . import synth_ba

CAM_KB8, CAM_PINHOLE = 0, 1


def q_from_R(R):
    """Unit quaternion (x y z w), w >= 0, of a rotation matrix."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    q = q if q[3] >= 0 else -q
    return q / np.linalg.norm(q)


def q_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _project(cam, model, X):
    return synth_ba.cam_project(cam.astype(np.float64), X, pinhole=(model == CAM_PINHOLE))


def make_vba_problem(n_kf=12, n_opt=7, n_pts=300, seed=1, cams="kb8", n_cams=4, stereo_frac=0.0, outlier_frac=0.0,
                     behind_frac=0.0, views=3, min_opt_views=0, n_fixed_only=10, n_edgeless=5, obs_noise=0.7,
                     pt_noise=0.05, rot_noise_deg=0.5, trans_noise=0.02, bf=40.0, speed=1.0, yaw_rate=0.15):
    """cams: "kb8" | "pinhole" | "mixed" (cameras 0, 2 Pinhole, 1, 3 KannalaBrandt8).  behind_frac: that fraction of
    n_pts as planted behind-the-camera edges (problem["behind"] lists their mono edge indices).  min_opt_views: every
    regular point is seen from at least that many optimisable keyframes.  The first n_fixed_only points are seen from
    fixed keyframes only; n_edgeless points without edges are appended."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cam, Rbc, tbc = synth_ba.rig()
    cam, Rbc, tbc = cam[:n_cams].copy(), Rbc[:n_cams], tbc[:n_cams]
    model = dict(kb8=[CAM_KB8] * n_cams, pinhole=[CAM_PINHOLE] * n_cams,
                 mixed=[CAM_PINHOLE if c % 2 == 0 else CAM_KB8 for c in range(n_cams)])[cams]
    model = np.array(model, np.int32)
    Rcb = np.transpose(Rbc, (0, 2, 1))
    tcb = -np.einsum("cij,cj->ci", Rcb, tbc)
    # camera c <- camera 0
    R_c0 = np.einsum("cij,jk->cik", Rcb, Rbc[0])
    t_c0 = np.einsum("cij,j->ci", Rcb, tbc[0]) + tcb
    R_c0[0], t_c0[0] = np.eye(3), 0.0
    q_c0 = np.stack([q_from_R(R) for R in R_c0])
    q_c0[0] = (0, 0, 0, 1)
    R_c0 = np.stack([q_to_R(q) for q in q_c0])
    true = synth_ba.trajectory(n_kf, speed=speed, yaw_rate=yaw_rate)
    ids = list(range(n_kf - 1, -1, -1))            # array order: newest first, so the optimisable come first
    slot = {kid: s for s, kid in enumerate(ids)}
    R0w = np.stack([Rcb[0] @ true[k][0].T for k in ids])                      # camera 0's Tcw per array slot
    t0w = np.stack([-Rcb[0] @ true[k][0].T @ true[k][1] + tcb[0] for k in ids])
    Rcw = np.einsum("cij,kjl->kcil", R_c0, R0w)                               # [slot][cam]
    tcw = np.einsum("cij,kj->kci", R_c0, t0w) + t_c0[None]
    first_opt_id = n_kf - n_opt

    def views_of(Xw, kf_ids):
        """(slot, cam, uv) of the first two cameras per keyframe that see Xw inside the image."""
        out = []
        for kid in kf_ids:
            s = slot[kid]
            Xc = np.einsum("cij,j->ci", Rcw[s], Xw) + tcw[s]
            n = 0
            for c in range(n_cams):
                if Xc[c, 2] < 0.3 or n == 2:
                    continue
                uv = _project(cam[c], model[c], Xc[c])
                if 5 <= uv[0] <= 715 and 5 <= uv[1] <= 535:
                    out.append((s, c, uv))
                    n += 1
        return out

    pts_t, obs = [], []   # obs: (pt, slot, cam, uv)
    while len(pts_t) < n_pts:
        p = len(pts_t)
        fixed_only = p < n_fixed_only and first_opt_id >= 2
        if fixed_only:
            a = int(rng.integers(0, first_opt_id))
            kf_ids = [k for k in range(a - views // 2, a - views // 2 + views) if 0 <= k < first_opt_id]
        else:
            a = int(rng.integers(max(0, first_opt_id - 1), n_kf))
            lo = min(max(0, a - views // 2), max(0, n_kf - views))
            kf_ids = list(range(lo, min(n_kf, lo + views)))
        c1 = int(rng.integers(0, n_cams))
        d = rng.normal(0, 1, 3)
        d[2] = abs(d[2]) * 1.5 + 0.6
        d /= np.linalg.norm(d)
        Xw = Rcw[slot[a], c1].T @ (d * rng.uniform(2.0, 20.0) - tcw[slot[a], c1])
        v = views_of(Xw, kf_ids)
        n_kfs = len({s for s, _, _ in v})
        n_optv = len({s for s, _, _ in v if s < n_opt})
        if n_kfs < 2 or (not fixed_only and n_optv < max(1, min_opt_views)):
            continue
        pts_t.append(Xw)
        obs += [(p, s, c, uv) for s, c, uv in v]
    pts_t = np.array(pts_t)
    o_pt = np.array([o[0] for o in obs], np.int32)
    o_kf = np.array([o[1] for o in obs], np.int32)
    o_cam = np.array([o[2] for o in obs], np.int32)
    o_uv = np.array([o[3] for o in obs], np.float64)
    o_uv += rng.normal(0, 1, o_uv.shape) * obs_noise
    inv_sig = (1.0 / np.float32(1.2) ** (2 * rng.integers(0, 8, len(o_pt)))).astype(np.float32)
    # gross outliers
    if outlier_frac > 0:
        bad = rng.random(len(o_pt)) < outlier_frac
        o_uv[bad] += rng.choice([-1.0, 1.0], (int(bad.sum()), 2)) * rng.uniform(20, 60, (int(bad.sum()), 2))
    # stereo observations on camera 0 (own stream: the rest of the window does not change with stereo_frac)
    fx, fy, cx, cy = (float(v) for v in cam[0][:4])
    st = np.zeros(len(o_pt), bool)
    st_obs = np.zeros((len(o_pt), 3))
    if stereo_frac > 0:
        srng = np.random.Generator(np.random.PCG64(seed + 7919))
        st = (o_cam == 0) & (srng.random(len(o_pt)) < stereo_frac)
        for e in np.nonzero(st)[0]:
            Xc = Rcw[o_kf[e], 0] @ pts_t[o_pt[e]] + tcw[o_kf[e], 0]
            u = fx * Xc[0] / Xc[2] + cx
            st_obs[e] = (u + srng.normal(0, obs_noise), fy * Xc[1] / Xc[2] + cy + srng.normal(0, obs_noise),
                         np.float32(u - bf / Xc[2] + srng.normal(0, obs_noise)))
        st &= st_obs[:, 2] >= 0
    # planted edges behind a KannalaBrandt8 camera: exact observations, theta in (95, 110) deg
    behind = []
    n_behind = int(round(behind_frac * n_pts))
    if n_behind:
        cand = []
        for e in rng.permutation(len(o_pt)):
            p, s = o_pt[e], o_kf[e]
            Xc = np.einsum("cij,j->ci", Rcw[s], pts_t[p]) + tcw[s]
            for c in range(n_cams):
                th = np.degrees(np.arctan2(np.hypot(Xc[c, 0], Xc[c, 1]), Xc[c, 2]))
                if model[c] == CAM_KB8 and 95 < th < 110 and p >= n_fixed_only:
                    cand.append((p, s, c, _project(cam[c], CAM_KB8, Xc[c])))
                    break
            if len(cand) == n_behind:
                break
        m = len(o_pt[~st])
        behind = list(range(m, m + len(cand)))
    keep = ~st
    mono_pt, mono_kf, mono_cam = o_pt[keep], o_kf[keep], o_cam[keep]
    mono_obs, mono_w = o_uv[keep], inv_sig[keep]
    if behind:
        mono_pt = np.concatenate([mono_pt, np.array([c[0] for c in cand], np.int32)])
        mono_kf = np.concatenate([mono_kf, np.array([c[1] for c in cand], np.int32)])
        mono_cam = np.concatenate([mono_cam, np.array([c[2] for c in cand], np.int32)])
        mono_obs = np.concatenate([mono_obs, np.array([c[3] for c in cand])])
        mono_w = np.concatenate([mono_w, np.ones(len(cand), np.float32)])
    # initial state: the optimisable keyframes disturbed by exp(d) * T, the points by pt_noise
    q_t = np.stack([q_from_R(R) for R in R0w])
    q_cw, t_cw = q_t.copy(), t0w.copy()
    for s in range(n_opt):
        ax = rng.normal(0, 1, 3)
        ax /= np.linalg.norm(ax)
        dR = synth_ba._exp(ax * np.deg2rad(rot_noise_deg))
        q_cw[s] = q_from_R(dR @ R0w[s])
        t_cw[s] = dR @ t0w[s] + rng.normal(0, 1, 3) * trans_noise
    pts = pts_t + rng.normal(0, 1, pts_t.shape) * pt_noise
    if n_edgeless:
        extra = pts_t[rng.integers(0, len(pts_t), n_edgeless)] + rng.normal(0, 0.5, (n_edgeless, 3))
        pts, pts_t = np.concatenate([pts, extra]), np.concatenate([pts_t, extra])
    return dict(n_cams=n_cams, cam=cam, cam_model=model, q_c0=q_c0, t_c0=t_c0, n_kf=n_kf, n_opt=n_opt, q_cw=q_cw,
                t_cw=t_cw, pts=pts, mono_pt=mono_pt, mono_kf=mono_kf, mono_cam=mono_cam, mono_obs=mono_obs,
                mono_inv_sigma2=mono_w, stereo_pt=o_pt[st], stereo_kf=o_kf[st], stereo_obs=st_obs[st],
                stereo_inv_sigma2=inv_sig[st], fx=fx, fy=fy, cx=cx, cy=cy, bf=float(np.float32(bf)),
                behind=np.array(behind, np.int64), truth=dict(q_cw=q_t, t_cw=t0w, pts=pts_t))


def as_vba_struct(prob, struct_cls):
    """Fill an omv_vba_problem ctypes struct from a problem dict; returns (struct, keepalive dict)."""
    import ctypes
    keep = {}

    def arr(name, dtype):
        a = np.array(prob[name], dtype=dtype, order="C", copy=True)   # never alias the caller's arrays
        keep[name] = a
        return ctypes.c_void_p(a.ctypes.data)

    s = struct_cls()
    s.n_cams, s.n_kf, s.n_opt = int(prob["n_cams"]), int(prob["n_kf"]), int(prob["n_opt"])
    s.cam = arr("cam", np.float32)
    if prob.get("cam_model") is not None:
        s.cam_model = arr("cam_model", np.int32)
    for f in ("q_c0", "t_c0", "q_cw", "t_cw", "pts", "mono_obs"):
        setattr(s, f, arr(f, np.float64))
    s.n_pts = int(len(prob["pts"]))
    s.n_mono = int(len(prob["mono_pt"]))
    for f in ("mono_pt", "mono_kf", "mono_cam"):
        setattr(s, f, arr(f, np.int32))
    s.mono_inv_sigma2 = arr("mono_inv_sigma2", np.float32)
    s.n_stereo = int(len(prob.get("stereo_pt", ())))
    if s.n_stereo:
        for f in ("stereo_pt", "stereo_kf"):
            setattr(s, f, arr(f, np.int32))
        s.stereo_obs = arr("stereo_obs", np.float64)
        s.stereo_inv_sigma2 = arr("stereo_inv_sigma2", np.float32)
    for f in ("fx", "fy", "cx", "cy", "bf"):
        setattr(s, f, float(prob.get(f, 0.0)))
    return s, keep
