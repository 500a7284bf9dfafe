"""Seeded synthetic FullInertialBA problems (Optimizer::FullInertialBA, src/Optimizer.cc:368-853), on top of synth_ba.

A whole small map: K keyframes on synth_ba's trajectory, oldest to newest in mnId order as GetAllKeyFrames lists them after
sorting, every one optimisable -- or, with fix_last (bFixLocal), the newest (the maxKFid keyframe) listed last and fixed.
One EdgeInertial per keyframe with a previous one (mPrevKF), every one Huber at its full information.  shared_bias is
the bInit form: one gyro / acc bias pair for the map, started at bg0 / ba0, under the two priors.

Variations: no_imu_first (the oldest keyframe is not bImu: a pose vertex only, and the edge from it does not exist),
break_chain (one keyframe in the middle has no mPrevKF), pinhole (Pinhole cameras), stereo_frac (EdgeStereo on camera 0),
fixed_only_pts (that many points seen by the fixed keyframe only: no vertices, they do not move), wide_landmarks
(landmarks observed by `wide_kfs` keyframes: past the 32 optimisable keyframes of a build group).
"""
import numpy as np

from . import synth_ba

FIBA_FIELDS = ("shared_bias", "prior_g", "prior_a", "bg0", "ba0")


def _drop_keyframe(prob, k):
    """Keyframe index k and everything attached to it leave the problem; later indices move down."""
    prob = dict(prob)
    K = prob["n_kf"]
    keep_kf = np.arange(K) != k
    new = np.cumsum(keep_kf) - 1
    for f in ("kf_imu", "Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba"):
        prob[f] = np.asarray(prob[f])[keep_kf]
    m = np.asarray(prob["mono_kf"]) != k
    for f in ("mono_pt", "mono_kf", "mono_cam", "mono_obs", "mono_inv_sigma2"):
        prob[f] = np.asarray(prob[f])[m]
    prob["mono_kf"] = new[prob["mono_kf"]].astype(np.int32)
    if prob.get("n_stereo", 0):
        m = np.asarray(prob["stereo_kf"]) != k
        for f in ("stereo_pt", "stereo_kf", "stereo_obs", "stereo_inv_sigma2"):
            prob[f] = np.asarray(prob[f])[m]
        prob["stereo_kf"] = new[prob["stereo_kf"]].astype(np.int32)
        prob["n_stereo"] = int(m.sum())
    m = (np.asarray(prob["imu_kf1"]) != k) & (np.asarray(prob["imu_kf2"]) != k)
    for f in ("imu_kf1", "imu_kf2", "preint", "imu_robust", "imu_info_scale"):
        prob[f] = np.asarray(prob[f])[m]
    prob["imu_kf1"], prob["imu_kf2"] = new[prob["imu_kf1"]].astype(np.int32), new[prob["imu_kf2"]].astype(np.int32)
    prob["n_kf"] = K - 1
    prob["n_opt"] = min(prob["n_opt"], K - 1)
    t = prob["truth"]
    prob["truth"] = dict(Rwb=t["Rwb"][keep_kf], twb=t["twb"][keep_kf], pts=t["pts"])
    return prob


def _reorder_keyframes(prob, order):
    """Keyframe `order[i]` becomes keyframe i."""
    prob = dict(prob)
    order = np.asarray(order)
    new = np.empty(len(order), np.int64)
    new[order] = np.arange(len(order))
    for f in ("kf_imu", "Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba"):
        prob[f] = np.asarray(prob[f])[order]
    for f in ("mono_kf", "imu_kf1", "imu_kf2") + (("stereo_kf",) if prob.get("n_stereo", 0) else ()):
        prob[f] = new[np.asarray(prob[f])].astype(np.int32)
    t = prob["truth"]
    prob["truth"] = dict(Rwb=t["Rwb"][order], twb=t["twb"][order], pts=t["pts"])
    return prob


def _drop_imu_edges(prob, mask):
    prob = dict(prob)
    for f in ("imu_kf1", "imu_kf2", "preint", "imu_robust", "imu_info_scale"):
        prob[f] = np.asarray(prob[f])[~mask]
    return prob


def _best_camera_obs(prob, k, X, pinhole):
    """Camera and projection of world point X in keyframe k's true pose: the camera that sees it at the largest depth."""
    t = prob["truth"]
    Rbw = t["Rwb"][k].T
    Xb = Rbw @ (X - t["twb"][k])
    Xc = np.einsum("cij,j->ci", prob["Rcb"], Xb) + prob["tcb"]
    c = int(np.argmax(Xc[:, 2]))
    return c, Xc[c], synth_ba.cam_project(np.asarray(prob["cam"][c], np.float64), Xc[c], pinhole)


def make_fiba_problem(n_kf=12, n_pts=300, seed=7, fix_last=False, shared_bias=True, prior_g=1e2, prior_a=1e5,
                      no_imu_first=False, break_chain=False, pinhole=False, stereo_frac=0.0, n_cams=5,
                      fixed_only_pts=0, wide_landmarks=0, wide_kfs=34, bias_sigma=(1e-4, 1e-3), **noise):
    """The problem dict of FullInertialBA.set_problem: synth_ba.make_lba_problem's fields plus shared_bias, prior_g,
    prior_a, bg0, ba0.  `noise`: obs_noise, pt_noise, rot_noise_deg, trans_noise of make_lba_problem."""
    K = int(n_kf)
    # K + 1 keyframes with the oldest fixed, which then leaves: every edge of the K others has its previous keyframe
    prob = synth_ba.make_lba_problem(n_kf=K + 1, n_opt=K, n_pts=n_pts, seed=seed, n_cams=n_cams, pinhole=pinhole,
                                     stereo_frac=stereo_frac, **noise)
    prob = _drop_keyframe(prob, K)
    # make_lba_problem lists newest first; a map lists by mnId (oldest first)
    prob = _reorder_keyframes(prob, np.arange(K)[::-1])
    rng = np.random.default_rng(seed + 104729)
    if wide_landmarks:
        t = prob["truth"]
        add = dict(pt=[], kf=[], cam=[], obs=[])
        first = np.linspace(0, max(K - wide_kfs, 0), wide_landmarks).astype(int)
        for p in range(wide_landmarks):
            seen = set(np.asarray(prob["mono_kf"])[np.asarray(prob["mono_pt"]) == p].tolist())
            for k in range(first[p], min(first[p] + wide_kfs, K)):
                if k in seen:
                    continue
                c, Xc, uv = _best_camera_obs(prob, k, t["pts"][p], pinhole)
                if pinhole and Xc[2] < 0.3:   # (KannalaBrandt8 projects any direction: every wide landmark gets them all)
                    continue
                add["pt"].append(p), add["kf"].append(k), add["cam"].append(c), add["obs"].append(uv + rng.normal(0, 0.7, 2))
        n = len(add["pt"])
        prob["mono_pt"] = np.concatenate([prob["mono_pt"], np.array(add["pt"], np.int32)])
        prob["mono_kf"] = np.concatenate([prob["mono_kf"], np.array(add["kf"], np.int32)])
        prob["mono_cam"] = np.concatenate([prob["mono_cam"], np.array(add["cam"], np.int32)])
        prob["mono_obs"] = np.concatenate([prob["mono_obs"], np.array(add["obs"], np.float64).reshape(n, 2)])
        prob["mono_inv_sigma2"] = np.concatenate([prob["mono_inv_sigma2"], np.ones(n, np.float32)])
    if fix_last:   # bFixLocal: the maxKFid keyframe after the optimisable ones (n_opt = n_kf - 1)
        prob["n_opt"] = K - 1
        if fixed_only_pts:   # points 0 .. n-1: seen by the fixed keyframe only
            keep = ~((np.asarray(prob["mono_pt"]) < fixed_only_pts) & (np.asarray(prob["mono_kf"]) < K - 1))
            for f in ("mono_pt", "mono_kf", "mono_cam", "mono_obs", "mono_inv_sigma2"):
                prob[f] = np.asarray(prob[f])[keep]
            t = prob["truth"]
            add = dict(pt=[], cam=[], obs=[])
            for p in range(fixed_only_pts):
                if ((np.asarray(prob["mono_pt"]) == p) & (np.asarray(prob["mono_kf"]) == K - 1)).any():
                    continue
                c, Xc, uv = _best_camera_obs(prob, K - 1, t["pts"][p], pinhole)
                add["pt"].append(p), add["cam"].append(c), add["obs"].append(uv)
            n = len(add["pt"])
            prob["mono_pt"] = np.concatenate([prob["mono_pt"], np.array(add["pt"], np.int32)])
            prob["mono_kf"] = np.concatenate([prob["mono_kf"], np.full(n, K - 1, np.int32)])
            prob["mono_cam"] = np.concatenate([prob["mono_cam"], np.array(add["cam"], np.int32)])
            prob["mono_obs"] = np.concatenate([prob["mono_obs"], np.array(add["obs"], np.float64).reshape(n, 2)])
            prob["mono_inv_sigma2"] = np.concatenate([prob["mono_inv_sigma2"], np.ones(n, np.float32)])
    else:
        prob["n_opt"] = K
    kf_imu = np.ones(K, np.uint8)
    drop = np.zeros(len(prob["imu_kf1"]), bool)
    if no_imu_first:   # an inertial edge exists between two bImu keyframes only (:469)
        kf_imu[0] = 0
        drop |= (np.asarray(prob["imu_kf1"]) == 0) | (np.asarray(prob["imu_kf2"]) == 0)
    if break_chain:    # a keyframe without mPrevKF (:461-464)
        drop |= np.asarray(prob["imu_kf2"]) == K // 2
    prob = _drop_imu_edges(prob, drop)
    prob["kf_imu"] = kf_imu
    # every EdgeInertial Huber at its full information (:514-516): what the other solvers of this dict are to use
    prob["imu_robust"] = np.ones(len(prob["imu_kf1"]), np.uint8)
    prob["imu_info_scale"] = np.ones(len(prob["imu_kf1"]), np.float32)
    prob["bg"] = rng.normal(0, bias_sigma[0], (K, 3)) * kf_imu[:, None]
    prob["ba"] = rng.normal(0, bias_sigma[1], (K, 3)) * kf_imu[:, None]
    prob["shared_bias"] = int(bool(shared_bias))
    prob["prior_g"], prob["prior_a"] = float(prior_g), float(prior_a)
    prob["bg0"], prob["ba0"] = rng.normal(0, bias_sigma[0], 3), rng.normal(0, bias_sigma[1], 3)
    if shared_bias:   # every bImu keyframe holds the pair
        prob["bg"] = np.where(kf_imu[:, None] > 0, prob["bg0"][None], 0.0)
        prob["ba"] = np.where(kf_imu[:, None] > 0, prob["ba0"][None], 0.0)
    return prob


def as_fiba_struct(prob, struct_cls, base_cls):
    """Fill an omv_fiba_problem ctypes struct from a problem dict; returns (struct, keepalive dict of the base arrays)."""
    base, keep = synth_ba.as_struct(prob, base_cls)
    s = struct_cls()
    s.base = base
    s.shared_bias = int(prob.get("shared_bias", 0))
    s.prior_g, s.prior_a = float(prob.get("prior_g", 0.0)), float(prob.get("prior_a", 0.0))
    for q in range(3):
        s.bg0[q] = float(np.asarray(prob.get("bg0", np.zeros(3)))[q])
        s.ba0[q] = float(np.asarray(prob.get("ba0", np.zeros(3)))[q])
    return s, keep
