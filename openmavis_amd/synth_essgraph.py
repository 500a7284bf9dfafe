"""Synthetic loop-closing pose graphs for Optimizer::OptimizeEssentialGraph / OptimizeEssentialGraph4DoF (the device
form: openmavis_amd.optimizer.EssentialGraph): a closed trajectory whose estimate drifted (scale drift for the Sim3 kind,
yaw and translation drift for the 4DoF kind), the last few keyframes with CorrectedSim3 / NonCorrectedSim3 entries, and
the edges in the reference's creation order -- loop connections, then per keyframe its spanning-tree edge, its edge to
the predecessor, its older loop edges and its covisibility edges (some more than one 16-row block apart, so the
factorisation fills)."""
import numpy as np


def _rot(axis, a):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _quat(R):
    """(x y z w) of a rotation matrix, w >= 0."""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:   # half-turns do not occur on these trajectories; kept for completeness
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
        q = np.zeros(4)
        q[i], q[3], q[j], q[k] = t / 2, (R[k, j] - R[j, k]) / (2 * t), (R[j, i] + R[i, j]) / (2 * t), (R[k, i] + R[i, k]) / (2 * t)
    return q / np.linalg.norm(q)


def _sim3(R, t, s=1.0):
    return np.concatenate([_quat(R), np.asarray(t, np.float64), [s]])


def make_essgraph_problem(kind="sim3", n_kf=40, seed=0, n_corrected=4, fix_scale=0, drift=1.0, covis=(2, 3), far=5,
                          old_loop=True, n_points=48, fixed=(0,), merge=False):
    """A problem dict for EssentialGraph.set_problem (and tests/essgraph_ref.py).

    kind 'sim3' | '4dof'; n_kf keyframes on a closed loop, keyframe 0 the loop keyframe; the last n_corrected keyframes
    carry a CorrectedSim3 entry (S_a) beside their drifted pose (S_b); `drift` scales the accumulated error; covis: the
    covisibility offsets of every keyframe, `far` one more for every third keyframe; fixed: the fixed vertices; merge:
    a merge-shaped graph -- a second fixed set, edges drawn from either table, a parallel pair and a fixed-fixed edge."""
    rng = np.random.default_rng(seed)
    sim3 = kind == "sim3"
    n = int(n_kf)
    # ground truth: camera centres on a circle, the camera yawing with it; Tcw = (R, t)
    ang = 2 * np.pi * np.arange(n) / n
    Rcw_gt, tcw_gt = [], []
    for a in ang:
        Rwc = _rot([0, 0, 1], a) @ _rot([1, 0, 0], 0.1 * np.sin(3 * a))
        twc = np.array([6 * np.cos(a), 6 * np.sin(a), 0.3 * np.sin(2 * a)])
        Rcw_gt.append(Rwc.T), tcw_gt.append(-Rwc.T @ twc)
    # the drifted estimate: the true relative motions, each with a small error, integrated from keyframe 0
    Rd, td = [Rcw_gt[0]], [tcw_gt[0]]
    scale = 1.0
    for k in range(1, n):
        dR = Rcw_gt[k] @ Rcw_gt[k - 1].T
        dt = tcw_gt[k] - dR @ tcw_gt[k - 1]
        if sim3:
            scale *= np.exp(drift * 0.004 * (1 + 0.3 * rng.standard_normal()))
            eR = _rot(rng.standard_normal(3), drift * 0.002 * rng.standard_normal())
            et = drift * 0.004 * rng.standard_normal(3)
        else:   # yaw (about the world's gravity axis) and translation drift only
            eR = _rot([0, 0, 1], drift * 0.004 * (1 + 0.3 * rng.standard_normal()))
            et = drift * 0.01 * rng.standard_normal(3)
        Rk = eR @ dR @ Rd[-1] if sim3 else dR @ Rd[-1] @ eR
        Rd.append(Rk), td.append(dR @ td[-1] + scale * dt + et)
    S_pose = np.stack([_sim3(Rd[k], td[k], 1.0) for k in range(n)])
    S_a, S_b = S_pose.copy(), S_pose.copy()
    a_end = 1.0 if (not sim3 or fix_scale) else scale
    corrected = list(range(n - n_corrected, n))
    for k in corrected:   # the loop's correction: the true pose in the drifted map's scale
        S_a[k] = _sim3(Rcw_gt[k], a_end * tcw_gt[k], a_end)
    fixed_flag = np.zeros(n, np.uint8)
    fixed_flag[list(fixed)] = 1
    ei, ej, et_ = [], [], []
    inserted = set()

    def add(i, j, tab):
        ei.append(i), ej.append(j), et_.append(tab)

    # loop connections (vScw on both sides): the corrected keyframes against the loop keyframe and its neighbours
    for i in corrected[-2:]:
        for j in (0, 1):
            add(i, j, 0)
            inserted.add((min(i, j), max(i, j)))
    old = (n // 2, n // 4) if old_loop and n >= 12 else None
    for k in range(n):
        if k > 0:
            if sim3:
                add(k, k - 1, 1)   # spanning tree: the parent
            add(k, k - 1, 1)       # the predecessor (mPrevKF): beside the parent's edge, a parallel pair
        if old and k == old[0]:
            add(k, old[1], 1)      # an older loop edge (pLKF->mnId < pKF->mnId)
        offs = list(covis) + ([far] if far and k % 3 == 0 else [])
        for o in offs:
            j = k - o
            if j < 0 or (j, k) in inserted or (old and (k, j) == old):
                continue
            add(k, j, 1)
    if merge:
        second = [n // 3, n // 3 + 1]
        fixed_flag[second] = 1
        add(second[1], second[0], 0)          # fixed-fixed: chi2 only
        add(n // 3 + 2, second[0], 0)         # drawn from the other table
        add(n - 1, n // 3 + 1, 0)
    prob = dict(kind=kind, vertices=None, fixed=fixed_flag, S_a=S_a, S_b=S_b, edge_i=np.array(ei, np.int32),
                edge_j=np.array(ej, np.int32), edge_table=np.array(et_, np.int32), fix_scale=int(fix_scale), Rcb=None,
                tcb=None)
    if sim3:
        prob["vertices"] = S_a.copy()
    else:
        Rcb = _rot([0.2, -0.5, 1.0], 0.4)
        tcb = np.array([0.05, -0.02, 0.1])
        v = np.zeros((n, 24))
        for k in range(n):   # ImuCamPose(pKF) / ImuCamPose(Rwc, twc, pKF) (G2oTypes.cc:142-166) from vScw's inverse
            R, t, s = _q_to_mat(S_a[k, :4]), S_a[k, 4:7], S_a[k, 7]
            Rwc, twc = R.T, -(R.T @ t) / s
            v[k, 0:9], v[k, 9:12] = Rwc.T.reshape(-1), -Rwc.T @ twc
            v[k, 12:21], v[k, 21:24] = (Rwc @ Rcb).reshape(-1), Rwc @ tcb + twc
        prob.update(vertices=v, Rcb=Rcb.reshape(-1), tcb=tcb)
    # map points near the trajectory, each with a reference keyframe (-1: not corrected)
    ref = rng.integers(0, n, n_points).astype(np.int32)
    ref[::7] = -1
    pts = (rng.standard_normal((n_points, 3)) * [4.0, 4.0, 0.5]).astype(np.float32)
    prob.update(points=pts, point_ref=ref)
    return prob


def _q_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
