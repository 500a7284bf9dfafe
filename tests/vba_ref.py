"""Float64 numpy restatement of the visual bundle adjustment's graph and optimiser, the reference of the device
LocalBundleAdjustment (openmavis_amd/csrc/lba.hip, the visual kind):

  SE3Quat            exp, product, map, normalizeRotation, toRotationMatrix (Thirdparty/g2o/g2o/types/se3quat.h)
  edges              EdgeSE3ProjectXYZ and the three ...ToBody edges (include/OptimizableTypes.h:130-260,
                     src/OptimizableTypes.cpp:202-371) and g2o::EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:190-274)
                     with the reference's literal formulas: the float invz and bf * invz of the stereo projection,
                     KannalaBrandt8::project's float atan2f / sqrtf
  robustify          RobustKernelHuber, the weight rho' only (base_binary_edge.hpp:55-116)
  buildSystem        dense, with a dense landmark Schur complement (block_solver.hpp:353-486)
  optimize           the Levenberg loop of optimization_algorithm_levenberg.cpp:61-169 with the stop rule on iniChi,
                     computeLambdaInit (:171-185), computeScale + 1e-3 (:187-194), and the per-edge level mask
                     (setLevel(1) / initializeOptimization(0))

jac="numeric" takes central differences of the errors instead of the analytic Jacobians and proj="smooth" projects in
double throughout, so the restatement can be checked against itself.  A problem is openmavis_amd.synth_vba's dict; an
edge array e of the functions below lists the 2-row edges first, then the stereo edges.
"""
import numpy as np

import lm_ref
import optsim3_ref
from optsim3_ref import q_from_mat, q_mul, q_rot, q_to_mat, skew

CHI2_MONO, CHI2_STEREO = 5.991, 7.815
HUBER_MONO, HUBER_STEREO = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))


# ---- SE3Quat as (q (x y z w), t) -------------------------------------------------------------------------------------
def normalize_rotation(q):
    q = np.array(q, np.float64)
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): u = (omega, upsilon)."""
    u = np.asarray(u, np.float64)
    w, ups = u[:3], u[3:]
    theta = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = skew(w)
    O2 = O @ O
    if theta < 0.00001:
        R = np.eye(3) + O + O2
        V = R
    else:
        R = np.eye(3) + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
        V = np.eye(3) + (1 - np.cos(theta)) / (theta * theta) * O + (theta - np.sin(theta)) / (theta ** 3) * O2
    return normalize_rotation(q_from_mat(R)), V @ ups


def se3_mul(a, b):
    """SE3Quat::operator* (:104-110)."""
    return normalize_rotation(q_mul(a[0], b[0])), a[1] + q_rot(a[0], b[1])


def se3_map(T, X):
    return q_rot(T[0], X) + T[1]


def oplus(T, u):
    """VertexSE3Expmap::oplusImpl: exp(u) * T."""
    return se3_mul(se3_exp(u), T)


# ---- the graph -------------------------------------------------------------------------------------------------------
class Graph:
    """The flattened window: constants of the problem, the edge arrays (2-row edges, then stereo) and the level mask."""

    def __init__(self, prob):
        p = prob
        self.C, self.K, self.n_opt = int(p["n_cams"]), int(p["n_kf"]), int(p["n_opt"])
        self.cam = np.asarray(p["cam"], np.float32)
        self.model = np.zeros(self.C, np.int32) if p.get("cam_model") is None else np.asarray(p["cam_model"], np.int32)
        self.T_c0 = [(normalize_rotation(q), np.asarray(t, np.float64)) for q, t in zip(p["q_c0"], p["t_c0"])]
        em, es = len(p["mono_pt"]), len(p.get("stereo_pt", ()))
        self.EM, self.ES, self.E = em, es, em + es
        cat = lambda a, b, dt: np.concatenate([np.asarray(p[a], dt), np.asarray(p.get(b, ()), dt)[:es]])
        self.pt, self.kf = cat("mono_pt", "stereo_pt", np.int64), cat("mono_kf", "stereo_kf", np.int64)
        self.cam_of = np.concatenate([np.asarray(p["mono_cam"], np.int64), np.zeros(es, np.int64)])
        self.w = cat("mono_inv_sigma2", "stereo_inv_sigma2", np.float32).astype(np.float64)
        self.obs = np.zeros((self.E, 3))
        self.obs[:em, :2] = np.asarray(p["mono_obs"], np.float64).reshape(-1, 2)
        if es:
            self.obs[em:] = np.asarray(p["stereo_obs"], np.float64).reshape(-1, 3)
            self.obs[em:, 2] = self.obs[em:, 2].astype(np.float32)   # mvuRight is a float
        self.stereo = np.arange(self.E) >= em
        self.pin = tuple(float(p.get(k, 0.0)) for k in ("fx", "fy", "cx", "cy", "bf"))
        self.P = len(p["pts"])
        self.level = np.zeros(self.E, np.uint8)

    def set_levels(self, mono_level=None, stereo_level=None):
        self.level[:] = 0
        if mono_level is not None:
            self.level[:self.EM] = np.asarray(mono_level, np.uint8) != 0
        if stereo_level is not None:
            self.level[self.EM:] = np.asarray(stereo_level, np.uint8) != 0


def start_of(prob):
    return dict(q=np.array([normalize_rotation(q) for q in prob["q_cw"]]), t=np.array(prob["t_cw"], np.float64),
                pts=np.array(prob["pts"], np.float64).reshape(-1, 3))


def cam_poses(G, st):
    """Per keyframe and camera `mTrl * T` as (q [K][C][4], t [K][C][3], R [K][C][3][3]); camera 0 is T itself."""
    q, t = np.zeros((G.K, G.C, 4)), np.zeros((G.K, G.C, 3))
    for k in range(G.K):
        T = (st["q"][k], st["t"][k])
        for c in range(G.C):
            q[k, c], t[k, c] = T if c == 0 else se3_mul(G.T_c0[c], T)
    R = np.array([[q_to_mat(q[k, c]) for c in range(G.C)] for k in range(G.K)])
    return q, t, R


def _q_rot_rows(q, v):
    qv = q[:, :3]
    uv = 2.0 * np.cross(qv, v)
    return v + q[:, 3:4] * uv + np.cross(qv, uv)


def _project_cam(G, c, X, proj):
    return optsim3_ref.project(int(G.model[c]), G.cam[c].astype(np.float64), X, proj)


def stereo_project(G, X, proj="literal"):
    """EdgeStereoSE3ProjectXYZ::cam_project (types_six_dof_expmap.cpp:190-197)."""
    fx, fy, cx, cy, bf = G.pin
    with np.errstate(all="ignore"):
        if proj == "smooth":
            invz = 1.0 / X[:, 2]
            bfz = bf * invz
        else:
            invz32 = (1.0 / X[:, 2]).astype(np.float32)
            invz = invz32.astype(np.float64)
            bfz = (np.float32(bf) * invz32).astype(np.float64)
        u = X[:, 0] * invz * fx + cx
        return np.stack([u, X[:, 1] * invz * fy + cy, u - bfz], 1)


def errors(G, st, proj="literal", poses=None):
    """computeError of every edge: e [E][3] (row 2 zero on a 2-row edge), chi2 [E], the depth in the edge's camera."""
    qc, tc, _ = poses if poses is not None else cam_poses(G, st)
    Xc = _q_rot_rows(qc[G.kf, G.cam_of], st["pts"][G.pt]) + tc[G.kf, G.cam_of]
    e = np.zeros((G.E, 3))
    for c in range(G.C):
        m = (G.cam_of == c) & ~G.stereo
        if m.any():
            e[m, :2] = G.obs[m, :2] - _project_cam(G, c, Xc[m], proj)
    if G.ES:
        e[G.stereo] = G.obs[G.stereo] - stereo_project(G, Xc[G.stereo], proj)
    chi2 = G.w * (e * e).sum(1)
    return e, chi2, Xc[:, 2]


def jacobians(G, st, jac="analytic", proj="literal"):
    """linearizeOplus: JXi [E][3][3] (d e / d point), JXj [E][3][6] (d e / d pose, (omega, upsilon)); row 2 zero on a
    2-row edge."""
    if jac == "numeric":
        return _numeric_jacobians(G, st, proj)
    qc, tc, Rc = cam_poses(G, st)
    X = st["pts"][G.pt]
    Xc = _q_rot_rows(qc[G.kf, G.cam_of], X) + tc[G.kf, G.cam_of]
    Xl = _q_rot_rows(st["q"][G.kf], X) + st["t"][G.kf]
    R = Rc[G.kf, G.cam_of]
    JXi, JXj = np.zeros((G.E, 3, 3)), np.zeros((G.E, 3, 6))
    d = np.zeros((G.E, 3, 6))   # SE3deriv at X_l
    x, y, z = Xl[:, 0], Xl[:, 1], Xl[:, 2]
    d[:, 0, 1], d[:, 0, 2], d[:, 0, 3] = z, -y, 1
    d[:, 1, 0], d[:, 1, 2], d[:, 1, 4] = -z, x, 1
    d[:, 2, 0], d[:, 2, 1], d[:, 2, 5] = y, -x, 1
    R_c0 = np.array([q_to_mat(T[0]) for T in G.T_c0])
    for c in range(G.C):
        m = (G.cam_of == c) & ~G.stereo
        if not m.any():
            continue
        pj = -optsim3_ref.project_jac(int(G.model[c]), G.cam[c], Xc[m])
        JXi[m, :2] = pj @ R[m]
        JXj[m, :2] = (pj @ R_c0[c]) @ d[m] if c else pj @ d[m]
    if G.ES:
        s = G.stereo
        fx, fy, _, _, bf = G.pin
        x, y, z = Xc[s, 0], Xc[s, 1], Xc[s, 2]
        z_2 = z * z
        Rs = R[s]
        for q in range(3):
            JXi[s, 0, q] = -fx * Rs[:, 0, q] / z + fx * x * Rs[:, 2, q] / z_2
            JXi[s, 1, q] = -fy * Rs[:, 1, q] / z + fy * y * Rs[:, 2, q] / z_2
            JXi[s, 2, q] = JXi[s, 0, q] - bf * Rs[:, 2, q] / z_2
        J = np.zeros((int(s.sum()), 3, 6))
        J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx
        J[:, 0, 3], J[:, 0, 5] = -1. / z * fx, x / z_2 * fx
        J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = (1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy
        J[:, 1, 4], J[:, 1, 5] = -1. / z * fy, y / z_2 * fy
        J[:, 2, 0], J[:, 2, 1], J[:, 2, 2] = J[:, 0, 0] - bf * y / z_2, J[:, 0, 1] + bf * x / z_2, J[:, 0, 2]
        J[:, 2, 3], J[:, 2, 5] = J[:, 0, 3], J[:, 0, 5] - bf / z_2
        JXj[s] = J
    return JXi, JXj


def _numeric_jacobians(G, st, proj, delta=1e-6):
    JXi, JXj = np.zeros((G.E, 3, 3)), np.zeros((G.E, 3, 6))
    for j in range(3):   # every point moved along axis j at once: an edge sees its own point only
        ep = []
        for sgn in (1, -1):
            s = dict(st, pts=st["pts"].copy())
            s["pts"][:, j] += sgn * delta
            ep.append(errors(G, s, proj)[0])
        JXi[:, :, j] = (ep[0] - ep[1]) / (2 * delta)
    for j in range(6):
        u = np.zeros(6)
        ep = []
        for sgn in (1, -1):
            u[j] = sgn * delta
            T = [oplus((st["q"][k], st["t"][k]), u) for k in range(G.K)]
            s = dict(st, q=np.array([a for a, _ in T]), t=np.array([b for _, b in T]))
            ep.append(errors(G, s, proj)[0])
        JXj[:, :, j] = (ep[0] - ep[1]) / (2 * delta)
    return JXi, JXj


def huber(e2, delta):
    """(rho, rho') of RobustKernelHuber; delta == 0: no kernel."""
    e2 = np.asarray(e2, np.float64)
    if not delta > 0:
        return e2.copy(), np.ones_like(e2)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        s = np.sqrt(e2)
        out = e2 > dsqr
        return np.where(out, 2 * s * delta - dsqr, e2), np.where(out, delta / s, 1.0)


def robust_chi2(G, chi2, hub):
    """activeRobustChi2 and the weights rho' per edge."""
    r0, r1 = np.zeros(G.E), np.ones(G.E)
    for m, d in ((~G.stereo, hub[0]), (G.stereo, hub[1])):
        r0[m], r1[m] = huber(chi2[m], d)
    act = G.level == 0
    return float(r0[act].sum()), r1


def build_system(G, st, e, chi2, hub, jac="analytic", proj="literal"):
    """buildSystem over the active edges: Hpp [n_opt][6][6] (diagonal blocks), Hll [P][3][3], Hpl [n_opt][P][6][3],
    bp [n_opt][6], bl [P][3]."""
    JXi, JXj = jacobians(G, st, jac, proj)
    _, r1 = robust_chi2(G, chi2, hub)
    act = G.level == 0
    w = np.where(act, G.w * r1, 0.0)
    JXi, JXj = np.where(act[:, None, None], JXi, 0.0), np.where(act[:, None, None], JXj, 0.0)
    om = -w[:, None] * np.where(act[:, None], e, 0.0)
    n = G.n_opt
    Hpp, Hll, Hpl = np.zeros((n, 6, 6)), np.zeros((G.P, 3, 3)), np.zeros((n, G.P, 6, 3))
    bp, bl = np.zeros((n, 6)), np.zeros((G.P, 3))
    np.add.at(Hll, G.pt, w[:, None, None] * np.einsum("eri,erj->eij", JXi, JXi))
    np.add.at(bl, G.pt, np.einsum("eri,er->ei", JXi, om))
    o = G.kf < n
    np.add.at(Hpp, G.kf[o], w[o, None, None] * np.einsum("eri,erj->eij", JXj[o], JXj[o]))
    np.add.at(bp, G.kf[o], np.einsum("eri,er->ei", JXj[o], om[o]))
    np.add.at(Hpl, (G.kf[o], G.pt[o]), w[o, None, None] * np.einsum("eri,erj->eij", JXj[o], JXi[o]))
    return dict(Hpp=Hpp, Hll=Hll, Hpl=Hpl, bp=bp, bl=bl, active_pt=np.bincount(G.pt[act], minlength=G.P) > 0)


def max_diagonal(sys_):
    """max |H(j,j)| over the active vertices (poses and landmarks)."""
    dp = np.abs(np.einsum("kii->ki", sys_["Hpp"]))
    dl = np.abs(np.einsum("pii->pi", sys_["Hll"]))[sys_["active_pt"]]
    return max(dp.max(initial=0.0), dl.max(initial=0.0))


def lambda_init(sys_):
    """computeLambdaInit without a user value."""
    return lm_ref.lambda_init(0.0, max_diagonal(sys_))


def reduce_system(sys_, lam):
    """The landmark Schur complement at damping lam: S [6 n][6 n], rhs [6 n], and what the back-substitution needs."""
    n, P = sys_["Hpp"].shape[0], sys_["Hll"].shape[0]
    act = sys_["active_pt"]
    D = sys_["Hll"] + lam * np.eye(3)
    Dinv = np.zeros_like(D)
    Dinv[act] = np.linalg.inv(D[act])
    Y = np.einsum("kpij,pjl->kpil", sys_["Hpl"], Dinv)   # Hpl Dinv
    S = np.zeros((6 * n, 6 * n))
    for k in range(n):
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = sys_["Hpp"][k] + lam * np.eye(6)
    Ym = Y.transpose(0, 2, 1, 3).reshape(6 * n, 3 * P)
    Hm = sys_["Hpl"].transpose(0, 2, 1, 3).reshape(6 * n, 3 * P)
    S -= Ym @ Hm.T
    rhs = sys_["bp"].reshape(-1) - Ym @ sys_["bl"].reshape(-1)
    return S, rhs, Dinv, Hm


def solve(sys_, lam):
    """One damped solve: (ok, xp [n][6], xl [P][3])."""
    S, rhs, Dinv, Hm = reduce_system(sys_, lam)
    try:
        xp = np.linalg.solve(S, rhs)
    except np.linalg.LinAlgError:
        return False, None, None
    xl = np.einsum("pij,pj->pi", Dinv, sys_["bl"] - (Hm.T @ xp).reshape(-1, 3))
    ok = bool(np.isfinite(xp).all() and np.isfinite(xl).all())
    return ok, xp.reshape(-1, 6), xl


def update(G, st, xp, xl):
    s = dict(q=st["q"].copy(), t=st["t"].copy(), pts=st["pts"] + xl)
    for k in range(G.n_opt):
        s["q"][k], s["t"][k] = oplus((st["q"][k], st["t"][k]), xp[k])
    return s


def optimize(G, st, iterations=10, lambda_init_user=0.0, max_trials=10, hub=(HUBER_MONO, HUBER_STEREO),
             jac="analytic", proj="literal"):
    """optimizer.optimize(iterations) from state `st`.  Returns (result, final state): err, err_end, iterations, trials,
    lambda_, lambda_init, chi2 [E] of the last computed errors, outlier [E] (chi2 > threshold || !isDepthPositive at the
    final state), and for the tests' own conditions `rhos` (every trial's rho) and `stops` (both sides of the stop rule
    per finished iteration)."""
    e, chi2, _ = errors(G, st, proj)
    chi, _ = robust_chi2(G, chi2, hub)
    res = dict(err=chi, iterations=0, trials=0, rhos=[], stops=[], lambda_init=lambda_init_user)
    lm = lm_ref.LmState()   # the step control: lm_ref
    cur_e, cur_chi2, cur_chi = e, chi2, chi
    last_chi2, last_chi = chi2, chi
    for it in range(iterations):
        res["iterations"] += 1
        sys_ = build_system(G, st, cur_e, cur_chi2, hub, jac, proj)
        md = max_diagonal(sys_) if it == 0 else 0.0
        lm_ref.begin_iteration(lm, it, cur_chi, lm_ref.lambda_init(lambda_init_user, md))
        if it == 0:
            res["lambda_init"] = lm.lam
        while True:
            ok, xp, xl = solve(sys_, lm.lam)
            scale, temp_chi = 0.0, 0.0   # a failed solve: lm_ref puts DBL_MAX in the chi2's place
            if ok:
                trial = update(G, st, xp, xl)
                te, tchi2, _ = errors(G, trial, proj)
                temp_chi, _ = robust_chi2(G, tchi2, hub)
                last_chi2, last_chi = tchi2, temp_chi
                scale = float((xp * (lm.lam * xp + sys_["bp"])).sum() + (xl * (lm.lam * xl + sys_["bl"])).sum())
            rho, accepted = lm_ref.trial(lm, temp_chi, ok, scale)
            res["trials"] += 1
            res["rhos"].append(rho)
            if accepted:
                st, cur_e, cur_chi2, cur_chi = trial, te, tchi2, temp_chi
            stop_sides = lm_ref.gain_sides(lm)
            nxt = lm_ref.next_step(lm, rho, max_trials)
            if nxt != lm_ref.TRIAL:
                break
        if nxt == lm_ref.ITERATION or lm.n_bad >= 3:   # the stop rule was reached (no Terminate from the trials)
            res["stops"].append(stop_sides)
        if nxt == lm_ref.STOP:
            break
    _, _, depth = errors(G, st, proj)
    thr = np.where(G.stereo, CHI2_STEREO, CHI2_MONO)
    res.update(err_end=last_chi, lambda_=lm.lam, chi2=last_chi2, depth=depth,
               outlier=((last_chi2 > thr) | ~(depth > 0.0)).astype(np.uint8))
    return res, st
