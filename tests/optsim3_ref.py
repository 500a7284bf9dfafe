"""Reference for the device Optimizer::OptimizeSim3 (src/Optimizer.cc:2460-2726): a float64 numpy restatement of the
whole function on the same inputs -- g2o::Sim3 (exp, *, inverse, map; Thirdparty/g2o/g2o/types/sim3.h) written
literally, VertexSim3Expmap::oplusImpl, the two projection edges, g2o's Levenberg-Marquardt with the reference's
modifications (optimization_algorithm_levenberg.cpp:61-169), the dense pivoted LDL^T (oracle/linalg_ref.py), the two
rounds with their stale-error test and the quirks (the z < 0 skip, the return before the write-back, the literal NaN
comparisons).

The Jacobian is selectable: jac="numeric" is g2o's central differences with delta = 1e-9 through oplus / computeError
(base_binary_edge.hpp:143-203; both edges have linearizeOplus commented out), jac="analytic" the closed forms the
device uses, with Y = S12 X2, Z = S12^-1 X1 and the update ordered (omega, upsilon, sigma):
    d e12 / d u = -Jpi1(Y) [ -[Y]x | I | Y ]          d e21 / d u = -Jpi2(Z) (R^T / s) [ [X1]x | -I | -X1 ]

The projection is selectable too.  proj="smooth" is sim3_ref.project (float64 throughout).  proj="literal" differs for
KannalaBrandt8 only: KannalaBrandt8::project(const Eigen::Vector3d&) takes theta and psi through atan2f / sqrtf on
float-cast arguments (KannalaBrandt8.cpp:28-46), which the device restates (g2o_types.h kb8_project); here the two float
functions come from the project's math header through the oracle library, so the residuals agree to double rounding.
That projection is piecewise constant at the 1e-7 rad level, so central differences with delta = 1e-9 through it are
meaningless: the numeric scheme is compared on the smooth projection.

A job is a dict.  Per entry (the i that pass the graph-side filter, openmavis_amd.optimizer.select_sim3_edges): index1
[N], Xw1, Xw2 [N][3] float32, obs1 [N][2] float32 (kp1.pt), inv_sigma2_1 [N] float32, has_kp2 [N], obs2 [N][2] float32
(kp2.pt; ignored without a keypoint), inv_sigma2_2 [N] float32.  Per job: pose1, pose2 [12] float32 (Riw row-major,
tiw), cam1, cam2 [8] float32, model1, model2 (0 KB8, 1 Pinhole), fix_scale, th2, and S12 as q [4] (x y z w), t [3], s
(float64).  Status per entry: 0 match kept but not counted (not an edge: z < 0; or the function returned 0 before the
final test), 1 inlier, 2 removed after round one, 3 removed at the end: n_in is always the number of status-1 entries."""
import numpy as np

import linalg_ref
import lm_ref
import sim3_ref

NOT_EDGE, INLIER, REMOVED_1, REMOVED_2 = 0, 1, 2, 3


# ---- Eigen quaternions on (x y z w) -------------------------------------------------------------------------------
def q_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def q_rot(q, v):
    """Quaternion * vector (_transformVector): v + w uv + q x uv with uv = 2 q x v; v [3] or [n][3]."""
    v = np.asarray(v, np.float64)
    qv = np.broadcast_to(q[:3], v.shape)
    uv = 2.0 * np.cross(qv, v)
    return v + q[3] * uv + np.cross(qv, uv)


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_from_mat(m):
    """Eigen::Quaterniond(Matrix3d)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def q_to_mat(q):
    """Quaterniond::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


# ---- g2o::Sim3 as (q, t, s) ---------------------------------------------------------------------------------------
def sim3_exp(u):
    """Sim3(const Vector7d &update) (sim3.h:70-142): four branches on |sigma| < 1e-5 and theta < 1e-5."""
    u = np.asarray(u, np.float64)
    omega, upsilon, sigma = u[:3], u[3:6], u[6]
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = skew(omega)
    s = np.exp(sigma)
    Om2 = Om @ Om
    I = np.eye(3)
    eps = 0.00001
    with np.errstate(all="ignore"):
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B = 1. / 2., 1. / 6.
                R = I + Om + Om @ Om
            else:
                theta2 = theta * theta
                A = (1 - np.cos(theta)) / theta2
                B = (theta - np.sin(theta)) / (theta2 * theta)
                R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = I + Om + Om2
            else:
                R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
                a, b = s * np.sin(theta), s * np.cos(theta)
                theta2, sigma2 = theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        W = A * Om + B * Om2 + C * I
        return q_from_mat(R), W @ upsilon, s


def sim3_mul(a, b):
    """operator*: r is not renormalised."""
    return q_mul(a[0], b[0]), a[2] * q_rot(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inverse(a):
    qc = q_conj(a[0])
    return qc, q_rot(qc, (-1. / a[2]) * a[1]), 1. / a[2]


def sim3_map(a, X):
    return a[2] * q_rot(a[0], X) + a[1]


def oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl."""
    u = np.array(u, np.float64)
    if fix_scale:
        u[6] = 0
    return sim3_mul(sim3_exp(u), S)


# ---- cameras --------------------------------------------------------------------------------------------------------
def _oracle():
    import oracle
    from openmavis_amd import selftest as st
    return oracle, st


def project(model, k, X, proj="literal"):
    """pCamera->project(const Eigen::Vector3d&) for [n][3] points."""
    if model == 1 or proj == "smooth":
        return sim3_ref.project(model, k, X)
    oracle, st = _oracle()
    k = np.asarray(k, np.float64)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x2y2 = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
        rf = oracle.math_map(st.SQRTF, x2y2.astype(np.float32))
        th = oracle.math_map(st.ATAN2F, rf, X[:, 2].astype(np.float32)).astype(np.float64)
        psi = oracle.math_map(st.ATAN2F, X[:, 1].astype(np.float32), X[:, 0].astype(np.float32)).astype(np.float64)
        t2 = th * th
        t3 = th * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = th + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9
        return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def project_f(model, k, X):
    """pCamera->project(const Eigen::Vector3f&) in float, through the project's math header on the host."""
    oracle, st = _oracle()
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    if len(X) == 0:
        return np.zeros((0, 2), np.float32)
    return oracle.math_map(st.PINHOLE_PROJECT if model == 1 else st.KB8_PROJECT, X, np.asarray(k, np.float32)).reshape(-1, 2)


def project_jac(model, k, X):
    """pCamera->projectJac for [n][3] points -> [n][2][3] (Pinhole.cpp:55-65, KannalaBrandt8.cpp:128-158)."""
    k32 = np.asarray(k, np.float32)
    k = k32.astype(np.float64)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    J = np.zeros((len(X), 2, 3))
    with np.errstate(all="ignore"):
        if model == 1:
            J[:, 0, 0] = k[0] / z
            J[:, 0, 2] = -k[0] * x / (z * z)
            J[:, 1, 1] = k[1] / z
            J[:, 1, 2] = -k[1] * y / (z * z)
            return J
        x2, y2, z2 = x * x, y * y, z * z
        r2 = x2 + y2
        r = np.sqrt(r2)
        r3 = r2 * r
        th = np.arctan2(r, z)
        t2 = th * th
        t3 = t2 * th
        t4 = t2 * t2
        t5 = t4 * th
        t6 = t2 * t4
        t7 = t6 * th
        t8 = t4 * t4
        t9 = t8 * th
        f = th + t3 * k[4] + t5 * k[5] + t7 * k[6] + t9 * k[7]
        kk = [np.float64(np.float32(m) * k32[4 + i]) for i, m in enumerate((3, 5, 7, 9))]   # int x float products
        fd = 1 + kk[0] * t2 + kk[1] * t4 + kk[2] * t6 + kk[3] * t8
        xy = fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3
        J[:, 0, 0] = k[0] * (fd * z * x2 / (r2 * (r2 + z2)) + f * y2 / r3)
        J[:, 1, 0] = k[1] * xy
        J[:, 0, 1] = k[0] * xy
        J[:, 1, 1] = k[1] * (fd * z * y2 / (r2 * (r2 + z2)) + f * x2 / r3)
        J[:, 0, 2] = -k[0] * fd * x / (r2 + z2)
        J[:, 1, 2] = -k[1] * fd * y / (r2 + z2)
    return J


# ---- the graph's numeric part (:2541-2653) ---------------------------------------------------------------------------
def _rt_f32(pose, Xw):
    """R Xw + t in float as Eigen evaluates it: each row a 3-term sum left to right, then the translation."""
    p = np.asarray(pose, np.float32)
    R, t = p[:9].reshape(3, 3), p[9:]
    X = np.asarray(Xw, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)], 1)


def prepare(job):
    """P3D1c / P3D2c (float, cast to double), the z < 0 skip, obs2 of the entries without a KF2 keypoint, the edge
    weights and Huber's delta."""
    X1f, X2f = _rt_f32(job["pose1"], job["Xw1"]), _rt_f32(job["pose2"], job["Xw2"])
    edge = ~(X2f[:, 2] < 0)
    has = np.asarray(job["has_kp2"], bool).reshape(-1)
    obs2 = np.asarray(job["obs2"], np.float32).reshape(-1, 2).copy()
    if (~has).any():
        obs2[~has] = project_f(job["model2"], job["cam2"], X2f[~has])
    th2 = np.float32(job["th2"])
    return dict(X1=X1f.astype(np.float64), X2=X2f.astype(np.float64), edge=edge,
                obs1=np.asarray(job["obs1"], np.float32).reshape(-1, 2).astype(np.float64), obs2=obs2.astype(np.float64),
                w1=np.asarray(job["inv_sigma2_1"], np.float32).astype(np.float64).reshape(-1),
                w2=np.asarray(job["inv_sigma2_2"], np.float32).astype(np.float64).reshape(-1),
                th2=np.float64(th2), delta=np.float64(np.float32(np.sqrt(th2))))


def start_of(job):
    return (np.array(job["q"], np.float64), np.array(job["t"], np.float64), np.float64(job["s"]))


def errors(job, pre, S, proj="literal"):
    """computeError of both edges for every entry: e12, e21 [N][2]."""
    with np.errstate(all="ignore"):
        e12 = pre["obs1"] - project(job["model1"], job["cam1"], sim3_map(S, pre["X2"]), proj)
        e21 = pre["obs2"] - project(job["model2"], job["cam2"], sim3_map(sim3_inverse(S), pre["X1"]), proj)
    return e12, e21


def chi2_of(pre, e12, e21):
    with np.errstate(all="ignore"):
        return (e12[:, 0] * (pre["w1"] * e12[:, 0]) + e12[:, 1] * (pre["w1"] * e12[:, 1]),
                e21[:, 0] * (pre["w2"] * e21[:, 0]) + e21[:, 1] * (pre["w2"] * e21[:, 1]))


def jacobians(job, pre, S, fix_scale, jac="analytic", proj="literal"):
    """_jacobianOplusXj of both edges: [N][2][7] each."""
    n = len(pre["X1"])
    if jac == "numeric":
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
        for d in range(7):
            add = np.zeros(7)
            add[d] = delta
            a12, a21 = errors(job, pre, oplus(S, add, fix_scale), proj)
            add[d] = -delta
            b12, b21 = errors(job, pre, oplus(S, add, fix_scale), proj)
            J12[:, :, d], J21[:, :, d] = scalar * (a12 - b12), scalar * (a21 - b21)
        return J12, J21
    with np.errstate(all="ignore"):
        Y = sim3_map(S, pre["X2"])
        Z = sim3_map(sim3_inverse(S), pre["X1"])
        X1 = pre["X1"]
        A = np.zeros((n, 3, 7))   # [ -[Y]x | I | Y ]
        A[:, 0, 1], A[:, 0, 2], A[:, 1, 0] = Y[:, 2], -Y[:, 1], -Y[:, 2]
        A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = Y[:, 0], Y[:, 1], -Y[:, 0]
        A[:, 0, 3] = A[:, 1, 4] = A[:, 2, 5] = 1.0
        A[:, :, 6] = Y
        B = np.zeros((n, 3, 7))   # [ [X1]x | -I | -X1 ]
        B[:, 0, 1], B[:, 0, 2], B[:, 1, 0] = -X1[:, 2], X1[:, 1], X1[:, 2]
        B[:, 1, 2], B[:, 2, 0], B[:, 2, 1] = -X1[:, 0], -X1[:, 1], X1[:, 0]
        B[:, 0, 3] = B[:, 1, 4] = B[:, 2, 5] = -1.0
        B[:, :, 6] = -X1
        Rts = q_to_mat(S[0]).T / S[2]
        J12 = -np.einsum("nij,njk->nik", project_jac(job["model1"], job["cam1"], Y), A)
        J21 = -np.einsum("nij,jk,nkl->nil", project_jac(job["model2"], job["cam2"], Z), Rts, B)
        if fix_scale:
            J12[:, :, 6] = 0.0
            J21[:, :, 6] = 0.0
    return J12, J21


def _huber(e2, delta):
    """RobustKernelHuber::robustify: (rho, rho')."""
    with np.errstate(all="ignore"):
        dsqr = delta * delta
        sq = np.sqrt(e2)
        small = e2 <= dsqr
        return np.where(small, e2, 2 * sq * delta - dsqr), np.where(small, 1.0, delta / sq)


def build_system(job, pre, S, active, robust, fix_scale, jac="analytic", proj="literal"):
    """computeActiveErrors + buildSystem: H [7][7], b [7], the robust chi2, and the per-pair chi2 (c12, c21)."""
    e12, e21 = errors(job, pre, S, proj)
    c12, c21 = chi2_of(pre, e12, e21)
    J12, J21 = jacobians(job, pre, S, fix_scale, jac, proj)
    H, b, chi = np.zeros((7, 7)), np.zeros(7), 0.0
    with np.errstate(all="ignore"):
        for e, c, J, w in ((e12, c12, J12, pre["w1"]), (e21, c21, J21, pre["w2"])):
            r0, r1 = _huber(c, pre["delta"]) if robust else (c, np.ones_like(c))
            a = active
            H += np.einsum("n,nri,nrj->ij", (w * r1)[a], J[a], J[a])
            b += np.einsum("nri,nr->i", J[a], (-w[:, None] * e * r1[:, None])[a])
            chi += r0[a].sum()
    return H, b, chi, c12, c21, e12, e21


def _lm(job, pre, S, x, active, robust, n_it, fix_scale, jac, proj, c12, c21, dbg):
    """optimize(n_it) of OptimizationAlgorithmLevenberg (its step control: lm_ref) on the active pairs.  c12 / c21: the
    edges' _error-derived chi2, updated in place by every computeActiveErrors (a rejected trial's included).  Returns
    (S, x)."""
    its = trials = 0
    lm = lm_ref.LmState()
    if not active.any():   # initializeOptimization finds no vertex: optimize() returns -1
        dbg["iterations"].append(0), dbg["trials"].append(0), dbg["max_trials"].append(0)
        return S, x
    max_trials = 0
    for it in range(n_it):
        H, b, chi, a12, a21, e12, e21 = build_system(job, pre, S, active, robust, fix_scale, jac, proj)
        c12[active], c21[active] = a12[active], a21[active]
        its += 1
        with np.errstate(all="ignore"):
            md = 0.0
            if it == 0:
                for j in range(7):
                    md = np.fmax(abs(H[j, j]), md)
            lm_ref.begin_iteration(lm, it, chi, lm_ref.lambda_init(0.0, md))
            if "H" not in dbg:
                dbg.update(H=H.copy(), b=b.copy(), chi2=chi, lambda_init=lm.lam, e12=e12.copy(), e21=e21.copy())
            while True:
                r = linalg_ref.ldlt_replay((H + lm.lam * np.eye(7)).tolist(), b.tolist(), num=float, looking="left")
                if r["ok"]:
                    x = np.array(r["x"], np.float64)
                if "x" not in dbg:
                    dbg["x"] = x.copy()
                St = oplus(S, x, fix_scale)
                t12, t21 = chi2_of(pre, *errors(job, pre, St, proj))
                c12[active], c21[active] = t12[active], t21[active]
                temp = 0.0
                for c in (t12, t21):
                    temp += (_huber(c, pre["delta"])[0] if robust else c)[active].sum()
                rho, accepted = lm_ref.trial(lm, temp, r["ok"], float((x * (lm.lam * x + b)).sum()))
                trials += 1
                if accepted:
                    S = St
                nxt = lm_ref.next_step(lm, rho, 10)
                if nxt != lm_ref.TRIAL:
                    break
            max_trials = max(max_trials, lm.qmax)
            if nxt == lm_ref.STOP:
                break
    dbg["iterations"].append(its), dbg["trials"].append(trials), dbg["max_trials"].append(max_trials)
    return S, x


def optimize_sim3(job, jac="analytic", proj="literal"):
    """Optimizer::OptimizeSim3 on one job.  Returns dict(n_in, q, t, s, status [N], H_acum (zero 7 x 7), dbg) with dbg:
    the first buildSystem (H, b, chi2, lambda_init, x of the first trial, e12, e21 [N][2] at the input), iterations /
    trials / max_trials per round, chi2_round1 (c12, c21: what the round-one test compared) and n_removed_1."""
    pre = prepare(job)
    n = len(pre["X1"])
    fix = bool(job["fix_scale"])
    S0 = start_of(job)
    S = S0
    status = np.zeros(n, np.uint8)
    active = pre["edge"].copy()
    c12, c21 = np.zeros(n), np.zeros(n)
    dbg = dict(iterations=[], trials=[], max_trials=[])
    e12, e21 = errors(job, pre, S0, proj)
    dbg["e12_0"], dbg["e21_0"] = e12, e21
    x = np.zeros(7)
    S, x = _lm(job, pre, S, x, active, True, 10, fix, jac, proj, c12, c21, dbg)
    with np.errstate(all="ignore"):
        bad = active & ((c12 > pre["th2"]) | (c21 > pre["th2"]))
    dbg["chi2_round1"] = (c12.copy(), c21.copy())
    n_corr, n_bad = int(active.sum()), int(bad.sum())
    dbg["n_removed_1"] = n_bad
    status[bad] = REMOVED_1
    active = active & ~bad
    out = dict(n_in=0, q=S0[0], t=S0[1], s=S0[2], status=status, H_acum=np.zeros((7, 7)), dbg=dbg, pre=pre)
    if n_corr - n_bad < 10:
        return out
    S, x = _lm(job, pre, S, x, active, False, 10 if n_bad > 0 else 5, fix, jac, proj, c12, c21, dbg)
    f12, f21 = chi2_of(pre, *errors(job, pre, S, proj))
    with np.errstate(all="ignore"):
        bad2 = active & ((f12 > pre["th2"]) | (f21 > pre["th2"]))
    status[active] = INLIER
    status[bad2] = REMOVED_2
    out.update(n_in=int((active & ~bad2).sum()), q=S[0], t=S[1], s=S[2])
    dbg["chi2_final"] = (f12, f21)
    return out
