"""Float64 numpy restatement of the two pose graphs of openmavis_amd/csrc/essgraph.hip: Optimizer::OptimizeEssentialGraph
(g2o::VertexSim3Expmap / EdgeSim3) and OptimizeEssentialGraph4DoF (VertexPose4DoF / Edge4DoF) -- g2o::Sim3's exp and log
branch for branch (Thirdparty/g2o/g2o/types/sim3.h:70-230), ImuCamPose::UpdateW, g2o's numeric Jacobians
(base_binary_edge.hpp:131-205: central difference, delta = 1e-9), a dense solve and the Levenberg-Marquardt of
tests/lm_ref.py.  `delta=1e-6` replaces the Jacobian's step: truncation (~1e-12) and rounding (~1e-10) are then both far
below the g2o form's rounding noise of ~1e-7 -- the "near-exact" run the GPU tests measure the reference's own spread
against.  Everything is batched over edges / vertices (leading axis)."""
import numpy as np

import lm_ref

SIM3, DOF4 = 0, 1
G2O_DELTA = 1e-9
EPS = 0.00001
INFO_4DOF = np.array([1e3, 1e3, 1.0, 1.0, 1.0, 1.0])   # (0, 0) set twice, (2, 2) never (Optimizer.cc:6241-6244)


# ---- quaternions (x y z w), Eigen's arithmetic ---------------------------------------------------------------------
def q_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def q_rot(q, v):
    u = 2 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * u + np.cross(q[..., :3], u)


def q_to_mat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def q_from_mat(R):
    """Eigen::Quaterniond(Matrix3d): the trace branch, or the branch of the largest diagonal entry."""
    R = np.asarray(R, np.float64)
    m = R.reshape(-1, 3, 3)
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    out = np.zeros((len(m), 4))
    with np.errstate(all="ignore"):
        t = np.sqrt(tr + 1.0)
        h = 0.5 / t
        out[:, 3] = 0.5 * t
        out[:, 0], out[:, 1], out[:, 2] = (m[:, 2, 1] - m[:, 1, 2]) * h, (m[:, 0, 2] - m[:, 2, 0]) * h, (m[:, 1, 0] - m[:, 0, 1]) * h
    big = np.where(m[:, 1, 1] > m[:, 0, 0], 1, 0)
    big = np.where(m[:, 2, 2] > m[np.arange(len(m)), big, big], 2, big)
    for n in np.flatnonzero(~(tr > 0)):
        i = int(big[n])
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[n, i, i] - m[n, j, j] - m[n, k, k] + 1.0)
        out[n, i] = 0.5 * t
        t = 0.5 / t
        out[n, 3] = (m[n, k, j] - m[n, j, k]) * t
        out[n, j] = (m[n, j, i] + m[n, i, j]) * t
        out[n, k] = (m[n, k, i] + m[n, i, k]) * t
    return out.reshape(R.shape[:-2] + (4,))


def hat(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).reshape(
        w.shape[:-1] + (3, 3))


# ---- g2o::Sim3 as an [..., 8] array: q (x y z w), t, s ---------------------------------------------------------------
def s_mul(a, b):
    return np.concatenate([q_mul(a[..., :4], b[..., :4]), a[..., 7:8] * q_rot(a[..., :4], b[..., 4:7]) + a[..., 4:7],
                           a[..., 7:8] * b[..., 7:8]], -1)


def s_inv(a):
    qc = a[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([qc, q_rot(qc, (-1.0 / a[..., 7:8]) * a[..., 4:7]), 1.0 / a[..., 7:8]], -1)


def s_map(a, X):
    return a[..., 7:8] * q_rot(a[..., :4], X) + a[..., 4:7]


def _abc(sigma, theta, s, small_theta):
    """A, B, C of Sim3(update) and Sim3::log in their four branches (sim3.h:92-135, :169-213)."""
    small_sigma = np.abs(sigma) < EPS
    with np.errstate(all="ignore"):
        th2, sg2 = theta * theta, sigma * sigma
        C = np.where(small_sigma, 1.0, (s - 1) / sigma)
        A00, B00 = 0.5, 1.0 / 6.0
        A01 = (1 - np.cos(theta)) / th2
        B01 = (theta - np.sin(theta)) / (th2 * theta)
        A10 = ((sigma - 1) * s + 1) / sg2
        B10 = ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), th2 + sg2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / th2
    A = np.where(small_sigma, np.where(small_theta, A00, A01), np.where(small_theta, A10, A11))
    B = np.where(small_sigma, np.where(small_theta, B00, B01), np.where(small_theta, B10, B11))
    return A, B, C


def sim3_exp(u):
    """Sim3(const Vector7d &update) (sim3.h:70-142); the small-angle rotation is I + Omega + Omega^2, not the series."""
    u = np.asarray(u, np.float64)
    omega, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt(np.sum(omega * omega, -1))
    O = hat(omega)
    O2 = O @ O
    s = np.exp(sigma)
    small = theta < EPS
    I = np.eye(3)
    with np.errstate(all="ignore"):
        Rb = I + (np.sin(theta) / theta)[..., None, None] * O + ((1 - np.cos(theta)) / (theta * theta))[..., None, None] * O2
    R = np.where(small[..., None, None], I + O + O2, Rb)
    A, B, C = _abc(sigma, theta, s, small)
    W = A[..., None, None] * O + B[..., None, None] * O2 + C[..., None, None] * I
    return np.concatenate([q_from_mat(R), np.einsum("...ij,...j->...i", W, ups), s[..., None]], -1)


def sim3_log(S):
    """Sim3::log (sim3.h:148-230); upsilon = W.lu().solve(t)."""
    S = np.asarray(S, np.float64)
    sigma = np.log(S[..., 7])
    R = q_to_mat(S[..., :4])
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small = d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.arccos(np.where(small, 0.0, d))
        f = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))
    omega = f[..., None] * dR
    A, B, C = _abc(sigma, theta, S[..., 7], small)
    O = hat(omega)
    W = A[..., None, None] * O + (B[..., None, None] * O) @ O + C[..., None, None] * np.eye(3)
    ups = np.linalg.solve(W, S[..., 4:7, None])[..., 0]
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def sim3_matrix(S):
    """[sR t; 0 1]."""
    M = np.zeros(S.shape[:-1] + (4, 4))
    M[..., :3, :3] = S[..., 7, None, None] * q_to_mat(S[..., :4] / np.linalg.norm(S[..., :4], axis=-1, keepdims=True))
    M[..., :3, 3] = S[..., 4:7]
    M[..., 3, 3] = 1
    return M


# ---- SO3 helpers of G2oTypes.cc --------------------------------------------------------------------------------------
def normalize_rotation(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def exp_so3(w):
    d2 = np.sum(w * w, -1)
    d = np.sqrt(d2)
    W = hat(w)
    with np.errstate(all="ignore"):
        big = np.eye(3) + W * (np.sin(d) / d)[..., None, None] + (W @ W) * ((1.0 - np.cos(d)) / d2)[..., None, None]
    res = np.where((d < 1e-5)[..., None, None], np.eye(3) + W + 0.5 * (W @ W), big)
    return normalize_rotation(res)


def log_so3(R):
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    w = np.stack([(R[..., 2, 1] - R[..., 1, 2]) / 2, (R[..., 0, 2] - R[..., 2, 0]) / 2, (R[..., 1, 0] - R[..., 0, 1]) / 2], -1)
    c = (tr - 1.0) * 0.5
    inside = (c <= 1) & (c >= -1)
    with np.errstate(all="ignore"):
        theta = np.arccos(np.where(inside, c, 1.0))
        s = np.sin(theta)
        scaled = theta[..., None] * w / s[..., None]
    return np.where((inside & (np.abs(s) >= 1e-5))[..., None], scaled, w)


# ---- the two kinds -----------------------------------------------------------------------------------------------
class Kind:
    def __init__(self, prob):
        self.fixed = np.asarray(prob["fixed"]).astype(bool)
        self.ei, self.ej = np.asarray(prob["edge_i"], np.int64), np.asarray(prob["edge_j"], np.int64)
        tab = np.stack([np.asarray(prob["S_a"], np.float64), np.asarray(prob["S_b"], np.float64)])
        t = np.asarray(prob["edge_table"], np.int64)
        self.Si_t, self.Sj_t = tab[t, self.ei], tab[t, self.ej]
        self.S_a = tab[0]


class Sim3Kind(Kind):
    V, D = 7, 7
    info = np.ones(7)
    lambda_user = 1e-16   # setUserLambdaInit (Optimizer.cc:1846)

    def __init__(self, prob):
        super().__init__(prob)
        self.fix_scale = bool(prob.get("fix_scale", 0))
        self.meas = s_mul(self.Sj_t, s_inv(self.Si_t))   # C = S_table[j] S_table[i]^-1
        self.state0 = np.array(prob["vertices"], np.float64)

    def oplus(self, x, u, n_acc=0):
        u = np.array(u, np.float64)
        if self.fix_scale:
            u[..., 6] = 0
        return s_mul(sim3_exp(u), x), u

    def error(self, xi, xj):
        return sim3_log(s_mul(s_mul(self.meas, xi), s_inv(xj)))

    def caller_vertices(self, x):
        return x.copy()

    def as_sim3(self, x):
        return x


class Dof4Kind(Kind):
    V, D = 4, 6
    info = INFO_4DOF
    lambda_user = 0.0     # computeLambdaInit

    def __init__(self, prob):
        super().__init__(prob)
        Sij = s_mul(self.Si_t, s_inv(self.Sj_t))         # S_table[i] S_table[j]^-1, the scale dropped
        self.dR, self.dt = q_to_mat(Sij[..., :4]), Sij[..., 4:7]
        self.meas = np.concatenate([self.dR.reshape(-1, 9), self.dt], -1)
        v = np.asarray(prob["vertices"], np.float64)
        n = len(v)
        self.Rcb, self.tcb = np.asarray(prob["Rcb"], np.float64).reshape(3, 3), np.asarray(prob["tcb"], np.float64)
        self.Rwb0 = v[:, 12:21].reshape(n, 3, 3)
        # state: DR | Rwb | twb | Rcw | tcw
        self.state0 = np.concatenate([np.tile(np.eye(3).reshape(1, 9), (n, 1)), v[:, 12:21], v[:, 21:24], v[:, 0:9], v[:, 9:12]], -1)

    def oplus(self, x, u, n_acc=0, rwb0=None):
        """ImuCamPose::UpdateW((0, 0, u0, u1, u2, u3)); n_acc % 5 == 4: the fifth kept update normalises DR."""
        u = np.asarray(u, np.float64)
        Rwb0 = self.Rwb0 if rwb0 is None else rwb0
        ur = np.zeros(u.shape[:-1] + (3,))
        ur[..., 2] = u[..., 0]
        DR = exp_so3(ur) @ x[..., 0:9].reshape(x.shape[:-1] + (3, 3))
        Rwb = DR @ Rwb0
        twb = x[..., 18:21] + u[..., 1:4]
        if n_acc % 5 == 4:
            DR = DR.copy()
            DR[..., 0, 2] = DR[..., 1, 2] = DR[..., 2, 0] = DR[..., 2, 1] = 0.0
            DR = normalize_rotation(DR)
        Rbw = np.swapaxes(Rwb, -1, -2)
        tbw = -np.einsum("...ij,...j->...i", Rbw, twb)
        Rcw = self.Rcb @ Rbw
        tcw = np.einsum("ij,...j->...i", self.Rcb, tbw) + self.tcb
        sh = x.shape[:-1]
        return np.concatenate([DR.reshape(sh + (9,)), Rwb.reshape(sh + (9,)), twb, Rcw.reshape(sh + (9,)), tcw], -1), u

    def error(self, xi, xj, sel=slice(None)):
        Ri, ti = xi[..., 21:30].reshape(xi.shape[:-1] + (3, 3)), xi[..., 30:33]
        Rj, tj = xj[..., 21:30].reshape(xj.shape[:-1] + (3, 3)), xj[..., 30:33]
        Rjt = np.swapaxes(Rj, -1, -2)
        er = log_so3(Ri @ Rjt @ np.swapaxes(self.dR[sel], -1, -2))
        et = np.einsum("...ij,...j->...i", Ri, -np.einsum("...ij,...j->...i", Rjt, tj)) + ti - self.dt[sel]
        return np.concatenate([er, et], -1)

    def caller_vertices(self, x):
        return np.concatenate([x[:, 21:30], x[:, 30:33], x[:, 9:18], x[:, 18:21]], -1)

    def as_sim3(self, x):
        """g2o::Sim3(Rcw, tcw, 1.) (Optimizer.cc:6446)."""
        return np.concatenate([q_from_mat(x[:, 21:30].reshape(-1, 3, 3)), x[:, 30:33], np.ones((len(x), 1))], -1)


def make_kind(kind, prob):
    return Sim3Kind(prob) if kind == SIM3 else Dof4Kind(prob)


def errors(K, x):
    return K.error(x[K.ei], x[K.ej])


def chi2_edges(K, e):
    return np.sum(e * (K.info * e), -1)


def jacobians(K, x, delta=G2O_DELTA):
    """linearizeOplus of every edge: (Ji, Jj) [E][D][V]; a fixed vertex's block is zero."""
    E = len(K.ei)
    J = [np.zeros((E, K.D, K.V)), np.zeros((E, K.D, K.V))]
    scalar = 1.0 / (2 * delta)
    for side, idx in ((0, K.ei), (1, K.ej)):
        for d in range(K.V):
            ev = []
            for sign in (1.0, -1.0):
                u = np.zeros((E, K.V))
                u[:, d] = sign * delta
                if isinstance(K, Dof4Kind):
                    moved, _ = K.oplus(x[idx], u, 0, K.Rwb0[idx])
                else:
                    moved, _ = K.oplus(x[idx], u)
                ev.append(K.error(moved, x[K.ej]) if side == 0 else K.error(x[K.ei], moved))
            J[side][:, :, d] = scalar * (ev[0] - ev[1])
        J[side][K.fixed[idx]] = 0.0
    return J[0], J[1]


def layout(K):
    """Rows of the solver's system: optimisable vertices in caller order, 16 // V per 16-row block."""
    per = 16 // K.V
    opt = np.flatnonzero(~K.fixed)
    row = np.full(len(K.fixed), -1, np.int64)
    o = np.arange(len(opt))
    row[opt] = 16 * (o // per) + K.V * (o % per)
    nb = (len(opt) + per - 1) // per
    real = np.zeros(16 * nb, bool)
    for r in row[opt]:
        real[r:r + K.V] = True
    return opt, row, nb, real


def build_system(K, x, delta=G2O_DELTA):
    """(H, b, chi2 per edge, e, Ji, Jj) in the solver's layout; pad rows: diagonal 1, zero right-hand side."""
    opt, row, nb, real = layout(K)
    e = errors(K, x)
    Ji, Jj = jacobians(K, x, delta)
    n = 16 * nb
    H, b = np.zeros((n, n)), np.zeros(n)
    for k in range(len(K.ei)):
        Js = (Ji[k], Jj[k])
        rows = (row[K.ei[k]], row[K.ej[k]])
        for a in range(2):
            if rows[a] < 0:
                continue
            b[rows[a]:rows[a] + K.V] += Js[a].T @ (-(K.info * e[k]))
            for c in range(2):
                if rows[c] < 0:
                    continue
                H[rows[a]:rows[a] + K.V, rows[c]:rows[c] + K.V] += (Js[a].T * K.info) @ Js[c]
    pad = np.flatnonzero(~real)
    H[pad, pad] = 1.0
    return H, b, chi2_edges(K, e), e, Ji, Jj


def solve_damped(K, H, b, lam):
    _, _, _, real = layout(K)
    A = H + np.diag(np.where(real, lam, 0.0))
    with np.errstate(all="ignore"):
        try:
            x = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            return np.zeros_like(b), False
    return x, bool(np.all(np.isfinite(x)))


def optimize(kind, prob, iterations=20, max_trials=10, delta=G2O_DELTA, log=None):
    """g2o's optimize(iterations): dict(err, err_end, iterations, trials, lambda_, vertices, state, n_acc)."""
    K = make_kind(kind, prob)
    opt, row, nb, real = layout(K)
    x = K.state0.copy()
    s = lm_ref.LmState()
    chi0 = float(np.sum(chi2_edges(K, errors(K, x))))
    res = dict(err=chi0, iterations=0, trials=0)
    n_acc, cur_chi, stop = 0, chi0, False
    for it in range(iterations):
        H, b, c2, _, _, _ = build_system(K, x, delta)
        cur_chi = float(np.sum(c2))
        res["iterations"] += 1
        lm_ref.begin_iteration(s, it, cur_chi, lm_ref.lambda_init(K.lambda_user, np.max(np.abs(np.diag(H))[real])))
        while True:
            dx, ok = solve_damped(K, H, b, s.lam)
            xt = x.copy()
            u_all = np.stack([dx[r:r + K.V] for r in row[opt]])
            if isinstance(K, Dof4Kind):
                xt[opt], u_used = K.oplus(x[opt], u_all, n_acc, K.Rwb0[opt])
            else:
                xt[opt], u_used = K.oplus(x[opt], u_all)
            rows = np.concatenate([np.arange(r, r + K.V) for r in row[opt]])
            scale = float(np.sum(u_used.reshape(-1) * (s.lam * u_used.reshape(-1) + b[rows])))
            with np.errstate(all="ignore"):
                chi = float(np.sum(chi2_edges(K, errors(K, xt))))
            rho, accepted = lm_ref.trial(s, chi, ok, scale if ok else 0.0)
            res["trials"] += 1
            if log is not None:
                log.append(dict(it=it, lam=s.lam, chi=chi, rho=rho, accepted=accepted))
            if accepted:
                x, n_acc, cur_chi = xt, n_acc + 1, chi
            nxt = lm_ref.next_step(s, rho, max_trials)
            if nxt != lm_ref.TRIAL:
                stop = nxt == lm_ref.STOP
                break
        if stop:
            break
    res.update(err_end=cur_chi, lambda_=s.lam, vertices=K.caller_vertices(x), state=x, n_acc=n_acc)
    return res


# ---- the epilogue ------------------------------------------------------------------------------------------------
def _quat_normalize(q):
    n2 = (q[..., 0] * q[..., 0] + q[..., 2] * q[..., 2]) + (q[..., 1] * q[..., 1] + q[..., 3] * q[..., 3])
    return q / np.sqrt(n2)[..., None]


def recover(kind, prob, state, mode, points=None, point_ref=None):
    """The SE3f of SetPose per vertex ([n][7] float32) and the corrected points (float32); mode 'loop' | 'merge' | '4dof'."""
    K = make_kind(kind, prob)
    S = K.as_sim3(np.asarray(state, np.float64))
    if mode == "loop":
        qf = _quat_normalize(S[:, :4].astype(np.float32))
        tf = S[:, 4:7].astype(np.float32) / S[:, 7:8].astype(np.float32)
        poses = np.concatenate([qf, tf], -1).astype(np.float32)
    else:
        q = _quat_normalize(S[:, :4])
        t = S[:, 4:7] / S[:, 7:8] if mode == "merge" else S[:, 4:7]
        poses = np.concatenate([q, t], -1).astype(np.float32)
    pts = None
    if points is not None:
        pts = np.array(points, np.float32)
        ref = np.asarray(point_ref, np.int64)
        m = ref >= 0
        P = pts[m].astype(np.float64)
        pts[m] = s_map(s_inv(S[ref[m]]), s_map(K.S_a[ref[m]], P)).astype(np.float32)
    return poses, pts
