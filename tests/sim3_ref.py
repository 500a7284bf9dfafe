"""Reference for the device Sim3Solver (src/Sim3Solver.cc): a float64 numpy restatement of the whole solver on the same
float32 inputs -- the camera-frame transform and projection, Horn's closed form through numpy.linalg.eigh, CheckInliers,
the sequential iterate state machine, the sampling replay and SetRansacParameters -- and a float32 restatement of
ComputeSim3 (numpy float32 operations in the reference's order, the eigenvector taken in float64 from the
float32-rounded N), whose error against the float64 result is the e_ref of tests/test_sim3solver_gpu.py.

A job is a dict: Xw1, Xw2 [N][3] float32, sigma2_1, sigma2_2 [N] float32, index1 [N] int32, mN1, pose1, pose2 [12]
(Riw row-major, tiw), cam1, cam2 [8], model1, model2 (0 KB8, 1 Pinhole), fix_scale."""
import numpy as np

import ransac_ref

U32 = 2.0 ** -24
NO_MORE, CONVERGE = 1, 2


# ---- SetRansacParameters (:184-207) -------------------------------------------------------------------------------
def ransac_max_its(prob, min_inliers, n, max_its):
    """mRansacMaxIts: epsilon = (float)mRansacMinInliers / N, then the shared tail."""
    return ransac_ref.ransac_its(prob, np.float32(min_inliers) / np.float32(n), min_inliers == n, max_its)


# ---- the sampling of iterate (:230-243) --------------------------------------------------------------------------
def sample_literal(n, r):
    """The three picks by the literal shrinking list; the draws must be in range."""
    assert all(0 <= r[i] <= n - 1 - i for i in range(3))
    return ransac_ref.sample_literal(n, r, 3)


def sample_replay(n, r):
    """The same picks as the device evaluates them."""
    return ransac_ref.sample_replay(n, r, 3)


# ---- cameras, float64 ------------------------------------------------------------------------------------------
def project(model, k, X):
    """GeometricCamera::project for [n][3] points -> [n][2]; float64 on float32 parameters."""
    k = np.asarray(k, np.float64)
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        if model == 1:
            return np.stack([k[0] * X[:, 0] / X[:, 2] + k[2], k[1] * X[:, 1] / X[:, 2] + k[3]], 1)
        th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
        psi = np.arctan2(X[:, 1], X[:, 0])
        r = th + k[4] * th ** 3 + k[5] * th ** 5 + k[6] * th ** 7 + k[7] * th ** 9
        return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def prepare(job):
    """The constructor's numeric part (:119-179): X3Dc1/2, mvP1im1 / mvP2im2 and the size_t thresholds."""
    p1, p2 = np.asarray(job["pose1"], np.float64), np.asarray(job["pose2"], np.float64)
    X1 = np.asarray(job["Xw1"], np.float64).reshape(-1, 3) @ p1[:9].reshape(3, 3).T + p1[9:]
    X2 = np.asarray(job["Xw2"], np.float64).reshape(-1, 3) @ p2[:9].reshape(3, 3).T + p2[9:]
    e1 = np.floor(9.210 * np.asarray(job["sigma2_1"], np.float32).astype(np.float64))
    e2 = np.floor(9.210 * np.asarray(job["sigma2_2"], np.float32).astype(np.float64))
    return dict(X1=X1, X2=X2, P1=project(job["model1"], job["cam1"], X1), P2=project(job["model2"], job["cam2"], X2),
                e1=e1, e2=e2)


# ---- ComputeSim3 (:360-457) ----------------------------------------------------------------------------------------
def _n_matrix(M):
    N11 = M[0, 0] + M[1, 1] + M[2, 2]
    N12, N13, N14 = M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
    N22 = M[0, 0] - M[1, 1] - M[2, 2]
    N23, N24 = M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
    N33 = -M[0, 0] + M[1, 1] - M[2, 2]
    N34 = M[1, 2] + M[2, 1]
    N44 = -M[0, 0] - M[1, 1] + M[2, 2]
    return np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], M.dtype)


def _quat_to_R(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def compute_sim3_64(P1, P2, fix_scale):
    """P1, P2 [3][3], column i = the i-th sampled X3Dc1 / X3Dc2 (float32 values) -> R, s, t, T12, T21 in float64 and
    kappa = |Pr1|_F |Pr2|_F / (lambda_1 - lambda_2) from eigh's eigenvalues."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.sum(1) / 3, P2.sum(1) / 3
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    with np.errstate(all="ignore"):
        lam, vec = np.linalg.eigh(_n_matrix(Pr2 @ Pr1.T))
        R = _quat_to_R(vec[:, 3])
        P3 = R @ Pr2
        s = 1.0 if fix_scale else (Pr1 * P3).sum() / (P3 * P3).sum()
        t = O1 - s * R @ O2
        T12, T21 = np.eye(4), np.eye(4)
        T12[:3, :3], T12[:3, 3] = s * R, t
        T21[:3, :3] = R.T / s
        T21[:3, 3] = -T21[:3, :3] @ t
        kappa = np.linalg.norm(Pr1) * np.linalg.norm(Pr2) / (lam[3] - lam[2])
    return dict(R=R, s=np.float64(s), t=t, T12=T12, T21=T21, kappa=kappa)


def _mv3_f32(A, x):
    """Eigen's fixed-size product in float: each coefficient a 3-term sum, left to right."""
    return np.array([(A[i, 0] * x[0] + A[i, 1] * x[1]) + A[i, 2] * x[2] for i in range(3)], np.float32)


def _so3_exp_f32(w):
    """Sophus::SO3f::exp(omega).matrix() in float32."""
    f = np.float32
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th2 < f(1e-10):   # Constants<float>::epsilon() squared
        imag, real = f(0.5) - f(1 / 48) * th2, f(1) - f(1 / 8) * th2
    else:
        half = f(0.5) * th
        imag, real = np.sin(half) / th, np.cos(half)
    x, y, z, qw = imag * w[0], imag * w[1], imag * w[2], real
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z   # Eigen::Quaternion::toRotationMatrix
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[f(1) - (tyy + tzz), txy - twz, txz + twy], [txy + twz, f(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, f(1) - (txx + tyy)]], np.float32)


def compute_sim3_32(P1, P2, fix_scale):
    """ComputeSim3 in numpy float32 operations in the reference's order; the eigenvector of the float32-rounded N in
    float64 (numpy.linalg.eigh), then atan2, the angle-axis vector and SO3f::exp in float32."""
    f = np.float32
    P1, P2 = np.asarray(P1, f), np.asarray(P2, f)
    with np.errstate(all="ignore"):
        O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / f(3)
        O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / f(3)
        Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
        M = np.array([[(Pr2[i, 0] * Pr1[j, 0] + Pr2[i, 1] * Pr1[j, 1]) + Pr2[i, 2] * Pr1[j, 2] for j in range(3)]
                      for i in range(3)], f)
        N = _n_matrix(M)
        lam, vec = np.linalg.eigh(N.astype(np.float64))
        evec = vec[:, 3].astype(f)
        v = evec[1:4]
        nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ang = np.arctan2(np.float64(nv), np.float64(evec[0]))
        if nv != 0:
            v = (f(2 * ang) * v) / nv
        R = _so3_exp_f32(v)
        P3 = np.stack([_mv3_f32(R, Pr2[:, j]) for j in range(3)], 1)
        if fix_scale:
            s = f(1)
        else:
            nom, den = f(0), f(0)
            for j in range(3):
                for i in range(3):
                    nom = nom + Pr1[i, j] * P3[i, j]
                    den = den + P3[i, j] * P3[i, j]
            s = f(np.float64(nom) / np.float64(den))
        sR = s * R
        t = O1 - _mv3_f32(sR, O2)
        T12, T21 = np.eye(4, dtype=f), np.eye(4, dtype=f)
        T12[:3, :3], T12[:3, 3] = sR, t
        sRinv = f(1.0 / np.float64(s)) * R.T
        T21[:3, :3], T21[:3, 3] = sRinv, _mv3_f32(-sRinv, t)
    return dict(R=R, s=s, t=t, T12=T12, T21=T21)


# ---- CheckInliers (:459-479) ----------------------------------------------------------------------------------------
def reprojection_errors(job, pre, T12, T21):
    """err1, err2 [N] in float64 for the given transforms."""
    T12, T21 = np.asarray(T12, np.float64).reshape(4, 4), np.asarray(T21, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        q1 = project(job["model1"], job["cam1"], pre["X2"] @ T12[:3, :3].T + T12[:3, 3])
        q2 = project(job["model2"], job["cam2"], pre["X1"] @ T21[:3, :3].T + T21[:3, 3])
        return ((pre["P1"] - q1) ** 2).sum(1), ((q2 - pre["P2"]) ** 2).sum(1)


def check_inliers(job, pre, T12, T21):
    with np.errstate(all="ignore"):
        err1, err2 = reprojection_errors(job, pre, T12, T21)
        return (err1 < pre["e1"]) & (err2 < pre["e2"])   # False for a NaN


# ---- iterate (:273-346) as a state machine -------------------------------------------------------------------------
def new_state(n, min_inliers, max_its):
    """The carried members after the constructor and SetRansacParameters; `flags` is sticky once a job is finished.
    N < mRansacMinInliers is iterate's entry test; N < 3 (undefined in the reference) is treated the same way."""
    return dict(iterations=0, best_inliers=0, best=None, flags=NO_MORE if (n < min_inliers or n < 3) else 0,
                min_inliers=min_inliers, max_its=max_its, n_inliers=0)


def select(state, counts, n_iterations):
    """Apply one iterate(n_iterations) call to `state` given the inlier counts of the chunk's hypotheses in order.
    Returns the chosen hypothesis of the call (the one copied into mBest*, None if none) and the chunk length."""
    if state["flags"]:
        return None, 0
    chunk = min(n_iterations, state["max_its"] - state["iterations"])
    chosen, converged = None, False
    for h in range(chunk):
        state["iterations"] += 1
        if counts[h] >= state["best_inliers"]:
            state["best_inliers"] = int(counts[h])
            chosen = h
            if counts[h] > state["min_inliers"]:
                converged = True
                break
    if converged:
        state["flags"] = CONVERGE
        state["n_inliers"] = state["best_inliers"]
    elif state["iterations"] >= state["max_its"]:
        state["flags"] = NO_MORE
    return chosen, chunk


class RefSolver:
    """One job's Sim3Solver in float64: SetRansacParameters, iterate (5-argument form, with the device's documented
    return value: the carried mBestT12 where the reference returns an uninitialised matrix) and find."""

    def __init__(self, job):
        self.job, self.pre, self.n = job, prepare(job), len(job["index1"])
        self.SetRansacParameters()

    def SetRansacParameters(self, prob=0.99, min_inliers=6, max_its=300):
        self.max_its = ransac_max_its(prob, min_inliers, self.n, max_its) if self.n else 1
        self.state = new_state(self.n, min_inliers, self.max_its)
        self.best = dict(T12=np.eye(4), R=np.eye(3), t=np.zeros(3), s=1.0, mask=np.zeros(self.n, bool))

    def hypothesis(self, r):
        idx = sample_replay(self.n, r)
        h = compute_sim3_64(self.pre["X1"][idx].T, self.pre["X2"][idx].T, self.job["fix_scale"])
        h["idx"], h["mask"] = idx, check_inliers(self.job, self.pre, h["T12"], h["T21"])
        return h

    def iterate(self, n_iterations, draws):
        """draws [n_iterations][3] raw RandomInt values.  Returns (T12, bNoMore, vbInliers [mN1], nInliers, bConverge)."""
        vb = np.zeros(self.job["mN1"], bool)
        st = self.state
        if not st["flags"]:   # the reference's loop as written (select() is the same rule on given counts)
            k = 0
            while st["iterations"] < self.max_its and k < n_iterations:
                h = self.hypothesis(draws[k])
                k += 1
                st["iterations"] += 1
                count = int(h["mask"].sum())
                if count >= st["best_inliers"]:
                    st["best_inliers"], self.best = count, h
                    if count > st["min_inliers"]:
                        st["flags"], st["n_inliers"] = CONVERGE, count
                        break
            if not st["flags"] and st["iterations"] >= self.max_its:
                st["flags"] = NO_MORE
        conv = bool(st["flags"] & CONVERGE)
        if conv:
            vb[np.asarray(self.job["index1"])[self.best["mask"]]] = True
        return self.best["T12"], bool(st["flags"] & NO_MORE), vb, st["n_inliers"] if conv else 0, conv

    def find(self, draws):
        T, _, vb, n, conv = self.iterate(self.max_its, draws)
        return (T if conv else np.eye(4)), vb, n
