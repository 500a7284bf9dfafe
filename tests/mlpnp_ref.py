"""Reference for the device MLPnPsolver (src/MLPnPsolver.cpp): a float64 numpy restatement of the whole solver on the
same float32 inputs -- the constructor's bearings and Householder nullspaces, SetRansacParameters, the sampling replay,
computePose (planarity by a literal FullPivHouseholderQR, the design matrix, numpy.linalg.svd / eigh for the
decompositions, the two sign / scale selections, the Gauss-Newton with the compact Jacobian), CheckInliers, Refine and
the sequential iterate state machine with the kept Refine outcome.

A job is a dict: P2D [N][2] float32, sigma2 [N] float32, Xw [N][3] float32, index [N] int32, mN, cam [8], model (0 KB8,
1 Pinhole).  compute_pose also reports what tests/test_mlpnp_gpu.py needs to judge a comparison: the conditioning kappa
and whether one of its decisions fell within 2^-20 (relative) of its threshold."""
import math

import numpy as np

import ransac_ref
from sim3_ref import project

NO_MORE, FOUND = 1, 2
EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
GN_MAXIT, GN_EPSP, GN_BREAK, GN_NAN = 0, 1, 2, 3
NEAR = 2.0 ** -20
DEFAULTS = (0.99, 8, 300, 6, 0.4, 5.991)     # include/MLPnPsolver.h:19-25
TRACKING = (0.99, 10, 300, 6, 0.5, 5.991)    # src/Tracking.cc Relocalization


# ---- SetRansacParameters (:177-218) --------------------------------------------------------------------------------
def ransac_parameters(n, prob=0.99, min_inliers=8, max_its=300, min_set=6, epsilon=0.4):
    """(mRansacMaxIts, mRansacMinInliers) in the reference's types: the float product N * epsilon truncated, float
    epsilon, double pow / log / ceil.  A NaN or out-of-range double -> int conversion (undefined in C++, INT_MIN on
    x86) counts as INT_MIN."""
    n_min = int(np.float32(n) * np.float32(epsilon))
    n_min = max(n_min, min_inliers, min_set)
    with np.errstate(all="ignore"):
        eps = max(np.float32(epsilon), np.float32(n_min) / np.float32(n))
    return ransac_ref.ransac_its(prob, eps, n_min == n, max_its), n_min


# ---- the sampling of iterate (:79-98) ------------------------------------------------------------------------------
def sample_literal(n, r, k=6):
    return ransac_ref.sample_literal(n, r, k)


def sample_replay(n, r, k=6):
    return ransac_ref.sample_replay(n, r, k)


# ---- the constructor (:28-45) --------------------------------------------------------------------------------------
def bearings(job):
    """cam_unproject_f(P2D) / z in float32, widened: z = 1, not unit length.  KannalaBrandt8::unproject's Newton in
    numpy float32 (the device's differs by the rounding of its tanf restatement)."""
    k = np.asarray(job["cam"], np.float32)
    p = np.asarray(job["P2D"], np.float32).reshape(-1, 2)
    one = np.float32(1)
    pw = np.stack([(p[:, 0] - k[2]) / k[0], (p[:, 1] - k[3]) / k[1]], 1).astype(np.float32)
    scale = np.ones(len(p), np.float32)
    if job["model"] == 0:
        for i in range(len(p)):
            td = np.float32(np.sqrt(pw[i, 0] * pw[i, 0] + pw[i, 1] * pw[i, 1]))
            td = np.float32(min(max(np.float32(-math.pi / 2), td), np.float32(math.pi / 2)))
            if float(td) > 1e-8:
                th = td
                for _ in range(10):
                    t2 = th * th
                    t4 = t2 * t2
                    t6, t8 = t4 * t2, t4 * t4
                    a, b, c, d = k[4] * t2, k[5] * t4, k[6] * t6, k[7] * t8
                    fix = np.float32((th * (one + a + b + c + d) - td) /
                                     (one + np.float32(3) * a + np.float32(5) * b + np.float32(7) * c + np.float32(9) * d))
                    th = np.float32(th - fix)
                    if abs(fix) < np.float32(1e-6):
                        break
                scale[i] = np.float32(np.tan(th)) / td
    ray = np.stack([pw[:, 0] * scale, pw[:, 1] * scale, np.ones(len(p), np.float32)], 1).astype(np.float32)
    return (ray / ray[:, 2:3]).astype(np.float64)


def householder_nullspace(f):
    """Columns 1 and 2 of V of JacobiSVD<MatrixXd, HouseholderQRPreconditioner>(f^T, ComputeFullV) (:325-328): the
    reflector makeHouseholder builds for f."""
    f = np.asarray(f, np.float64)
    c0, tail_sq = f[0], f[1] * f[1] + f[2] * f[2]
    v = np.array([1.0, 0.0, 0.0])
    if tail_sq <= DBL_MIN:
        tau = 0.0
    else:
        beta = math.sqrt(c0 * c0 + tail_sq)
        if c0 >= 0:
            beta = -beta
        v[1:] = f[1:] / (c0 - beta)
        tau = (beta - c0) / beta
    H = np.eye(3) - tau * np.outer(v, v)
    return H[:, 1:3].copy()


def prepare(job, th2=5.991, bearing=None):
    """f [N][3], nullspaces [N][3][2], Xw [N][3] (float64) and mvMaxError = sigma2 * th2 in float32.  `bearing`: the
    device's bearings (omv_pnp_debug) in place of this file's float32 restatement."""
    f = bearings(job) if bearing is None else np.asarray(bearing, np.float64)
    ns = np.stack([householder_nullspace(x) for x in f]) if len(f) else np.zeros((0, 3, 2))
    return dict(f=f, ns=ns, Xw=np.asarray(job["Xw"], np.float32).astype(np.float64).reshape(-1, 3),
                P2D=np.asarray(job["P2D"], np.float32).astype(np.float64).reshape(-1, 2),
                max_err=(np.asarray(job["sigma2"], np.float32) * np.float32(th2)).astype(np.float64))


# ---- computePose (:306-617) ----------------------------------------------------------------------------------------
class _Decisions:
    """Collects how close each decision of a computePose came to its threshold."""

    def __init__(self):
        self.near = False

    def cmp(self, a, b):
        with np.errstate(all="ignore"):
            if np.isfinite(a) and np.isfinite(b) and abs(a - b) <= NEAR * max(abs(a), abs(b)):
                self.near = True


def fullpiv_rank3(M, dec=None):
    """FullPivHouseholderQR<Matrix3d>(M).rank() with the default threshold, literally (computeInPlace / rank)."""
    m = np.array(M, np.float64)
    prec = 3.0 * EPS
    maxpivot = biggest = 0.0
    nonzero = 3
    for k in range(3):
        row = col = k
        big = abs(m[k, k])
        for c in range(k, 3):          # maxCoeff visits the column-major block, the first maximum wins
            for r in range(k, 3):
                if abs(m[r, c]) > big:
                    big, row, col = abs(m[r, c]), r, c
        if k == 0:
            biggest = big
        if dec is not None:
            dec.cmp(big, biggest * prec)
        if big <= biggest * prec:
            nonzero = k
            break
        m[[k, row], k:] = m[[row, k], k:]
        m[:, [k, col]] = m[:, [col, k]]
        c0 = m[k, k]
        tail = m[k + 1:, k].copy()
        tail_sq = float(tail @ tail)
        if tail_sq <= DBL_MIN:
            tau, beta, ess = 0.0, c0, np.zeros(len(tail))
        else:
            beta = math.sqrt(c0 * c0 + tail_sq)
            if c0 >= 0:
                beta = -beta
            ess = tail / (c0 - beta)
            tau = (beta - c0) / beta
        m[k, k] = beta
        maxpivot = max(maxpivot, abs(beta))
        for c in range(k + 1, 3):
            s = m[k, c] + ess @ m[k + 1:, c]
            m[k, c] -= tau * s
            m[k + 1:, c] -= tau * ess * s
    rank = 0
    for i in range(nonzero):
        if dec is not None:
            dec.cmp(abs(m[i, i]), maxpivot * prec)
        rank += abs(m[i, i]) > maxpivot * prec
    return rank


def rodrigues2rot(w):
    w = np.asarray(w, np.float64)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    n = math.sqrt(w @ w) if np.isfinite(w).all() else float("nan")
    R = np.eye(3)
    if n > EPS:
        R = R + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):
    w = np.zeros(3)
    trace = np.trace(R) - 1.0
    with np.errstate(all="ignore"):
        wn = float(np.arccos(trace / 2.0))     # NaN outside [-1, 1], as acos
    if wn > EPS:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))
    return w


def residuals(x, pts, ns):
    """r [2n] of mlpnp_residuals_and_jacs (:718-762)."""
    R = rodrigues2rot(x[:3])
    c = pts @ R.T + x[3:]
    u = c / np.linalg.norm(c, axis=1)[:, None]
    return np.einsum("nij,ni->nj", ns, u).reshape(-1)


def residuals_and_jac(x, pts, ns):
    """(r [2n], Jac [2n][6]): mlpnpJacs (:764-1393) as d(N^T normalize(R(w) p + t)) / d(w, t) through the chain rule,
    dR / dw from the Rodrigues form with its unguarded coefficients (w == 0 divides by zero, as the reference)."""
    x = np.asarray(x, np.float64)
    w = x[:3]
    R = rodrigues2rot(w)
    c = pts @ R.T + x[3:]
    nc = np.linalg.norm(c, axis=1)
    u = c / nc[:, None]
    r = np.einsum("nij,ni->nj", ns, u)
    with np.errstate(all="ignore"):
        n2 = float(w @ w)
        n = math.sqrt(n2)
        sn, cn = math.sin(n), math.cos(n)
        a, b = np.float64(sn) / n, np.float64(1.0 - cn) / n2
        da, db = np.float64(n * cn - sn) / (n2 * n), np.float64(n * sn - 2.0 * (1.0 - cn)) / (n2 * n2)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        # g = N^T (I - u u^T) / |c|   [n][2][3]
        g = (np.transpose(ns, (0, 2, 1)) - r[:, :, None] * u[:, None, :]) / nc[:, None, None]
        J = np.zeros((len(pts), 2, 6))
        for k in range(3):
            G = np.zeros((3, 3))
            e = np.zeros(3)
            e[k] = 1.0
            G[:, :] = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
            dR = (da * w[k]) * K + a * G + (db * w[k]) * (K @ K) + b * (G @ K + K @ G)
            J[:, :, k] = np.einsum("nij,nj->ni", g, pts @ dR.T)
        J[:, :, 3:] = g
    return r.reshape(-1), J.reshape(-1, 6)


def gauss_newton(x, pts, ns, dec=None):
    """mlpnp_gn (:650-716) -> (x, iterations, exit reason, worst cond(Jac^T Jac))."""
    x = np.array(x, np.float64)
    it, reason, cond = 0, GN_MAXIT, 1.0
    while it < 5:
        r, J = residuals_and_jac(x, pts, ns)
        A, g = J.T @ J, J.T @ r
        if not (np.isfinite(A).all() and np.isfinite(g).all()):
            x[:] = np.nan       # the reference goes on with NaN to a non-finite pose
            reason = GN_NAN
            break
        cond = max(cond, float(np.linalg.cond(A)))
        try:
            dx = np.linalg.solve(A, g)
        except np.linalg.LinAlgError:
            reason = GN_NAN
            break
        if not np.isfinite(dx).all():
            reason = GN_NAN
            break
        mx, mn = np.abs(dx).max(), np.abs(dx).min()
        if dec is not None:
            dec.cmp(mx, 5.0)
            dec.cmp(mn, 1.0)
        if mx > 5.0 or mn > 1.0:
            reason = GN_BREAK
            break
        dl = np.abs(J @ dx).max()
        if dec is not None:
            dec.cmp(dl, 1e-5)
        x = x - dx
        if dl < 1e-5:
            reason = GN_EPSP
            break
        it += 1
    return x, it, reason, cond


def _nearest_rotation(T):
    U, _, Vt = np.linalg.svd(T)
    return U @ Vt


def _direction_error(R, t, pts6, f6):
    v = pts6 @ R.T + t
    v = v / np.linalg.norm(v, axis=1)[:, None]
    e = 0.0
    for k in range(6):
        e += 1.0 - float(v[k] @ f6[k])
    return e


def fixed_sign(v):
    """An eigenvector with its largest component (the first on ties) positive: the solver's sign is free."""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def compute_pose(f, ns, pts):
    """computePose over n >= 6 correspondences (bearings f [n][3], nullspaces ns [n][3][2], points pts [n][3]) ->
    dict(planar, R0, t0, R, t, its, reason, kappa, near)."""
    dec = _Decisions()
    f, ns, pts = np.asarray(f, np.float64), np.asarray(ns, np.float64), np.asarray(pts, np.float64)
    n = len(pts)
    M = pts.T @ pts
    planar = fullpiv_rank3(M, dec) == 2
    E = np.eye(3)
    p3 = pts
    if planar:
        lam, vec = np.linalg.eigh(M)
        E = np.stack([fixed_sign(vec[:, i]) for i in range(3)])
        for i in range(3):
            a = np.sort(np.abs(vec[:, i]))
            dec.cmp(a[2], a[1])
        p3 = pts @ E.T
    A = np.zeros((2 * n, 9 if planar else 12))
    for s in range(2):
        v = ns[:, :, s]
        if planar:
            for a in range(3):
                A[s::2, 2 * a] = v[:, a] * p3[:, 1]
                A[s::2, 2 * a + 1] = v[:, a] * p3[:, 2]
            A[s::2, 6:] = v
        else:
            for a in range(3):
                A[s::2, 3 * a:3 * a + 3] = v[:, a:a + 1] * p3
            A[s::2, 9:] = v
    AtA = A.T @ A
    with np.errstate(all="ignore"):
        try:
            _, sv, Vt = np.linalg.svd(AtA)
        except np.linalg.LinAlgError:
            sv, Vt = np.full(AtA.shape[0], np.nan), np.full(AtA.shape, np.nan)
        x = Vt[-1]
        kappa = float(sv[0] / (sv[-2] - sv[-1])) if sv[-2] > sv[-1] else float("inf")
        if planar:
            c1, c2 = x[[0, 2, 4]], x[[1, 3, 5]]
            T = np.stack([np.cross(c1, c2), c1, c2])
            scale = 1.0 / math.sqrt(abs(np.linalg.norm(T[:, 1]) * np.linalg.norm(T[:, 2])))
            R1 = _nearest_rotation(T)
            if np.linalg.det(R1) < 0:
                R1 = -R1
            Q = -(E.T @ R1).T
            if np.linalg.det(Q) < 0:
                Q[:, 2] *= -1
            Q2 = Q * np.array([-1.0, -1.0, 1.0])
            t = scale * x[6:9]
            cand = [(Q, t), (Q, -t), (Q2, t), (Q2, -t)]
            errs = [_direction_error(R, tt, pts[:6], f[:6]) for R, tt in cand]
            best = int(np.argmin(errs))          # the first minimum, as std::min_element
            so = np.sort(errs)
            dec.cmp(so[0], so[1])
            R0, t0 = cand[best]
        else:
            T = np.array([[x[0], x[3], x[6]], [x[1], x[4], x[7]], [x[2], x[5], x[8]]])
            scale = 1.0 / abs(np.linalg.norm(T[:, 0]) * np.linalg.norm(T[:, 1]) * np.linalg.norm(T[:, 2])) ** (1.0 / 3.0)
            R1 = _nearest_rotation(T)
            if np.linalg.det(R1) < 0:
                R1 = -R1
            R0 = R1.T
            tp, tm = -(scale * x[9:12]), scale * x[9:12]
            e0, e1 = _direction_error(R0, tp, pts[:6], f[:6]), _direction_error(R0, tm, pts[:6], f[:6])
            dec.cmp(e0, e1)
            t0 = tp if e0 < e1 else tm
        x0 = np.concatenate([rot2rodrigues(R0), t0])
        xs, its, reason, cond = gauss_newton(x0, pts, ns, dec)
    kappa_final = kappa * cond
    if not kappa_final <= 1e8:
        dec.near = True
    dec.cmp(kappa_final, 1e8)
    return dict(planar=bool(planar), R0=np.array(R0), t0=np.array(t0), R=rodrigues2rot(xs[:3]), t=xs[3:].copy(),
                its=its, reason=reason, kappa=kappa, kappa_final=kappa_final, near=dec.near)


# ---- CheckInliers (:220-247) ---------------------------------------------------------------------------------------
def reprojection_errors(job, pre, R, t):
    """error2 [N] in float64 of the pose (R, t): the camera point narrowed to float32 as the reference does."""
    with np.errstate(all="ignore"):
        Xc = (pre["Xw"] @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)).astype(np.float32)
        uv = project(job["model"], job["cam"], Xc)
        d = pre["P2D"] - uv
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def check_inliers(job, pre, R, t):
    """(mask [N], count); a non-finite pose has none."""
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return np.zeros(len(pre["Xw"]), bool), 0
    with np.errstate(all="ignore"):
        m = reprojection_errors(job, pre, R, t) < pre["max_err"]
    return m, int(m.sum())


def pose32(R, t):
    """mBestTcw / mRefinedTcw: the double pose narrowed to float."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float64).astype(np.float32), np.asarray(t, np.float64).astype(np.float32)
    return T


# ---- iterate (:56-175) ---------------------------------------------------------------------------------------------
def new_state():
    return dict(iterations=0, best=0, valid=False, ok=False, rcount=0)


def replay_call(st, counts, refine, n_iterations, n_draws, n, min_inliers, max_its):
    """One iterate call on the carried state st from the per-hypothesis inlier counts: `refine(h)` is called for every
    hypothesis h of the call that becomes the best and returns (mnRefinedInliers, success); its outcome is kept.
    Returns dict(flags, kind, n_inliers, done, bests): kind 0 identity / 1 the refined outcome / 2 the best; done the
    hypotheses consumed; bests the hypotheses that became best."""
    out = dict(flags=0, kind=0, n_inliers=0, done=0, bests=[])
    if n < min_inliers:
        out["flags"] = NO_MORE
        return out
    cur = 0
    # while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations), within the draws supplied
    while (st["iterations"] < max_its or cur < n_iterations) and cur < n_draws:
        c = int(counts[cur])
        cur += 1
        st["iterations"] += 1
        out["done"] = cur
        if c >= min_inliers:
            if c > st["best"]:
                st["best"], st["valid"] = c, False
                out["bests"].append(cur - 1)
            if not st["valid"]:
                st["rcount"], st["ok"] = refine(cur - 1)
                st["valid"] = True
            if st["ok"]:
                out.update(flags=FOUND, kind=1, n_inliers=int(st["rcount"]))
                return out
    if st["iterations"] >= max_its:
        out["flags"] = NO_MORE
        if st["best"] >= min_inliers:
            out.update(flags=NO_MORE | FOUND, kind=2, n_inliers=int(st["best"]))
    return out


class RefSolver:
    """One job's MLPnPsolver: SetRansacParameters, hypothesis, Refine, iterate."""

    def __init__(self, job, bearing=None):
        self.job, self._bearing = job, bearing
        self.n = len(np.asarray(job["index"]))
        self.SetRansacParameters(*DEFAULTS)

    def SetRansacParameters(self, prob=0.99, min_inliers=8, max_its=300, min_set=6, epsilon=0.4, th2=5.991):
        assert min_set == 6
        self.pre = prepare(self.job, th2, self._bearing)
        self.max_its, self.min_inliers = ransac_parameters(self.n, prob, min_inliers, max_its, min_set, epsilon)
        self.state = new_state()
        self.best = self.refined = None
        self.n_refine_calls = 0
        return self

    def pose_of(self, idx):
        idx = np.asarray(idx, np.int64)
        return compute_pose(self.pre["f"][idx], self.pre["ns"][idx], self.pre["Xw"][idx])

    def hypothesis(self, draws):
        idx = sample_replay(self.n, draws)
        h = self.pose_of(idx)
        h["idx"] = idx
        h["mask"], h["count"] = check_inliers(self.job, self.pre, h["R"], h["t"])
        return h

    def refine(self, best_mask):
        """Refine (:249-303) as a function of mvbBestInliers: computePose over its correspondences, CheckInliers of the
        result, success if the count is strictly greater than mRansacMinInliers."""
        self.n_refine_calls += 1
        r = self.pose_of(np.nonzero(best_mask)[0])
        r["mask"], r["count"] = check_inliers(self.job, self.pre, r["R"], r["t"])
        r["ok"] = r["count"] > self.min_inliers
        return r

    def iterate(self, n_iterations, draws):
        """iterate(nIterations, ...) on raw draws [n_draws][6] -> dict(flags, n_inliers, T [4][4] float32, vb [mN]),
        Refine evaluated once per distinct best (iterate_literal calls it at every qualifying hypothesis)."""
        hyps = {}

        def hyp(h):
            if h not in hyps:
                hyps[h] = self.hypothesis(draws[h])
            return hyps[h]

        class _Counts:
            def __getitem__(_, h):
                return hyp(h)["count"]

        def refine(h):
            self.best = hyp(h)
            self.refined = self.refine(self.best["mask"])
            return self.refined["count"], self.refined["ok"]

        out = replay_call(self.state, _Counts(), refine, n_iterations, len(draws), self.n, self.min_inliers,
                          self.max_its)
        T, vb = np.eye(4, dtype=np.float32), np.zeros(int(self.job["mN"]), bool)
        src = self.refined if out["kind"] == 1 else (self.best if out["kind"] == 2 else None)
        if src is not None:
            T = pose32(src["R"], src["t"])
            vb[np.asarray(self.job["index"])[src["mask"]]] = True
        out.update(T=T, vb=vb, hyps=hyps)
        return out

    def iterate_literal(self, n_iterations, draws):
        """The reference's text, Refine at every hypothesis that passes :129 (no kept outcome), on a state of its own:
        (flags, n_inliers, T, vb, state)."""
        if not hasattr(self, "lit"):
            self.lit = dict(iterations=0, best=0, best_h=None)
        st = self.lit
        T, vb = np.eye(4, dtype=np.float32), np.zeros(int(self.job["mN"]), bool)
        if self.n < self.min_inliers:
            return NO_MORE, 0, T, vb
        cur = 0
        index = np.asarray(self.job["index"])
        while (st["iterations"] < self.max_its or cur < n_iterations) and cur < len(draws):
            h = self.hypothesis(draws[cur])
            cur += 1
            st["iterations"] += 1
            if h["count"] >= self.min_inliers:
                if h["count"] > st["best"]:
                    st["best"], st["best_h"] = h["count"], h
                r = self.refine(st["best_h"]["mask"])
                if r["ok"]:
                    vb[index[r["mask"]]] = True
                    return FOUND, r["count"], pose32(r["R"], r["t"]), vb
        if st["iterations"] >= self.max_its:
            if st["best"] >= self.min_inliers:
                b = st["best_h"]
                vb[index[b["mask"]]] = True
                return NO_MORE | FOUND, b["count"], pose32(b["R"], b["t"]), vb
            return NO_MORE, 0, T, vb
        return 0, 0, T, vb
