"""A float64 numpy reference of Optimizer::FullInertialBA's optimisation (src/Optimizer.cc:368-853), the checker of the
device solver's full inertial kind (omv_fiba, openmavis_amd/csrc/lba.hip).

The graph is the reference's: VertexPose per keyframe, VertexVelocity per bImu keyframe, VertexGyroBias / VertexAccBias
per bImu keyframe (shared_bias 0) or ONE pair for the map (shared_bias 1, the bInit form), marginalised points; EdgeMono /
EdgeStereo (Huber sqrt(5.991) / sqrt(7.815), float thresholds), EdgeInertial (Huber sqrt(16.92), the full information),
EdgeGyroRW / EdgeAccRW beside every EdgeInertial (shared_bias 0) or EdgePriorGyro / EdgePriorAcc on the pair (shared_bias
1: error 0 - b, Jacobian -I, information prior * I3, no kernel; G2oTypes.h:704-747).  A point seen by fixed keyframes only
is no vertex (:771-774).  The system is built dense, the points are eliminated by a dense Schur complement, the step
control is tests/lm_ref.py's.

The edges' residuals and Jacobians are the project's existing statement of them, the CPU oracle (oracle.lba_evaluate:
EdgeMono / EdgeStereo 2|3 x 3 and x 6, EdgeInertial 9 x 24 over [P1 V1 G1 A1 P2 V2]).  What is restated here is the graph:
which vertex a Jacobian column belongs to (with the shared pair, columns G1 A1 of every edge are the pair's), the
information matrices, the robust weights, the priors, the update (ImuCamPose::Update with its every-third
NormalizeRotation) and the Levenberg loop.  tests/test_fiba_ref_cpu.py anchors it to the oracle's own LM on the ground
they share (shared_bias 0) and checks the shared pair's columns against central differences.
"""
import numpy as np

import inertial_ref
import lm_ref

HUBER_MONO = float(np.float32(np.sqrt(5.991)))
HUBER_STEREO = float(np.float32(np.sqrt(7.815)))
HUBER_IMU = float(np.sqrt(16.92))
STATE = ("Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba", "pts")


def huber(e2, delta):
    e2 = np.asarray(e2, np.float64)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        s = np.sqrt(e2)
        out = e2 > dsqr
        return np.where(out, 2 * s * delta - dsqr, e2), np.where(out, delta / s, 1.0)


class Graph:
    """The vertices and edges of a problem dict (openmavis_amd.synth_fiba.make_fiba_problem's fields).  Variables:
    per optimisable keyframe k a block of `kw` = 15 (pose 6 (rotation, translation) | v 3 | bg 3 | ba 3) at kw * k -- the
    v / bias rows of a keyframe that is not bImu, and with the shared pair every keyframe's bias rows, are absent
    (`present` false) --, then with the shared pair its 6 (bg | ba), then 3 per point vertex."""

    def __init__(self, prob):
        p = prob
        self.prob = p
        self.K, self.n_opt, self.C = int(p["n_kf"]), int(p["n_opt"]), int(p["n_cams"])
        self.kf_imu = np.asarray(p["kf_imu"], bool)
        self.shared = bool(p.get("shared_bias", 0))
        self.prior_g, self.prior_a = float(p.get("prior_g", 0.0)), float(p.get("prior_a", 0.0))
        self.P = len(p["pts"])
        self.m_pt, self.m_kf = np.asarray(p["mono_pt"], np.int64), np.asarray(p["mono_kf"], np.int64)
        self.m_w = np.asarray(p["mono_inv_sigma2"], np.float64)
        ns = int(p.get("n_stereo", 0))
        self.s_pt = np.asarray(p["stereo_pt"], np.int64) if ns else np.zeros(0, np.int64)
        self.s_kf = np.asarray(p["stereo_kf"], np.int64) if ns else np.zeros(0, np.int64)
        self.s_w = np.asarray(p["stereo_inv_sigma2"], np.float64) if ns else np.zeros(0)
        # bAllFixed (:583, :771-774): a point is a vertex when an optimisable keyframe observes it
        self.pt_vertex = np.zeros(self.P, bool)
        self.pt_vertex[self.m_pt[self.m_kf < self.n_opt]] = True
        self.pt_vertex[self.s_pt[self.s_kf < self.n_opt]] = True
        self.m_in, self.s_in = self.pt_vertex[self.m_pt], self.pt_vertex[self.s_pt]
        self.k1, self.k2 = np.asarray(p["imu_kf1"], np.int64), np.asarray(p["imu_kf2"], np.int64)
        self.NI = len(self.k1)
        assert self.kf_imu[self.k1].all() and self.kf_imu[self.k2].all(), "an EdgeInertial joins two bImu keyframes (:469)"
        pre = np.asarray(p["preint"], np.float32).reshape(-1, 292)
        self.info9 = inertial_ref.information(pre) if self.NI else np.zeros((0, 9, 9))
        Cc = pre[:, 67:67 + 225].reshape(-1, 15, 15).astype(np.float64)
        self.infoG = np.array([np.linalg.inv(c[9:12, 9:12]) for c in Cc]).reshape(-1, 3, 3)   # :524-534
        self.infoA = np.array([np.linalg.inv(c[12:15, 12:15]) for c in Cc]).reshape(-1, 3, 3)
        self.kw = 15
        self.n_kf_vars = self.kw * self.n_opt
        self.off_shared = self.n_kf_vars if self.shared else -1
        self.n_pose = self.n_kf_vars + (6 if self.shared else 0)
        self.pt_index = np.full(self.P, -1, np.int64)
        self.pt_index[self.pt_vertex] = np.arange(int(self.pt_vertex.sum()))
        self.n_ptv = int(self.pt_vertex.sum())
        self.n_var = self.n_pose + 3 * self.n_ptv
        present = np.zeros(self.n_pose, bool)
        for k in range(self.n_opt):
            present[15 * k:15 * k + 6] = True
            if self.kf_imu[k]:
                present[15 * k + 6:15 * k + 9] = True
                if not self.shared:
                    present[15 * k + 9:15 * k + 15] = True
        if self.shared:
            present[self.off_shared:] = True
        self.present = present

    # columns of an EdgeInertial's 24 Jacobian columns [P1 6 | V1 3 | G1 3 | A1 3 | P2 6 | V2 3] in the variable vector
    # (-1: a fixed vertex)
    def imu_columns(self, i):
        a, b = int(self.k1[i]), int(self.k2[i])
        col = np.full(24, -1, np.int64)
        if a < self.n_opt:
            col[0:9] = 15 * a + np.arange(9)
        if self.shared:
            col[9:15] = self.off_shared + np.arange(6)   # vertices 2 and 3 are the pair (:485-486)
        elif a < self.n_opt:
            col[9:15] = 15 * a + 9 + np.arange(6)
        if b < self.n_opt:
            col[15:24] = 15 * b + np.arange(9)
        return col


def start_of(prob):
    st = {k: np.array(prob[k], np.float64, copy=True) for k in STATE}
    st["Rwb"], st["Rcw"] = st["Rwb"].reshape(-1, 3, 3), st["Rcw"].reshape(len(st["Rwb"].reshape(-1, 3, 3)), -1, 3, 3)
    st["tcw"] = st["tcw"].reshape(st["Rcw"].shape[0], -1, 3)
    return st


def cam_poses(G, Rwb, twb):
    Rcb, tcb = np.asarray(G.prob["Rcb"], np.float64).reshape(-1, 3, 3), np.asarray(G.prob["tcb"], np.float64).reshape(-1, 3)
    Rbw = Rwb.T
    tbw = -Rbw @ twb
    return np.einsum("cij,jk->cik", Rcb, Rbw), np.einsum("cij,j->ci", Rcb, tbw) + tcb


def evaluate(G, st, oracle):
    """The edges at state `st` through the oracle's statement of them."""
    o = oracle.lba_evaluate(dict(G.prob, **{k: st[k] for k in STATE}))
    ns = len(G.s_pt)
    return dict(mono_err=o["mono_err"], mono_jx=o["mono_jx"].reshape(-1, 2, 3), mono_jp=o["mono_jp"].reshape(-1, 2, 6),
                stereo_err=o["stereo_err"].reshape(ns, 3), stereo_jx=o["stereo_jx"].reshape(ns, 3, 3),
                stereo_jp=o["stereo_jp"].reshape(ns, 3, 6), imu_err=o["imu_err"], imu_jac=o["imu_jac"])


def shared_value(G, st):
    """The shared pair's value: every bImu keyframe holds it; read where the device reads it (the first one)."""
    k = int(np.argmax(G.kf_imu))
    return st["bg"][k], st["ba"][k]


def chi2_of(G, st, ev):
    """Per-edge chi2 and the robust weights: dict of (chi2, rho, rho') per edge kind, and activeRobustChi2."""
    out = {}
    c = G.m_w * (ev["mono_err"] ** 2).sum(1)
    out["mono"] = (c,) + huber(c, HUBER_MONO)
    c = G.s_w * (ev["stereo_err"] ** 2).sum(1)
    out["stereo"] = (c,) + huber(c, HUBER_STEREO)
    c = np.einsum("ei,eij,ej->e", ev["imu_err"], G.info9, ev["imu_err"]) if G.NI else np.zeros(0)
    out["imu"] = (c,) + huber(c, HUBER_IMU)   # every EdgeInertial has the kernel (:514-516)
    total = out["mono"][1][G.m_in].sum() + out["stereo"][1][G.s_in].sum() + out["imu"][1].sum()
    if G.shared:
        bg, ba = shared_value(G, st)
        out["prior"] = np.array([G.prior_g * (bg @ bg), G.prior_a * (ba @ ba)])   # e = 0 - b
        total += out["prior"].sum()
    elif G.NI:
        eg, ea = st["bg"][G.k2] - st["bg"][G.k1], st["ba"][G.k2] - st["ba"][G.k1]
        out["rw"] = np.einsum("ei,eij,ej->e", eg, G.infoG, eg) + np.einsum("ei,eij,ej->e", ea, G.infoA, ea)
        total += out["rw"].sum()
    out["total"] = float(total)
    return out


def build_system(G, st, ev, ch):
    """buildSystem, dense: H [n_var][n_var] and b = -J^T Omega rho' e over [keyframe blocks | shared pair | point vertices]."""
    n = G.n_var
    H, b = np.zeros((n, n)), np.zeros(n)

    def add(cols, J, W, e, r1):
        m = cols >= 0
        Jm = J[:, m]
        WJ = (W @ Jm) * r1
        ix = cols[m]
        H[np.ix_(ix, ix)] += Jm.T @ WJ
        b[ix] += -(Jm.T @ (W @ e)) * r1

    for (pt, kf, w, err, jx, jp, inn, r1, nr) in (
            (G.m_pt, G.m_kf, G.m_w, ev["mono_err"], ev["mono_jx"], ev["mono_jp"], G.m_in, ch["mono"][2], 2),
            (G.s_pt, G.s_kf, G.s_w, ev["stereo_err"], ev["stereo_jx"], ev["stereo_jp"], G.s_in, ch["stereo"][2], 3)):
        for e in np.flatnonzero(inn):
            cols = np.full(9, -1, np.int64)
            cols[0:3] = G.n_pose + 3 * G.pt_index[pt[e]] + np.arange(3)
            if kf[e] < G.n_opt:
                cols[3:9] = 15 * kf[e] + np.arange(6)
            add(cols, np.concatenate([jx[e], jp[e]], axis=1), w[e] * np.eye(nr), err[e], r1[e])
    for i in range(G.NI):
        add(G.imu_columns(i), ev["imu_jac"][i], G.info9[i], ev["imu_err"][i], ch["imu"][2][i])
        if not G.shared:   # EdgeGyroRW / EdgeAccRW: e = b2 - b1, J1 = -I, J2 = I
            a, c = int(G.k1[i]), int(G.k2[i])
            for off, info, vec in ((9, G.infoG[i], st["bg"]), (12, G.infoA[i], st["ba"])):
                cols = np.concatenate([15 * a + off + np.arange(3) if a < G.n_opt else np.full(3, -1),
                                       15 * c + off + np.arange(3) if c < G.n_opt else np.full(3, -1)]).astype(np.int64)
                add(cols, np.concatenate([-np.eye(3), np.eye(3)], axis=1), info, vec[c] - vec[a], 1.0)
    if G.shared:   # EdgePriorGyro / EdgePriorAcc
        bg, ba = shared_value(G, st)
        add(G.off_shared + np.arange(3), -np.eye(3), G.prior_g * np.eye(3), 0.0 - bg, 1.0)
        add(G.off_shared + 3 + np.arange(3), -np.eye(3), G.prior_a * np.eye(3), 0.0 - ba, 1.0)
    return H, b


def reduce_system(G, H, b, lam):
    """The landmark Schur complement at damping lam over the present pose-side variables: (S, rhs, index of its rows in
    the variable vector, what the back-substitution needs)."""
    ip = np.flatnonzero(G.present)
    npz = G.n_pose
    Hpp, Hpl, Hll = H[np.ix_(ip, ip)], H[ip, npz:], H[npz:, npz:]
    D = Hll.reshape(G.n_ptv, 3, G.n_ptv, 3)[np.arange(G.n_ptv), :, np.arange(G.n_ptv), :] + lam * np.eye(3)
    Dinv = np.linalg.inv(D) if G.n_ptv else np.zeros((0, 3, 3))
    Y = np.einsum("apj,pjl->apl", Hpl.reshape(len(ip), G.n_ptv, 3), Dinv).reshape(len(ip), -1)   # Hpl Dinv
    S = Hpp + lam * np.eye(len(ip)) - Y @ Hpl.T
    rhs = b[ip] - Y @ b[npz:]
    return S, rhs, ip, (Dinv, Hpl)


def device_layout(G, S, rhs, ip, lam):
    """The reduced system as omv_fiba_debug_solve lays it out: 16 rows per block (keyframe k: pose 0-5, v 6-8, bg 9-11,
    ba 12-14, pad 15; the shared pair: block n_opt, rows 9-14), an absent row has lam on its diagonal and a zero
    right-hand side."""
    nb = G.n_opt + (1 if G.shared else 0)
    at = np.empty(len(ip), np.int64)
    for q, v in enumerate(ip):
        at[q] = 16 * (v // 15) + v % 15 if v < G.n_kf_vars else 16 * G.n_opt + 9 + (v - G.off_shared)
    S16, r16 = lam * np.eye(16 * nb), np.zeros(16 * nb)
    S16[np.ix_(at, at)] = S
    r16[at] = rhs
    return S16, r16, at


def solve(G, H, b, lam, order=None):
    """One damped solve: (ok, x [n_var]).  order: a permutation of the reduced system's rows to eliminate in (the
    solution does not depend on it beyond rounding)."""
    S, rhs, ip, (Dinv, Hpl) = reduce_system(G, H, b, lam)
    try:
        if order is None:
            xp = np.linalg.solve(S, rhs)
        else:
            xp = np.empty(len(ip))
            xp[order] = np.linalg.solve(S[np.ix_(order, order)], rhs[order])
    except np.linalg.LinAlgError:
        return False, None
    xl = np.einsum("pij,pj->pi", Dinv, b[G.n_pose:].reshape(-1, 3) - (Hpl.T @ xp).reshape(-1, 3))
    x = np.zeros(G.n_var)
    x[ip], x[G.n_pose:] = xp, xl.reshape(-1)
    return bool(np.isfinite(x).all()), x


def update(G, st, x, normalize):
    """oplus of every vertex: ImuCamPose::Update (G2oTypes.cc:211-235: twb += Rwb ut, Rwb = Rwb Exp(ur), NormalizeRotation
    after every third update), v, the biases, the points."""
    s = {k: v.copy() for k, v in st.items()}
    for k in range(G.n_opt):
        u = x[15 * k:15 * k + 15]
        s["twb"][k] = st["twb"][k] + st["Rwb"][k] @ u[3:6]
        R = st["Rwb"][k] @ inertial_ref.exp_so3(u[0:3])
        if normalize:
            uu, _, vt = np.linalg.svd(R)
            R = uu @ vt
        s["Rwb"][k] = R
        s["Rcw"][k], s["tcw"][k] = cam_poses(G, R, s["twb"][k])
        if G.kf_imu[k]:
            s["vel"][k] = st["vel"][k] + u[6:9]
            if not G.shared:
                s["bg"][k], s["ba"][k] = st["bg"][k] + u[9:12], st["ba"][k] + u[12:15]
    if G.shared:   # every bImu keyframe holds the pair (:818-829)
        d = x[G.off_shared:G.off_shared + 6]
        s["bg"][G.kf_imu] = st["bg"][G.kf_imu] + d[0:3]
        s["ba"][G.kf_imu] = st["ba"][G.kf_imu] + d[3:6]
    s["pts"][G.pt_vertex] = st["pts"][G.pt_vertex] + x[G.n_pose:].reshape(-1, 3)
    return s


def optimize(G, st, oracle, iterations=100, lambda_init=1e-5, max_trials=10, order=None):
    """optimizer.optimize(iterations) from `st`.  Returns (result, final state): err, err_end, iterations, trials, lambda_,
    mono_chi2 / stereo_chi2 of the last computed errors, and for the tests' own conditions `rhos`, `dchi` (every trial's
    rho and its numerator, the chi2 the trial gained) and `stops` (both sides of the stop rule per finished iteration)."""
    ev = evaluate(G, st, oracle)
    ch = chi2_of(G, st, ev)
    res = dict(err=ch["total"], iterations=0, trials=0, rhos=[], stops=[], dchi=[])
    lm = lm_ref.LmState()
    cur_ev, cur_ch, last_ch = ev, ch, ch
    n_acc = 0
    nxt = lm_ref.ITERATION
    for it in range(iterations):
        res["iterations"] += 1
        H, b = build_system(G, st, cur_ev, cur_ch)
        lm_ref.begin_iteration(lm, it, cur_ch["total"], lambda_init)
        while True:
            ok, x = solve(G, H, b, lm.lam, order)
            scale, temp_chi = 0.0, 0.0
            if ok:
                trial = update(G, st, x, n_acc % 3 == 2)
                tev = evaluate(G, trial, oracle)
                tch = chi2_of(G, trial, tev)
                temp_chi, last_ch = tch["total"], tch
                scale = float((x * (lm.lam * x + b)).sum())
            before = lm.current_chi
            rho, accepted = lm_ref.trial(lm, temp_chi, ok, scale)
            res["trials"] += 1
            res["rhos"].append(rho)
            res["dchi"].append(before - temp_chi if ok else float("nan"))
            if accepted:
                st, cur_ev, cur_ch = trial, tev, tch
                n_acc += 1
            stop_sides = lm_ref.gain_sides(lm)
            nxt = lm_ref.next_step(lm, rho, max_trials)
            if nxt != lm_ref.TRIAL:
                break
        if nxt == lm_ref.ITERATION or lm.n_bad >= 3:
            res["stops"].append(stop_sides)
        if nxt == lm_ref.STOP:
            break
    res.update(err_end=last_ch["total"], lambda_=lm.lam, mono_chi2=np.where(G.m_in, last_ch["mono"][0], 0.0),
               stereo_chi2=np.where(G.s_in, last_ch["stereo"][0], 0.0))
    return res, st


# ---- gauge-invariant view of a state (no fixed keyframe: translation and yaw about gravity are free) -----------------------
def gauge_invariant(st):
    """Keyframe poses relative to keyframe 0, Rwb^T v, the biases, and the points in keyframe 0's body frame."""
    R0, t0 = st["Rwb"][0], st["twb"][0]
    return dict(Rrel=np.einsum("ji,kjl->kil", R0, st["Rwb"]), trel=(st["twb"] - t0) @ R0,
                vb=np.einsum("kji,kj->ki", st["Rwb"], st["vel"]), bg=st["bg"].copy(), ba=st["ba"].copy(),
                pts=(st["pts"] - t0) @ R0)
