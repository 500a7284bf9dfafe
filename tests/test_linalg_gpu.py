"""The device linear-algebra routines against exact and high-precision references (oracle/linalg_ref.py, validated
without a GPU by tests/test_linalg_ref_cpu.py), through the library's test hooks (omv_selftest_*, omv_lba_debug_solve):

  ldlt_pick_solve<6 | 9 | 24>, ldlt_pivot_solve_wave<15 | 30>   generic SPD systems against the 50-digit solution, and
      exact systems (every intermediate representable) bit for bit against the Fraction replay of Eigen's LDLT: x, the
      pivot order and the verdict, with diagonal ties, zero pivots, a zero diagonal, negative D, and a NaN at the
      first, second, third, fifth, middle and last diagonal position (false, x untouched)
  pinv15_wave                 the LDL^T shortcut and the Jacobi fallback against the 50-digit truncated pseudo-inverse
  inertial_info9_wave<f / t>  real preintegration covariances, and ones with a negative / a huge eigen-direction whose
                              inverse eigenvalue is zeroed, against the 50-digit inverse -> symmetrise -> clamp
  inv16                       padded 15 + 1 and 6 + 10 blocks (real ones from the reduced system, and a condition sweep)
  the reduced system          S, rhs and x of one LM trial on windows that reach each plan of the block solver (every
                              block in LDS at 3 and at its limit of 12 dense keyframes, the hybrid LDS / global storage
                              at 13, two clusters that factor side by side), x against the refined solution of the
                              returned system, and S, rhs themselves against the Schur complement formed from the
                              handle's own Jacobians (visual-only windows, EdgeMono and EdgeStereo)
Every case asserts the path it is named for.  The all-global storage of the block solver (ldlt_kernel<1>) is reachable
only through a special build (-DOMV_LBA_FORCE_G) and is left out.

Bars (no hand-picked epsilons).  Solves, inverses, pseudo-inverses: e = |got - exact|_inf / |exact|_inf <=
max(4 e_ref, 3 n u kappa_2), u = 2^-53, e_ref the error of the plain float64 LAPACK result (numpy solve / inv / eigh)
against the same exact answer.  kappa_2 comes from the 50-digit spectrum for pinv15_wave (over the kept eigenvalues),
inertial_info9_wave and inv16; for the LDL^T solves (every N) and the reduced system it comes from the Rayleigh
quotients of float64 eigenvectors evaluated exactly -- a lower bound of kappa_2, so the bar is never wider than stated.  The reduced system's padding rows decouple exactly (asserted), so its solve is judged on the
coupled unknowns alone (again the narrower bar: lambda = 1e-9 on the padding would put 1e15 into kappa_2), and
inv16's padding pivots are judged as the 1 x 1 systems they are.  Schur entries: error over the entrywise absolute
accumulation sum |J^T W J| + sum |Hpl| |(Hll + lambda I)^-1| |Hlp|, <= 8 x the same figure of a float64 numpy
evaluation of the formula; the reference is the same formula in 80-bit long double (u = 5e-20, three digits below what
is measured, not the 40 digits of the other references: an exact or mpmath evaluation of the whole window takes tens of
seconds per case), so this check needs a platform whose long double is the x87 one and fails its own assertion
elsewhere.  Exact cases: bit equality.

Measured on an MI355X (worst case over the cases of each routine; each test prints its figures, pytest -s):
                                        e / (n u kappa_2)   e / e_ref
  ldlt_pick_solve<6>                    0.020               5.7
  ldlt_pick_solve<9>                    0.0055              1.4
  ldlt_pick_solve<24>                   0.0036              1.9
  ldlt_pivot_solve_wave<15>             0.0074              1.9
  ldlt_pivot_solve_wave<30>             0.0041              3.1
  pinv15_wave, LDL^T path               0.034               0.67
  pinv15_wave, Jacobi path              0.55                5.5
  inertial_info9_wave<false>            0.027               3.5
  inertial_info9_wave<true>, shortcut   0.00022             0.81
  inertial_info9_wave<true>, Jacobi     0.027               4.7
  inv16                                 0.024               4.1
  reduced-system solve (24 cases)       0.0013              1.7
  (where e / e_ref exceeds 4 the case passes on the second term, well inside 3 n u kappa_2)
  Schur complement, normalised error over numpy's: S 0.49 .. 1.41, rhs 0.20 .. 2.26 (bar 8)
"""
from fractions import Fraction

import numpy as np
import pytest

import linalg_ref as ref
from openmavis_amd import selftest, synth_ba, synth_imu, synth_pose
from openmavis_amd.optimizer import LocalInertialBA
from openmavis_amd.synth_ba_const import IMU_NOISE

pytestmark = pytest.mark.gpu

LDLT = [(selftest.PICK, 6), (selftest.PICK, 9), (selftest.PICK, 24), (selftest.PIVOT, 15), (selftest.PIVOT, 30)]
LDLT_IDS = ["pick6", "pick9", "pick24", "pivot15", "pivot30"]
SENTINEL = -7.5
LAMBDAS = (1e-9, 1e-2, 1e2)


def _report(label, e, e_ref, n, kappa):
    print(f"[linalg] {label}: e {e:.3e}  e/(n u kappa) {e / (n * ref.U * kappa):.3g}  e/e_ref {e / max(e_ref, 1e-300):.3g}"
          f"  (n {n}, kappa {kappa:.3g}, e_ref {e_ref:.3e})")


def _spd(n, kappa, rng):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    H = (Q * np.logspace(0, -np.log10(kappa), n)) @ Q.T
    return (H + H.T) / 2


# ---- pivoted LDL^T ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pose_hessians(oracle):
    """Marginalised 15 x 15 Hessians of PoseInertialOptimizationLastFrame (entries ~1e3 .. 1e7), symmetrised."""
    b = synth_pose.make_last_frame_batch(n_frames=4, n_pts=200, seed=6)
    H = oracle.pose_last_frame(b)[3].reshape(-1, 15, 15)
    return (H + np.transpose(H, (0, 2, 1))) / 2


def _pose_like(H15, n, rng):
    """An n x n system with a real pose Hessian's scaling: the leading block of B^T diag(H1, H2) B, B unit lower."""
    T = rng.normal(size=(15, 15))
    K = np.block([[H15[0] + T.T @ H15[1] @ T, T.T @ H15[1]], [H15[1] @ T, H15[1]]])
    K = (K + K.T) / 2
    return H15[2][:n, :n] if n <= 15 else K[:n, :n]


def _check_order(routine, order, diag):
    pick, tr = ref.pivot_order(diag)
    if routine == selftest.PICK:
        assert list(order) == pick, (list(order), pick)
    else:
        assert list(order) == tr and ref.order_from_transpositions(list(order)) == pick, (list(order), tr)


@pytest.mark.parametrize("routine,n", LDLT, ids=LDLT_IDS)
def test_ldlt_generic_spd(torch_cuda, pose_hessians, routine, n):
    rng = np.random.default_rng(40 + n)
    Hs = [_spd(n, kappa, rng) for kappa in (1e2, 1e6, 1e10) for _ in range(2)]
    names = [f"kappa {k:g}" for k in (1e2, 1e6, 1e10) for _ in range(2)] + ["pose", "pose"]
    Hs += [_pose_like(pose_hessians, n, rng), _pose_like(pose_hessians[::-1], n, rng)]
    bs = [rng.normal(size=n) * np.abs(H).max() for H in Hs]
    x, order, ok = selftest.ldlt(routine, np.stack(Hs), np.stack(bs), SENTINEL)
    worst = (0.0, 0.0)
    for i, (H, b) in enumerate(zip(Hs, bs)):
        assert ok[i] == 1, names[i]
        diag = np.diag(H).tolist()
        assert len(set(np.abs(diag))) == n   # distinct diagonals: the rank-order path of ldlt_pick_solve
        _check_order(routine, order[i], diag)
        _, exact = ref.mp_solve(H, b)
        kappa = ref.rayleigh_cond_lower_bound(H)
        e, e_ref = ref.forward_error(x[i], exact), ref.forward_error(np.linalg.solve(H, b), exact)
        _report(f"ldlt {LDLT_IDS[LDLT.index((routine, n))]} {names[i]}", e, e_ref, n, kappa)
        assert e <= ref.solve_bound(n, kappa, e_ref), (names[i], e, e_ref, kappa)
        worst = max(worst, (e / (n * ref.U * kappa), e / e_ref))
    print(f"[linalg] ldlt {LDLT_IDS[LDLT.index((routine, n))]} worst e/(n u kappa), its e/e_ref: {worst}")


@pytest.mark.parametrize("routine,n", LDLT, ids=LDLT_IDS)
def test_ldlt_exact_cases_bit_for_bit(torch_cuda, routine, n):
    cases = ref.exact_suite(n, seed=7)
    names = list(cases)
    x, order, ok = selftest.ldlt(routine, np.array([cases[k][0] for k in names]), np.array([cases[k][1] for k in names]),
                                 SENTINEL)
    for i, name in enumerate(names):
        H, b = cases[name]
        r = ref.ldlt_replay(H, b)
        assert bool(ok[i]) == r["ok"], (name, ok[i])
        if r["ok"]:
            assert np.array_equal(ref.bits(x[i]), ref.bits([float(v) for v in r["x"]])), (name, x[i], r["x"])
        else:   # isPositive() false: x is left as it was
            assert np.array_equal(ref.bits(x[i]), ref.bits(np.full(n, SENTINEL))), (name, x[i])
        if r["pick"] is not None:
            want = r["pick"] if routine == selftest.PICK else r["tr"]
            assert list(order[i]) == want, (name, list(order[i]), want)
        # the path the case is named for: ties go through ldlt_pick_solve's step-by-step replay, distinct
        # magnitudes through its rank order
        diag = [abs(H[q][q]) for q in range(n)]
        assert (len(set(diag)) < n) == (name not in ("distinct", "negative_d") and not name.startswith("nan_")), name
    nans = {f"nan_diagonal_{q}" for q in ref.nan_positions(n)}
    assert len(nans) >= 6 and {k for k in names if not ref.ldlt_replay(*cases[k])["ok"]} == {
        "negative_d", "indefinite_equal_abs"} | nans


# ---- pinv15_wave ------------------------------------------------------------------------------------------------
def _sym_from_spectrum(w, rng):
    Q, _ = np.linalg.qr(rng.normal(size=(len(w), len(w))))
    A = (Q * np.asarray(w)) @ Q.T
    return (A + A.T) / 2


def test_pinv15_both_paths(torch_cuda):
    rng = np.random.default_rng(15)
    fast = [np.logspace(-3, 3, 15), np.logspace(-3, 0, 15), np.logspace(0, 1, 15), np.full(15, 2.0) + np.arange(15)]
    slow = [np.concatenate([np.logspace(-4, 2, 12), d]) for d in ([0, 0, 0], [1e-9, -1e-9, 0], [1e-9, 1e-9, 1e-9])]
    slow += [np.concatenate([np.logspace(-4, 0, 14), [0.0]]), np.concatenate([np.logspace(-2, 2, 14), [-1e-9]])]
    # a kept negative eigenvalue (1 / w stays negative), with and without dropped directions
    slow += [np.concatenate([np.logspace(-3, 1, 13), [-0.5, 1e-9]]), np.concatenate([np.logspace(-3, 1, 14), [-1e-4]])]
    # rank 1 and a tiny-frame block: one strong direction only
    slow += [np.concatenate([[5.0], np.zeros(14)]), np.concatenate([[3.0, 1e-4], [1e-9] * 13])]
    A = [_sym_from_spectrum(w, rng) for w in fast + slow]
    P, path = selftest.pinv15(np.stack(A))
    worst = {0: (0.0, 0.0), 1: (0.0, 0.0)}
    for i, Ai in enumerate(A):
        want = 1 if i < len(fast) else 0
        assert path[i] == want, (i, path[i])
        _, exact, kept, allw = ref.mp_pinv_trunc(Ai)
        dropped = [v for v in allw if abs(v) <= 1e-6]
        # both sides of the 1e-6 cut are cleared by 100 x: the exact answer is not discontinuous under rounding
        assert min(abs(v) for v in kept) >= 0.99e-4 and all(abs(v) <= 1e-8 for v in dropped)
        assert len(dropped) == int(np.sum(np.abs((fast + slow)[i]) <= 1e-6))
        if i >= len(fast) + 5 and i < len(fast) + 7:
            assert min(kept) < 0 and np.linalg.eigvalsh(P[i]).min() < 0
        kappa = float(max(abs(v) for v in kept) / min(abs(v) for v in kept))
        w, V = np.linalg.eigh(Ai)
        keep = np.abs(w) > 1e-6
        P_ref = (V[:, keep] / w[keep]) @ V[:, keep].T
        ex = [exact[r, c] for r in range(15) for c in range(15)]
        e, e_ref = ref.forward_error(P[i], ex), ref.forward_error(P_ref, ex)
        _report(f"pinv15 case {i} path {want}", e, e_ref, 15, kappa)
        assert e <= ref.solve_bound(15, kappa, e_ref), (i, e, e_ref, kappa)
        worst[want] = max(worst[want], (e / (15 * ref.U * kappa), e / e_ref))
    print(f"[linalg] pinv15 worst e/(n u kappa), its e/e_ref: LDL^T path {worst[1]}, Jacobi path {worst[0]}")


# ---- inertial_info9_wave ----------------------------------------------------------------------------------------
def _covariances():
    """Real float covariances: the preintegrations of an LBA window (0.1 s at 400 Hz), longer and shorter intervals, and
    noisy 200 Hz streams with a bias (synth_imu); entries from ~1e-20 to ~1e-3."""
    prob = synth_ba.make_lba_problem(n_kf=6, n_opt=3, n_pts=20, seed=2, n_cams=2)
    C = [c.reshape(15, 15) for c in prob["preint"][:, -225:]]
    C += [synth_ba.preintegrate(t0, t1)[-225:].reshape(15, 15) for t0, t1 in ((0.0, 0.05), (1.0, 1.5), (2.0, 3.0))]
    ng, na, ngw, naw = IMU_NOISE
    Nga = [(ng * np.sqrt(200.0)) ** 2] * 3 + [(na * np.sqrt(200.0)) ** 2] * 3
    imu = synth_imu.make_imu_batch(n_rec=4, seed=3)
    for r in range(4):
        m = imu["meas"][imu["start"][r]:imu["start"][r + 1]]
        C.append(synth_imu.integrate64(m, imu["bias"][r], Nga, [ngw ** 2] * 3 + [naw ** 2] * 3)[-225:].reshape(15, 15))
    return [np.asarray(c, np.float32) for c in C]


def _negative_direction(C):
    """C with its strongest eigen-direction's eigenvalue replaced by -1e-3 (then cast to float as the product's is)."""
    c9 = C[:9, :9].astype(np.float64)
    w, V = np.linalg.eigh((c9 + c9.T) / 2)
    out = C.copy()
    out[:9, :9] = (c9 + (-1e-3 - w[-1]) * np.outer(V[:, -1], V[:, -1])).astype(np.float32)
    return out


def _huge_axis(C, k):
    """C with coordinate k cut loose and given the variance 1e14 (exactly representable as a float matrix): the
    inverse's eigenvalue 1e-14 lies below the 1e-12 cut."""
    out = C.copy()
    out[k, :9] = out[:9, k] = 0.0
    out[k, k] = 1e14
    return out


def test_inertial_info9_both_variants(torch_cuda):
    plain = _covariances()
    neg = [_negative_direction(c) for c in plain[:4]]                 # inverse eigenvalue about -1e3: zeroed
    huge = [_huge_axis(c, k) for c, k in zip(plain[:4], (8, 0, 4, 6))]   # inverse eigenvalue 1e-14 < 1e-12: zeroed
    C = plain + neg + huge
    got = {par: selftest.inertial_info9(np.stack(C), par) for par in (False, True)}
    worst = {}
    for i, Ci in enumerate(C):
        exact, ev = ref.mp_inertial_info9(Ci)
        clamped = [v for v in ev if v < 1e-12]
        kept = [v for v in ev if not v < 1e-12]
        assert len(clamped) == (0 if i < len(plain) else 1)
        # clear of the 1e-12 cut by 100 x on both sides
        assert all(v <= 1e-14 * (1 + 1e-6) for v in clamped) and min(kept) >= 1e-10
        kappa = float(max(kept) / min(kept))
        c9 = Ci[:9, :9].astype(np.float64)
        I = np.linalg.inv(c9)
        w, V = np.linalg.eigh((I + I.T) / 2)
        w = np.where(w < 1e-12, 0.0, w)
        e_ref = ref.forward_error((V * w) @ V.T, exact.ravel())
        for par in (False, True):
            info, path = got[par]
            want = 2 if clamped else (0 if par else 1)
            assert path[i] == want, (i, par, path[i], want)
            e = ref.forward_error(info[i], exact.ravel())
            _report(f"inertial_info9<{par}> case {i} path {want}", e, e_ref, 9, kappa)
            assert e <= ref.solve_bound(9, kappa, e_ref), (i, par, e, e_ref, kappa)
            worst[(par, want)] = max(worst.get((par, want), (0.0, 0.0)), (e / (9 * ref.U * kappa), e / e_ref))
    print(f"[linalg] inertial_info9 worst e/(n u kappa), its e/e_ref per (variant, path): {worst}")


# ---- the reduced system: windows, plans, the solve --------------------------------------------------------------
def _solver(prob):
    return LocalInertialBA(max_kf=prob["n_kf"], max_cams=prob["n_cams"], max_pts=len(prob["pts"]),
                           max_mono=len(prob["mono_pt"]) + int(prob.get("n_stereo", 0)),
                           max_imu=max(1, len(prob["imu_kf1"])))


MONO = ("mono_pt", "mono_kf", "mono_cam", "mono_obs", "mono_inv_sigma2")


def _keep_mono(prob, keep):
    for k in MONO:
        prob[k] = np.asarray(prob[k])[keep]
    return prob


def _add_views(prob, pts, kfs, rng):
    """EdgeMono observations of the points `pts` from every keyframe of `kfs` whose camera (the point's first one) sees
    it: projection of the true point through the true pose + N(0, 0.7 px)."""
    tr = prob["truth"]
    cams = np.asarray(prob["cam"], np.float64)
    add = {k: [] for k in MONO}
    for p in pts:
        c = int(np.asarray(prob["mono_cam"])[np.flatnonzero(np.asarray(prob["mono_pt"]) == p)[0]])
        seen = set(np.asarray(prob["mono_kf"])[(np.asarray(prob["mono_pt"]) == p) & (np.asarray(prob["mono_cam"]) == c)])
        for k in kfs:
            if k in seen:
                continue
            Rcw = prob["Rcb"][c] @ tr["Rwb"][k].T
            X = Rcw @ (tr["pts"][p] - tr["twb"][k]) + prob["tcb"][c]
            if X[2] < 0.3:
                continue
            uv = synth_ba.kb8_project(cams[c], X)
            if not (5 <= uv[0] <= 715 and 5 <= uv[1] <= 535):
                continue
            add["mono_pt"].append(p), add["mono_kf"].append(k), add["mono_cam"].append(c)
            add["mono_obs"].append(uv + rng.normal(0, 0.7, 2)), add["mono_inv_sigma2"].append(1.0)
    for k in MONO:
        a = np.asarray(prob[k])
        prob[k] = np.concatenate([a, np.asarray(add[k], a.dtype).reshape((-1,) + a.shape[1:])])
    return prob


def _visual_only(prob):
    prob["kf_imu"] = np.zeros(prob["n_kf"], np.uint8)
    for k in ("imu_kf1", "imu_kf2", "preint", "imu_robust", "imu_info_scale"):
        prob[k] = prob[k][:0]
    return prob


def _awkward_landmarks(prob, rng):
    """Landmarks seen by fixed keyframes only, landmarks without edges, and one with more edges than a build group holds
    (> 256: build_big_kernel's records enter the assembly)."""
    n_opt = prob["n_opt"]
    pt, kf = np.asarray(prob["mono_pt"]), np.asarray(prob["mono_kf"])
    both = [p for p in range(60) if (kf[pt == p] < n_opt).any() and (kf[pt == p] >= n_opt).any()]
    fixed_only, heavy = both[:8], max(both[8:], key=lambda p: ((pt == p) & (kf < n_opt)).sum())
    prob["fixed_only"] = fixed_only
    _keep_mono(prob, ~(np.isin(pt, fixed_only) & (kf < n_opt)))
    if prob.get("n_stereo", 0):
        keep = ~(np.isin(prob["stereo_pt"], fixed_only) & (np.asarray(prob["stereo_kf"]) < n_opt))
        for k in ("stereo_pt", "stereo_kf", "stereo_obs", "stereo_inv_sigma2"):
            prob[k] = np.asarray(prob[k])[keep]
        prob["n_stereo"] = int(keep.sum())
    sel = np.flatnonzero(np.asarray(prob["mono_pt"]) == heavy)
    rep = np.tile(sel, 300 // len(sel) + 1)
    assert len(rep) > 256
    for k in MONO:
        a = np.asarray(prob[k])
        new = a[rep] + (rng.normal(0, 0.5, (len(rep), 2)) if k == "mono_obs" else 0)
        prob[k] = np.concatenate([a, new.astype(a.dtype)])
    extra = np.asarray(prob["pts"])[:5] + rng.normal(0, 0.5, (5, 3))   # edgeless
    prob["pts"] = np.concatenate([prob["pts"], extra])
    prob["pt_track_depth"] = np.concatenate([prob["pt_track_depth"], np.full(5, 10.0, np.float32)])
    return prob


def _window(case):
    """The windows of the plan table (module docstring).  Returns (problem, expectations)."""
    rng = np.random.default_rng(77)
    visual = case.endswith("_visual") or case.endswith("_stereo")
    stereo = 0.5 if case.endswith("_stereo") else 0.0
    base = case.split("_")[0]
    if base == "chain3":
        prob = dict(synth_ba.make_lba_problem(n_kf=6, n_opt=3, n_pts=150, seed=2, n_cams=3, stereo_frac=stereo))
        expect = dict(mode=1, n_lev=3, cols=[1, 1, 1], n_slots=6)
    elif base in ("dense12", "dense13"):
        n_opt = int(base[5:])
        prob = dict(synth_ba.make_lba_problem(n_kf=n_opt + 2, n_opt=n_opt, n_pts=260, seed=4, n_cams=3,
                                              stereo_frac=stereo))
        far = [p for p in range(60, 260) if np.linalg.norm(prob["truth"]["pts"][p] - prob["truth"]["twb"][n_opt // 2]) > 8]
        _add_views(prob, far[:24], range(n_opt), rng)
        expect = dict(mode=1 if n_opt == 12 else 2, n_slots=n_opt * (n_opt + 1) // 2, n_lev=n_opt, cols=[1] * n_opt)
    elif base == "clusters14":
        prob = dict(synth_ba.make_lba_problem(n_kf=16, n_opt=14, n_pts=300, seed=6, n_cams=3))
        pt, kf = np.asarray(prob["mono_pt"]), np.asarray(prob["mono_kf"])
        lo = np.zeros(len(prob["pts"]), bool)
        hi = np.zeros(len(prob["pts"]), bool)
        lo[pt[kf <= 6]] = True
        hi[pt[(kf >= 7) & (kf < 14)]] = True
        _keep_mono(prob, ~(lo & hi)[pt])   # no landmark joins the clusters: only the IMU edge 6 - 7 does
        expect = dict(mode=1)
    else:
        raise AssertionError(case)
    if visual:
        _visual_only(prob)
        _awkward_landmarks(prob, rng)
    return prob, expect


WINDOWS = ["chain3", "dense12", "dense13", "clusters14", "chain3_visual", "dense13_visual", "chain3_stereo",
           "dense13_stereo"]


@pytest.fixture(scope="module")
def windows():
    cache = {}

    def get(case):
        if case not in cache:
            prob, expect = _window(case)
            cache[case] = (prob, expect, _solver(prob).set_problem(prob))
        return cache[case]
    return get


def _coupled(prob):
    """Indices (16 k + r) of the coupled unknowns, and of the padding rows, in keyframe order."""
    dof = 15 if len(prob["imu_kf1"]) else 6
    idx = np.arange(16 * prob["n_opt"])
    return idx[idx % 16 < dof], idx[idx % 16 >= dof]


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("case", WINDOWS)
def test_reduced_system_plan_padding_and_solve(torch_cuda, windows, case, lam):
    prob, expect, ba = windows(case)
    r = ba.debug_solve(lam)
    S, rhs, x = r["S"], r["rhs"], r["x"]
    n_opt = prob["n_opt"]
    # the plan the case is named for
    print(f"[linalg] plan {case}: mode {r['mode']} slots {r['n_slots']} lds {r['n_lds']} levels {r['n_lev']} cols {r['cols']}")
    for k, v in expect.items():
        assert r[k] == v, (case, k, r[k], v)
    assert sum(r["cols"]) == n_opt and min(r["cols"]) >= 1
    if r["mode"] == 2:
        assert 0 < r["n_lds"] < r["n_slots"], r
    else:
        assert r["n_lds"] == r["n_slots"], r
    if case.startswith("clusters"):
        assert max(r["cols"]) >= 2 and r["n_lev"] < n_opt, r
    assert r["fail"] == 0
    # 1. padding rows: zero off the diagonal, lambda on it, zero right-hand side, solved to exactly 0
    core, pad = _coupled(prob)
    assert len(pad) == n_opt * (1 if len(prob["imu_kf1"]) else 10)
    off = S[pad].copy()
    off[np.arange(len(pad)), pad] = 0
    assert not off.any() and np.array_equal(S[pad, pad], np.full(len(pad), lam))
    assert not rhs[pad].any() and not x[pad].any()
    # 2. symmetric, finite
    assert np.array_equal(S, S.T) and np.isfinite(S).all() and np.isfinite(rhs).all()
    # 3. x against the refined solution of the returned system (its coupled part: the padding decouples exactly)
    Sc, bc = S[np.ix_(core, core)], rhs[core]
    terms, _ = ref.refine_solve(Sc, bc)
    _, exact = ref.sum_terms(terms)
    kappa = ref.rayleigh_cond_lower_bound(Sc)
    e, e_ref = ref.forward_error(x[core], exact), ref.forward_error(np.linalg.solve(Sc, bc), exact)
    _report(f"lba solve {case} lambda {lam:g}", e, e_ref, len(core), kappa)
    assert e <= ref.solve_bound(len(core), kappa, e_ref), (case, lam, e, e_ref, kappa)


def test_reduced_system_nan_observation_fails(torch_cuda):
    prob, _ = _window("chain3")
    obs = np.array(prob["mono_obs"], np.float64)
    obs[int(np.flatnonzero(np.asarray(prob["mono_kf"]) < prob["n_opt"])[0]), 0] = np.nan
    prob["mono_obs"] = obs
    r = _solver(prob).set_problem(prob).debug_solve(1e-2)
    assert r["fail"] != 0


def test_debug_solve_rejects_zero_lambda(torch_cuda, windows):
    from openmavis_amd import _lib
    _, _, ba = windows("chain3")
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.OmvError):
            ba.debug_solve(lam)


# ---- the reduced system itself against the Schur complement -------------------------------------------------------
def _schur(prob, ev, lam, dt):
    """S (6 x 6 pose blocks, [n_opt][n_opt][6][6]) and rhs ([n_opt][6]) of a visual-only window from the edges' residuals
    and Jacobians, with g2o's first-order Huber weights, in the float type `dt`; and the entrywise absolute
    accumulations of both."""
    n_opt, P = prob["n_opt"], len(prob["pts"])
    nm = len(prob["mono_pt"])
    ns = int(prob.get("n_stereo", 0))
    pt = np.concatenate([prob["mono_pt"], prob["stereo_pt"] if ns else []]).astype(np.int64)
    kf = np.concatenate([prob["mono_kf"], prob["stereo_kf"] if ns else []]).astype(np.int64)
    wi = np.concatenate([prob["mono_inv_sigma2"], prob["stereo_inv_sigma2"] if ns else []]).astype(np.float32).astype(dt)
    E = nm + ns
    err, JX, JP = np.zeros((E, 3), dt), np.zeros((E, 3, 3), dt), np.zeros((E, 3, 6), dt)
    err[:nm, :2], JX[:nm, :2], JP[:nm, :2] = ev["mono_err"], ev["mono_jx"].reshape(-1, 2, 3), ev["mono_jp"].reshape(-1, 2, 6)
    if ns:
        err[nm:], JX[nm:], JP[nm:] = ev["stereo_err"], ev["stereo_jx"].reshape(-1, 3, 3), ev["stereo_jp"].reshape(-1, 3, 6)
    chi2 = wi * (err * err).sum(1)
    delta = np.where(np.arange(E) < nm, dt(np.float32(np.sqrt(5.991))), dt(np.float32(np.sqrt(7.815))))
    rho1 = np.where(chi2 <= delta * delta, dt(1), delta / np.sqrt(np.maximum(chi2, dt(1e-300))))
    w = wi * rho1
    opt = kf < n_opt
    Hll, Hll_abs = np.zeros((P, 3, 3), dt), np.zeros((P, 3, 3), dt)
    bl, bl_abs = np.zeros((P, 3), dt), np.zeros((P, 3), dt)
    t = w[:, None, None] * np.einsum("eri,erj->eij", JX, JX)
    np.add.at(Hll, pt, t)
    np.add.at(Hll_abs, pt, np.abs(w[:, None, None]) * np.einsum("eri,erj->eij", np.abs(JX), np.abs(JX)))
    np.add.at(bl, pt, -w[:, None] * np.einsum("eri,er->ei", JX, err))
    np.add.at(bl_abs, pt, w[:, None] * np.einsum("eri,er->ei", np.abs(JX), np.abs(err)))
    S, A = np.zeros((n_opt, n_opt, 6, 6), dt), np.zeros((n_opt, n_opt, 6, 6), dt)
    b, b_abs = np.zeros((n_opt, 6), dt), np.zeros((n_opt, 6), dt)
    eo = np.flatnonzero(opt)
    np.add.at(S, (kf[eo], kf[eo]), w[eo, None, None] * np.einsum("eri,erj->eij", JP[eo], JP[eo]))
    np.add.at(A, (kf[eo], kf[eo]), w[eo, None, None] * np.einsum("eri,erj->eij", np.abs(JP[eo]), np.abs(JP[eo])))
    np.add.at(b, kf[eo], -w[eo, None] * np.einsum("eri,er->ei", JP[eo], err[eo]))
    np.add.at(b_abs, kf[eo], w[eo, None] * np.einsum("eri,er->ei", np.abs(JP[eo]), np.abs(err[eo])))
    for k in range(n_opt):
        S[k, k] += dt(lam) * np.eye(6, dtype=dt)
        A[k, k] += dt(lam) * np.eye(6, dtype=dt)
    Wpl = w[eo, None, None] * np.einsum("eri,erj->eij", JP[eo], JX[eo])   # [e][6][3]
    for p in np.unique(pt[eo]):
        sel = np.flatnonzero(pt[eo] == p)
        ks = np.unique(kf[eo][sel])
        W = np.zeros((len(ks), 6, 3), dt)
        np.add.at(W, np.searchsorted(ks, kf[eo][sel]), Wpl[sel])
        D = Hll[p] + dt(lam) * np.eye(3, dtype=dt)
        c = np.array([[D[(i + 1) % 3, (j + 1) % 3] * D[(i + 2) % 3, (j + 2) % 3] -
                       D[(i + 1) % 3, (j + 2) % 3] * D[(i + 2) % 3, (j + 1) % 3] for j in range(3)] for i in range(3)], dt)
        Dinv = c.T / (D[0] @ c[0])   # adjugate / determinant
        T = W @ Dinv
        S[np.ix_(ks, ks)] -= np.einsum("aij,bkj->abik", T, W)
        A[np.ix_(ks, ks)] += np.einsum("aij,bkj->abik", np.abs(W) @ np.abs(Dinv), np.abs(W))
        b[ks] -= T @ bl[p]
        b_abs[ks] += (np.abs(W) @ np.abs(Dinv)) @ bl_abs[p]
    return S, b, A, b_abs


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("case", [c for c in WINDOWS if c.endswith(("_visual", "_stereo"))])
def test_reduced_system_is_the_schur_complement(torch_cuda, windows, case, lam):
    prob, _, ba = windows(case)
    assert np.finfo(np.longdouble).eps < 2e-19, "the Schur reference needs the 80-bit long double"
    n_opt = prob["n_opt"]
    pt, kf = np.asarray(prob["mono_pt"]), np.asarray(prob["mono_kf"])
    # the awkward landmarks are there: fixed-only, edgeless, and one heavy enough for build_big_kernel
    assert len(prob["fixed_only"]) == 8 and all((kf[pt == p] >= n_opt).all() and (pt == p).any() for p in prob["fixed_only"])
    assert not np.isin(np.arange(len(prob["pts"]) - 5, len(prob["pts"])), pt).any()
    assert np.bincount(pt).max() > 256
    if case.endswith("_stereo"):
        assert (np.asarray(prob["stereo_kf"]) < n_opt).sum() > 20
    ev = ba.evaluate()
    r = ba.debug_solve(lam)
    assert r["fail"] == 0
    q = (16 * np.arange(n_opt)[:, None] + np.arange(6)[None, :]).ravel()
    got_S = r["S"][np.ix_(q, q)].reshape(n_opt, 6, n_opt, 6).transpose(0, 2, 1, 3)
    got_b = r["rhs"][q].reshape(n_opt, 6)
    S_hi, b_hi, A, b_abs = _schur(prob, ev, lam, np.longdouble)
    S_64, b_64, _, _ = _schur(prob, ev, lam, np.float64)
    live = A > 0
    assert not got_S[~live].any()   # blocks no edge reaches stay exactly zero
    eS = float((np.abs(got_S.astype(np.longdouble) - S_hi)[live] / A[live]).max())
    eS_ref = float((np.abs(S_64.astype(np.longdouble) - S_hi)[live] / A[live]).max())
    lb = b_abs > 0
    eb = float((np.abs(got_b.astype(np.longdouble) - b_hi)[lb] / b_abs[lb]).max())
    eb_ref = float((np.abs(b_64.astype(np.longdouble) - b_hi)[lb] / b_abs[lb]).max())
    print(f"[linalg] schur {case} lambda {lam:g}: S {eS:.3e} (numpy {eS_ref:.3e}, ratio {eS / eS_ref:.3g}); "
          f"rhs {eb:.3e} (numpy {eb_ref:.3e}, ratio {eb / eb_ref:.3g})")
    assert eS <= 8 * eS_ref, (case, lam, eS, eS_ref)
    assert eb <= 8 * eb_ref, (case, lam, eb, eb_ref)


# ---- inv16 ------------------------------------------------------------------------------------------------------
def _check_inv16(blocks, dofs, labels):
    full = []
    for D in blocks:
        F = np.tril(D) + np.tril(D, -1).T
        U = F.copy()
        U[np.triu_indices(16, 1)] = np.nan   # only the lower triangle may be read
        full.append((F, U))
    inv, bad = selftest.inv16(np.stack([u for _, u in full]))
    worst = (0.0, 0.0)
    for i, (F, _) in enumerate(full):
        d = dofs[i]
        assert bad[i] == 0, labels[i]
        core = F[:d, :d]
        lam = F[d:, d:].diagonal()
        assert not F[d:, :d].any() and np.array_equal(F[d:, d:], np.diag(lam))
        # the padding: exactly decoupled, each pivot the 1 x 1 system it is (3 n u kappa_2 with n = kappa_2 = 1)
        assert not inv[i][d:, :d].any() and not inv[i][:d, d:].any() and not (inv[i][d:, d:] - np.diag(inv[i][d:, d:].diagonal())).any()
        for v, l in zip(inv[i][d:, d:].diagonal(), lam):
            assert abs(Fraction(float(v)) * Fraction(float(l)) - 1) <= 3 * Fraction(ref.U), (labels[i], v, l)
        _, Em = ref.mp_inverse(core)
        ex = [Em[r, c] for r in range(d) for c in range(d)]
        wv, _ = ref.mp_eigsy(core)
        kappa = float(max(wv) / min(wv))
        assert min(wv) > 0
        e, e_ref = ref.forward_error(inv[i][:d, :d], ex), ref.forward_error(np.linalg.inv(core), ex)
        _report(f"inv16 {labels[i]}", e, e_ref, d, kappa)
        assert e <= ref.solve_bound(d, kappa, e_ref), (labels[i], e, e_ref, kappa)
        worst = max(worst, (e / (d * ref.U * kappa), e / e_ref))
    print(f"[linalg] inv16 worst e/(n u kappa), its e/e_ref: {worst}")


def test_inv16_synthetic_sweep(torch_cuda):
    rng = np.random.default_rng(16)
    blocks, dofs, labels = [], [], []
    for d in (15, 6):
        for kappa in (1e2, 1e6, 1e10):
            for lam in (1e-9, 1e-2, 1e3):
                D = np.zeros((16, 16))
                D[:d, :d] = _spd(d, kappa, rng) * 10.0 ** rng.integers(-2, 7)
                D[np.arange(d, 16), np.arange(d, 16)] = lam
                blocks.append(D), dofs.append(d), labels.append(f"{d}+{16 - d} kappa {kappa:g} lambda {lam:g}")
    _check_inv16(blocks, dofs, labels)


def test_inv16_real_diagonal_blocks(torch_cuda, windows):
    blocks, dofs, labels = [], [], []
    for case, d in (("chain3", 15), ("dense13", 15), ("chain3_visual", 6), ("dense13_visual", 6)):
        prob, _, ba = windows(case)
        for lam in (1e-9, 1e-2, 1e3):
            S = ba.debug_solve(lam)["S"]
            for k in (0, prob["n_opt"] - 1):
                blocks.append(S[16 * k:16 * k + 16, 16 * k:16 * k + 16].copy()), dofs.append(d)
                labels.append(f"{case} keyframe {k} lambda {lam:g}")
    _check_inv16(blocks, dofs, labels)


def test_inv16_flags_zero_pivot_and_nan(torch_cuda):
    rng = np.random.default_rng(17)
    good = _spd(16, 1e2, rng)
    zero = good.copy()
    zero[0, :] = zero[:, 0] = 0.0          # a zero first pivot
    late = good.copy()
    late[15, :] = late[:, 15] = 0.0        # a zero last pivot (the padding pivot with lambda = 0)
    nan = good.copy()
    nan[9, 4] = nan[4, 9] = np.nan         # a NaN below the diagonal
    nand = good.copy()
    nand[7, 7] = np.nan
    inv, bad = selftest.inv16(np.stack([good, zero, late, nan, nand]))
    assert list(bad) == [0, 1, 1, 1, 1], list(bad)
    assert np.isfinite(inv[0]).all() and not np.isfinite(inv[1]).all()
