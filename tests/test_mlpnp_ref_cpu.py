"""tests/mlpnp_ref.py, the float64 restatement of src/MLPnPsolver.cpp the device MLPnPsolver is tested against, checked
on its own: it recovers planted poses, its SetRansacParameters tables are the reference's, its compact Jacobian is the
derivative of its residual, its iterate replay keeps the reference's quirks, and the case lists of
tests/test_mlpnp_gpu.py leave few enough hypotheses out of a comparison."""
import numpy as np
import pytest

import mlpnp_cases as cases
import mlpnp_ref as ref
from openmavis_amd import synth_pnp
from openmavis_amd.sim3solver import draw

KB8, PIN = 0, 1


# ---- planted poses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [KB8, PIN])
@pytest.mark.parametrize("scene", ["general", "planar", "identity"])
def test_planted_pose_is_recovered_noise_free(scene, model):
    """Noise-free pixels are still rounded to float32 (about 3e-5 px, 1e-7 rad at f = 380 px); with the conditioning
    of these scenes (up to a few tens) the pose is expected within 1e-5."""
    job = synth_pnp.make_job(40, 3, model, scene, noise_px=0.0)
    pre = ref.prepare(job)
    for sel in (np.arange(40), np.arange(6), np.array([5, 11, 17, 23, 29, 35, 39])):
        r = ref.compute_pose(pre["f"][sel], pre["ns"][sel], pre["Xw"][sel])
        assert r["planar"] == (scene == "planar")
        if scene == "identity" and not np.isfinite(r["t"]).all():
            continue   # w == 0 exactly: the reference divides by zero (:797), see test_identity_pose_can_end_non_finite
        assert np.abs(r["R"] - job["Rcw"]).max() < 1e-5 and np.abs(r["t"] - job["tcw"]).max() < 1e-5, (sel, r)
        mask, count = ref.check_inliers(job, pre, r["R"], r["t"])
        assert count == 40 and mask.all()


@pytest.mark.parametrize("model", [KB8, PIN])
def test_rank_one_scene_takes_the_twelve_column_branch(model):
    """Every world point on one line through the origin: sum p p^T has rank 1, which is not the planar branch.  The
    pose is not observable there (A^T A has a null space of more than one dimension, kappa is infinite or beyond 1e8),
    so nothing is claimed about its value."""
    job = synth_pnp.make_job(40, 4, model, "rank1", noise_px=0.0)
    pre = ref.prepare(job)
    assert ref.fullpiv_rank3(pre["Xw"].T @ pre["Xw"]) == 1
    r = ref.compute_pose(pre["f"], pre["ns"], pre["Xw"])
    assert not r["planar"] and not r["kappa_final"] <= 1e8 and r["near"]


def test_rank_of_exactly_planar_and_general_points():
    for scene, rank in (("planar", 2), ("general", 3)):
        job = synth_pnp.make_job(30, 8, PIN, scene)
        X = job["Xw"].astype(np.float64)
        assert ref.fullpiv_rank3(X.T @ X) == rank == np.linalg.matrix_rank(X.T @ X, tol=1e-9 * np.abs(X.T @ X).max())


def test_identity_pose_can_end_non_finite():
    """With Tcw = I the linear stage returns a rotation within an ulp of I; where its trace is >= 3, rot2rodrigues
    gives w == 0 exactly and the Jacobian's sin(|w|) / |w| is 0 / 0: a non-finite pose and no inliers."""
    job = synth_pnp.make_job(20, 6, PIN, "identity", noise_px=0.0)
    rs = ref.RefSolver(job)
    d = draw(np.random.default_rng(1), 64, 20, 6)
    hyps = [rs.hypothesis(r) for r in d]
    bad = [h for h in hyps if not np.isfinite(h["t"]).all()]
    assert bad and all(h["count"] == 0 and h["reason"] == ref.GN_NAN for h in bad)
    assert all(h["count"] == 20 for h in hyps if np.isfinite(h["t"]).all() and h["reason"] == ref.GN_EPSP)


# ---- the Householder nullspace -----------------------------------------------------------------------------------------
def test_nullspace_is_the_householder_reflector():
    rng = np.random.default_rng(2)
    for _ in range(50):
        f = np.array([rng.normal(), rng.normal(), 1.0])
        N = ref.householder_nullspace(f)
        assert np.abs(N.T @ f).max() < 1e-15 * np.linalg.norm(f) * 4 and np.abs(N.T @ N - np.eye(2)).max() < 1e-15
        # the reflector maps f to beta e0 with beta = -sign(f0) |f|
        H = np.column_stack([np.cross(N[:, 0], N[:, 1]), N])
        assert abs(abs(np.linalg.det(H)) - 1) < 1e-14
    assert np.array_equal(ref.householder_nullspace([2.0, 0.0, 0.0]), np.eye(3)[:, 1:3])   # tau = 0


# ---- SetRansacParameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,params,expected", [
    (200, ref.TRACKING, (35, 100)),     # int(200 * 0.5f) = 100; eps 0.5: ceil(log 0.01 / log(1 - 0.125)) = ceil(34.49)
    (130, ref.TRACKING, (35, 65)),
    (100, ref.DEFAULTS, (70, 40)),      # eps 0.4: ceil(4.605 / 0.06614) = ceil(69.6)
    (15, ref.TRACKING, (14, 10)),       # int(7.5) = 7 -> minInliers 10; eps 10 / 15: ceil(4.605 / 0.3514) = ceil(13.1)
    (7, ref.DEFAULTS, (1, 8)),          # minInliers 8 > N: eps > 1, log of a negative number -> NaN -> INT_MIN -> 1
    (6, (0.99, 6, 300, 6, 0.4), (1, 6)),    # minInliers == N: nIterations = 1
    (6, ref.TRACKING, (1, 10)),
    (5, ref.TRACKING, (1, 10)),
    (0, ref.TRACKING, (1, 10)),
    (20, (0.99, 2, 300, 6, 0.1), (300, 6)),   # the minSet clamp; eps 0.3: 168.2 -> 169
    (1000, (0.99, 10, 20, 6, 0.5), (20, 500)),   # the maxIterations clamp
])
def test_ransac_parameter_tables(n, params, expected):
    got = ref.ransac_parameters(n, *params[:5])
    if n == 20:
        expected = (min(300, int(np.ceil(np.log(0.01) / np.log(1 - float(np.float32(6) / np.float32(20)) ** 3)))), 6)
    assert got == expected


# ---- the compact Jacobian --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-3, 2.5])
def test_jacobian_agrees_with_central_differences(scale):
    job = synth_pnp.make_job(20, 5, KB8, "general")
    pre = ref.prepare(job)
    x = np.concatenate([ref.rot2rodrigues(job["Rcw"]) * scale / max(scale, 1.0), job["tcw"]]) + 0.01 * scale
    r, J = ref.residuals_and_jac(x, pre["Xw"], pre["ns"])
    assert np.allclose(r, ref.residuals(x, pre["Xw"], pre["ns"]), rtol=0, atol=1e-15)
    h = 1e-6
    Jn = np.stack([(ref.residuals(x + h * e, pre["Xw"], pre["ns"]) - ref.residuals(x - h * e, pre["Xw"], pre["ns"])) /
                   (2 * h) for e in np.eye(6)], 1)
    # central differences: h^2 |f'''| / 6 + eps |f| / h, about 1e-10 for residuals of order one
    assert np.abs(J - Jn).max() < 1e-8 * max(1.0, np.abs(J).max()), np.abs(J - Jn).max()


def test_jacobian_divides_by_zero_at_w_zero():
    job = synth_pnp.make_job(8, 5, PIN, "general")
    pre = ref.prepare(job)
    r, J = ref.residuals_and_jac(np.array([0, 0, 0, 0.1, 0.2, 0.3]), pre["Xw"], pre["ns"])
    assert np.isfinite(r).all() and not np.isfinite(J[:, :3]).any()


# ---- sampling ------------------------------------------------------------------------------------------------------
def test_sampling_replay_equals_the_literal_list():
    for n in (6, 7, 8):
        rng = np.random.default_rng(n)
        for _ in range(400):
            r = [int(rng.integers(0, n - i)) for i in range(6)]
            a = ref.sample_literal(n, r)
            assert a == ref.sample_replay(n, r) and len(set(a)) == 6
    assert ref.sample_literal(9, [99, -5, 3, 3, 3, 0]) == ref.sample_replay(9, [99, -5, 3, 3, 3, 0])   # clamped


# ---- the iterate replay ----------------------------------------------------------------------------------------------
def _run(counts, refine_table, n_it, n_draws, n=50, min_inl=10, max_its=8, st=None):
    calls = []

    def refine(h):
        calls.append(h)
        return refine_table[h]

    st = ref.new_state() if st is None else st
    return ref.replay_call(st, counts, refine, n_it, n_draws, n, min_inl, max_its), calls, st


def test_iterate_or_loop_runs_the_whole_ransac_on_the_first_call():
    out, calls, st = _run([0] * 20, {}, 5, 20)        # max(5, 8 - 0) hypotheses, then exhausted
    assert (out["done"], out["flags"], st["iterations"]) == (8, ref.NO_MORE, 8) and not calls
    out, calls, st = _run([0] * 20, {}, 5, 20, st=st)   # a later call still runs nIterations
    assert (out["done"], out["flags"], st["iterations"]) == (5, ref.NO_MORE, 13)
    out, _, st = _run([0] * 20, {}, 12, 20)           # nIterations beyond mRansacMaxIts
    assert (out["done"], st["iterations"]) == (12, 12)
    out, _, st = _run([0] * 3, {}, 5, 3)              # fewer draws than the call would run: not exhausted
    assert (out["done"], out["flags"]) == (3, 0)


def test_iterate_comparisons_and_kept_refine_outcome():
    # count >= minInliers qualifies (10 does), the best is replaced only by a strictly greater count (the second 12 is
    # not a new best), Refine runs once per distinct best, and succeeds only above minInliers (strictly)
    counts = [9, 10, 12, 12, 11, 15, 3, 3]
    table = {1: (10, False), 2: (9, False), 5: (11, True)}
    out, calls, st = _run(counts, table, 5, 8)
    assert calls == [1, 2, 5] and out["bests"] == [1, 2, 5]
    assert (out["flags"], out["kind"], out["n_inliers"], out["done"], st["best"]) == (ref.FOUND, 1, 11, 6, 15)
    # a later call returns the kept outcome at its first qualifying hypothesis, without a new Refine
    out, calls, st = _run([0, 0, 10, 99], {}, 4, 4, st=st)
    assert (out["flags"], out["kind"], out["n_inliers"], out["done"]) == (ref.FOUND, 1, 11, 3) and not calls
    assert st["iterations"] == 9
    # Refine fails on one best and succeeds on a later one
    out, calls, _ = _run([20, 0, 21, 0], {0: (10, False), 2: (30, True)}, 4, 4, max_its=4)
    assert calls == [0, 2] and (out["flags"], out["n_inliers"], out["done"]) == (ref.FOUND, 30, 3)


def test_iterate_exhaustion_returns_the_unrefined_best():
    out, calls, st = _run([0, 12, 0, 11, 0, 0, 0, 0], {1: (10, False)}, 5, 8)
    assert calls == [1] and (out["flags"], out["kind"], out["n_inliers"]) == (ref.NO_MORE | ref.FOUND, 2, 12)
    out, _, _ = _run([0] * 8, {}, 5, 8)
    assert (out["flags"], out["kind"], out["n_inliers"]) == (ref.NO_MORE, 0, 0)
    out, calls, _ = _run([50] * 8, {}, 5, 8, n=9)     # N < mRansacMinInliers: bNoMore, no work
    assert (out["flags"], out["done"]) == (ref.NO_MORE, 0) and not calls


@pytest.mark.parametrize("outliers,model", [(0.4, KB8), (0.75, PIN)])
def test_kept_refine_outcome_equals_refine_at_every_hypothesis(outliers, model):
    """Refine is a pure function of mvbBestInliers: evaluating it once per distinct best gives the calls the
    reference's text gives, over two consecutive iterate calls."""
    job = synth_pnp.make_job(40, 9, model, "general", outlier_share=outliers)
    a, b = ref.RefSolver(job), ref.RefSolver(job)
    for s in (a, b):
        s.SetRansacParameters(0.99, 10, 12, 6, 0.5, 5.991)
    rng = np.random.default_rng(4)
    for n_it in (5, 5):
        d = draw(rng, 12, 40, 6)
        x = a.iterate(n_it, d)
        flags, n_inl, T, vb = b.iterate_literal(n_it, d)
        assert (x["flags"], x["n_inliers"]) == (flags, n_inl)
        assert x["T"].tobytes() == T.tobytes() and np.array_equal(x["vb"], vb)
    assert a.n_refine_calls <= b.n_refine_calls


# ---- the GPU tests' case lists -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.B_CASES, ids=lambda c: f"N{'-'.join(map(str, c[0]))}-{c[6]}")
def test_left_out_share_of_the_compute_pose_cases(case):
    jobs, draws = cases.make(case)
    for job, d in zip(jobs, draws):
        rs = ref.RefSolver(job)
        near = sum(rs.pose_of(ref.sample_replay(rs.n, r))["near"] for r in d)
        assert near <= cases.LEFT_OUT_CAP * len(d), (len(job["index"]), near, len(d))


@pytest.mark.parametrize("case", cases.C_CASES, ids=lambda c: f"N{'-'.join(map(str, c[0]))}-{c[6]}")
def test_band_share_of_the_check_inliers_cases(case):
    jobs, draws = cases.make(case)
    tot = band = 0
    for job, d in zip(jobs, draws):
        rs = ref.RefSolver(job)
        for r in d:
            h = rs.hypothesis(r)
            if np.isfinite(h["t"]).all():
                e = ref.reprojection_errors(job, rs.pre, h["R"], h["t"])
                band += int((np.abs(e - rs.pre["max_err"]) <= cases.DELTA * rs.pre["max_err"]).sum())
            tot += rs.n
    assert band <= cases.BAND_CAP * tot, (band, tot)
