"""The visual bundle adjustment's numpy reference (tests/vba_ref.py) checked against itself, and the conditions the GPU
parity test (tests/test_vba_gpu.py) relies on, asserted on the reference alone."""
import numpy as np
import pytest

import vba_cases
import vba_ref
from openmavis_amd import synth_vba


def _exp_series(u, terms=40):
    """exp of the 4 x 4 twist matrix by its power series: (R, t)."""
    A = np.zeros((4, 4))
    A[:3, :3], A[:3, 3] = vba_ref.skew(u[:3]), u[3:]
    M, T = np.eye(4), np.eye(4)
    for n in range(1, terms):
        T = T @ A / n
        M = M + T
    return M[:3, :3], M[:3, 3]


@pytest.mark.parametrize("u", [[1e-7, -2e-7, 1.5e-7, 0.3, -0.2, 0.1], [2e-6, 1e-6, -3e-6, 1.0, 2.0, -1.0],
                               [0.01, -0.02, 0.015, 0.1, 0.2, -0.3], [0.7, -0.4, 0.9, -1.0, 0.5, 2.0],
                               [2.0, 1.5, -1.0, 0.3, 0.1, -0.2]])
def test_exp_against_series(u):
    """Small angles and large ones.  Below theta = 1e-5 SE3Quat::exp takes R = V = I + W + W^2 where the series has
    I + W + W^2 / 2 and I + W / 2: it is off by theta^2 / 2 in R and theta |upsilon| / 2 in t by construction, and the
    restatement keeps that."""
    u = np.array(u, np.float64)
    q, t = vba_ref.se3_exp(u)
    R, ts = _exp_series(u)
    theta, ups = np.linalg.norm(u[:3]), np.linalg.norm(u[3:])
    small = theta < 1e-5
    assert abs(np.linalg.norm(q) - 1) <= 1e-15 and q[3] >= 0
    assert np.abs(vba_ref.q_to_mat(q) - R).max() <= 1e-12 + (theta * theta if small else 0.0)
    assert np.abs(t - ts).max() <= 1e-12 + (theta * ups if small else 0.0)


def test_product_and_map_agree_with_matrices():
    rng = np.random.default_rng(0)
    a, b = vba_ref.se3_exp(rng.normal(0, 1, 6)), vba_ref.se3_exp(rng.normal(0, 1, 6))
    X = rng.normal(0, 3, 3)
    ab = vba_ref.se3_mul(a, b)
    assert np.abs(vba_ref.se3_map(ab, X) - vba_ref.se3_map(a, vba_ref.se3_map(b, X))).max() <= 1e-13
    assert np.abs(vba_ref.q_to_mat(ab[0]) - vba_ref.q_to_mat(a[0]) @ vba_ref.q_to_mat(b[0])).max() <= 1e-14


@pytest.mark.parametrize("name", ["small", "pin", "mixed"])
def test_analytic_jacobians_against_central_differences(oracle, name):
    """All five edges (camera 0, the three ToBody edges, the stereo edge), both camera models, on the smooth (all-double)
    projections.  Central differences with delta 1e-6 carry about eps |proj| / delta = 1e-7 px of rounding noise and a
    delta^2 truncation term: 1e-7 of max(1, the Jacobian's largest entry), the bar of the other reference tests."""
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    st = vba_ref.start_of(prob)
    _, _, depth = vba_ref.errors(G, st, "smooth")
    ok = depth > 0.3   # the planted edges behind their camera sit past the projection's smooth range
    assert set(np.unique(G.cam_of[ok])) == set(range(G.C)) and (name == "small" or G.ES > 50)
    Ja = vba_ref.jacobians(G, st, "analytic", "smooth")
    Jn = vba_ref.jacobians(G, st, "numeric", "smooth")
    for a, n in zip(Ja, Jn):
        tol = 1e-7 * max(1.0, float(np.abs(a[ok]).max()))
        assert np.abs(a[ok] - n[ok]).max() <= tol, (np.abs(a[ok] - n[ok]).max(), tol)


def test_planted_problem_returns_to_the_planted_state(oracle):
    """Noise-free observations, disturbed poses and points, 5 fixed keyframes: LM run until it stops ends at the truth."""
    prob = synth_vba.make_vba_problem(n_kf=10, n_opt=5, n_pts=150, seed=9, obs_noise=0.0, n_fixed_only=0, n_edgeless=3)
    G = vba_ref.Graph(prob)
    st0 = vba_ref.start_of(prob)
    res, st = vba_ref.optimize(G, st0, 100, 0.0, hub=(0.0, 0.0))
    assert res["iterations"] < 100 and res["err_end"] <= 1e-6 * max(res["err"], 1.0), res["err_end"]
    tr = prob["truth"]
    n = len(tr["pts"]) - 3
    assert np.abs(st0["t"][:5] - tr["t_cw"][:5]).max() > 1e-3      # it was disturbed
    assert np.abs(st["t"] - tr["t_cw"]).max() <= 1e-5
    assert np.abs(np.abs((st["q"] * tr["q_cw"]).sum(1)) - 1).max() <= 1e-10
    assert np.abs(st["pts"][:n] - tr["pts"][:n]).max() <= 1e-3
    assert np.array_equal(st["pts"][n:], st0["pts"][n:])           # the points without edges stay


def test_masked_edges_and_edgeless_points(oracle):
    """An excluded edge adds nothing to chi2 or the system; a point whose edges are all excluded, or that has none, is no
    active vertex and does not move; the excluded edge's chi2 is still reported at the final state."""
    prob = vba_cases.problem("small")
    G = vba_ref.Graph(prob)
    st0 = vba_ref.start_of(prob)
    victim = int(G.pt[G.kf < G.n_opt][0])
    lv = (G.pt[:G.EM] == victim).astype(np.uint8)
    lv[::7] = 1
    G.set_levels(lv)
    e, chi2, _ = vba_ref.errors(G, st0)
    hub = (vba_ref.HUBER_MONO, vba_ref.HUBER_STEREO)
    chi, _ = vba_ref.robust_chi2(G, chi2, hub)
    full = vba_ref.huber(chi2, hub[0])[0]
    assert abs(chi - full[lv == 0].sum()) <= 1e-9 * chi
    sys_ = vba_ref.build_system(G, st0, e, chi2, hub)
    assert not sys_["active_pt"][victim] and not sys_["Hll"][victim].any() and not sys_["bl"][victim].any()
    edgeless = np.setdiff1d(np.arange(G.P), G.pt)
    assert len(edgeless) >= 3 and not sys_["active_pt"][edgeless].any()
    res, st = vba_ref.optimize(G, st0, 3, 100.0)
    still = np.concatenate([[victim], edgeless])
    assert np.array_equal(st["pts"][still], st0["pts"][still])
    assert np.abs(st["pts"] - st0["pts"]).max() > 1e-4
    _, chi2_end, _ = vba_ref.errors(G, st)
    assert (res["chi2"][lv == 1] > 0).all() and res["chi2"].shape == chi2_end.shape


def test_lambda_init_is_the_largest_diagonal(oracle):
    """1e-5 max |H(j,j)| over poses and landmarks: once with a pose holding the maximum, once with a landmark."""
    prob = vba_cases.problem("small")
    hub = (vba_ref.HUBER_MONO, vba_ref.HUBER_STEREO)
    for boost in (False, True):
        p = dict(prob)
        if boost:   # one landmark next to a fixed camera with heavy observations: its Hll diagonal beats every pose's
            w = np.array(p["mono_inv_sigma2"], np.float32)
            w[np.asarray(p["mono_pt"]) == 0] = 1e7
            p["mono_inv_sigma2"] = w
        G = vba_ref.Graph(p)
        st = vba_ref.start_of(p)
        e, chi2, _ = vba_ref.errors(G, st)
        sys_ = vba_ref.build_system(G, st, e, chi2, hub)
        dp = np.abs(np.einsum("kii->ki", sys_["Hpp"])).max()
        dl = np.abs(np.einsum("pii->pi", sys_["Hll"])).max()
        assert (dl > dp) == boost, (dl, dp)
        assert vba_ref.lambda_init(sys_) == 1e-5 * max(dp, dl)
        res, _ = vba_ref.optimize(G, st, 1, 0.0)
        assert res["lambda_init"] == 1e-5 * max(dp, dl)


@pytest.mark.parametrize("name", list(vba_cases.CASES))
def test_cases_meet_the_parity_tests_conditions(oracle, name):
    """What tests/test_vba_gpu.py relies on, on the reference alone: no LM decision is marginal (every |rho| above 1e-6,
    the stop rule's two sides more than 1e-6 relative apart), at most 1 % of the edges lie within the chi2 tolerance of
    their outlier threshold, and no depth-planted edge does."""
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    runs = [vba_cases.reference(name, lam)[0] for lam in vba_cases.LAMBDAS]
    if name in ("small", "mixed"):
        runs += list(vba_cases.reference_two_rounds(name)[:2])
    for r in runs:
        assert min(abs(x) for x in r["rhos"]) > 1e-6, r["rhos"]
        for a, b in r["stops"]:
            assert abs(a - b) > 1e-6 * max(abs(a), abs(b)), (a, b)
        near = vba_cases.band(G, r["chi2"])
        assert near.sum() <= 0.01 * G.E, (int(near.sum()), G.E)
        assert not near[prob["behind"]].any()
    if name == "mixed":
        r = runs[0]
        b = prob["behind"]
        assert len(b) >= 3 and (r["depth"][b] < -0.05).all()
        assert (r["chi2"][b] < vba_ref.CHI2_MONO).all() and r["outlier"][b].all()   # under the threshold: flagged by depth alone
        assert r["outlier"].sum() > 0.03 * G.E                                             # the gross outliers too
    if name == "wide":
        opt = np.zeros((G.P, G.n_opt), bool)
        m = G.kf < G.n_opt
        opt[G.pt[m], G.kf[m]] = True
        seen = opt.sum(1)
        assert (seen[10:600] >= 34).all() and seen.max() > 32
