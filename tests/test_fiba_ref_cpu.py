"""The float64 reference of FullInertialBA (tests/fiba_ref.py) anchored, on the CPU alone.

The committed oracle (oracle/ba_oracle.cpp) has no shared-bias mode, so the reference is tied to it on the ground they
share -- the edges, and the whole Levenberg loop with per-keyframe biases -- and the shared pair's own part (its Jacobian
columns, the two priors) is checked against central differences and planted problems.  Last, every case of
tests/fiba_cases.py that tests/test_fiba_gpu.py optimises is shown to have no marginal LM decision, on the reference alone.
"""
import numpy as np
import pytest

import fiba_cases
import fiba_ref
import inertial_ref
from openmavis_amd import synth_fiba


@pytest.fixture(scope="module")
def per_kf():
    return synth_fiba.make_fiba_problem(n_kf=8, n_pts=200, seed=3, fix_last=True, shared_bias=False, stereo_frac=0.3)


# ---- evaluate parity -----------------------------------------------------------------------------------------------------
def test_edges_equal_the_oracles(per_kf, oracle):
    """shared_bias == 0: the reference's EdgeInertial residuals and 9 x 24 Jacobians, and its EdgeMono / EdgeStereo residuals
    and Jacobians, are oracle.lba_evaluate's (1e-9 / 1e-9 relative)."""
    G = fiba_ref.Graph(per_kf)
    ev = fiba_ref.evaluate(G, fiba_ref.start_of(per_kf), oracle)
    o = oracle.lba_evaluate(per_kf)
    assert G.NI == 7 and len(G.s_pt) > 50
    assert np.abs(ev["imu_err"] - o["imu_err"]).max() <= 1e-9
    assert np.abs(ev["imu_jac"] - o["imu_jac"]).max() <= 1e-9 * np.abs(o["imu_jac"]).max()
    assert np.abs(ev["mono_err"] - o["mono_err"]).max() <= 1e-9
    for k, shape in (("mono_jx", (-1, 2, 3)), ("mono_jp", (-1, 2, 6)), ("stereo_jx", (-1, 3, 3)), ("stereo_jp", (-1, 3, 6))):
        assert np.abs(ev[k] - o[k].reshape(shape)).max() <= 1e-9 * np.abs(o[k]).max(), k


def test_shared_pair_reads_the_same_edges(oracle):
    """With the shared pair every bImu keyframe holds its value, so an edge's residual and its G1 / A1 columns are those of
    the per-keyframe problem at the same state: the graph only routes the columns to another vertex."""
    prob = fiba_cases.problem("eval_shared")
    G, Gk = fiba_ref.Graph(prob), fiba_ref.Graph(dict(prob, shared_bias=0))
    st = fiba_ref.start_of(prob)
    a, b = fiba_ref.evaluate(G, st, oracle), fiba_ref.evaluate(Gk, st, oracle)
    assert np.array_equal(a["imu_err"], b["imu_err"]) and np.array_equal(a["imu_jac"], b["imu_jac"])
    for i in range(G.NI):
        c, ck = G.imu_columns(i), Gk.imu_columns(i)
        assert np.array_equal(c[9:15], G.off_shared + np.arange(6)) and np.array_equal(ck[9:15], 15 * G.k1[i] + 9 + np.arange(6))
        assert np.array_equal(c[:9], ck[:9]) and np.array_equal(c[15:], ck[15:])


# ---- LM parity -------------------------------------------------------------------------------------------------------------
def test_lm_parity_with_the_oracle(per_kf, oracle):
    """shared_bias == 0, K = 8: fiba_ref.optimize and oracle.lba_optimize (large, every edge robust at scale 1, lambda_0 =
    1e-5) agree on the iteration and trial counts and on err / err_end to 1e-5 relative (tests/test_lba_gpu.py's bar)."""
    assert (np.asarray(per_kf["imu_robust"]) == 1).all() and (np.asarray(per_kf["imu_info_scale"]) == 1).all()
    ro, so, _ = oracle.lba_optimize(per_kf, opt_it=15, lambda_init=1e-5, max_trials=10, large=True)
    G = fiba_ref.Graph(per_kf)
    assert G.pt_vertex.all()   # (the oracle's graph keeps a point that only fixed keyframes see; none here)
    rr, sr = fiba_ref.optimize(G, fiba_ref.start_of(per_kf), oracle, iterations=15, lambda_init=1e-5, max_trials=10)
    assert (rr["iterations"], rr["trials"]) == (ro["iterations"], ro["trials"]), (rr["iterations"], rr["trials"], ro)
    for k in ("err", "err_end"):   # (the oracle reports floats, as the reference implementation does)
        assert abs(rr[k] - ro[k]) <= 1e-5 * abs(ro[k]), (k, rr[k], ro[k])
    for k in ("Rwb", "twb", "vel", "bg", "ba"):
        init = np.asarray(per_kf[k], np.float64).reshape(np.asarray(sr[k]).shape)
        step = np.abs(np.asarray(sr[k]) - init).max()
        assert np.abs(np.asarray(so[k]).reshape(init.shape) - sr[k]).max() <= 1e-5 * max(step, 1e-3), k


# ---- the shared pair's Jacobian columns ---------------------------------------------------------------------------------
def test_shared_columns_match_central_differences(oracle):
    """d (all inertial residuals, both prior errors) / d (the pair) from the graph's column routing against central
    differences of the residuals (every bImu keyframe's bias moved together): 1e-7 of max(1, largest entry)."""
    prob = fiba_cases.problem("eval_shared")
    G = fiba_ref.Graph(prob)
    st = fiba_ref.start_of(prob)
    ev_ = fiba_ref.evaluate(G, st, oracle)
    J = np.zeros((9 * G.NI + 6, 6))
    for i in range(G.NI):
        cols = G.imu_columns(i)
        sel = (cols >= G.off_shared) & (cols < G.off_shared + 6)
        assert sel.sum() == 6
        J[9 * i:9 * i + 9, cols[sel] - G.off_shared] = ev_["imu_jac"][i][:, sel]
    J[9 * G.NI:] = -np.eye(6)   # EdgePriorGyro / EdgePriorAcc: e = 0 - b

    # The oracle's residual takes the preintegrated deltas in float, as IMU::Preintegrated::GetDeltaRotation does: a step
    # function at 6e-8, which no difference quotient resolves.  EdgeInertial::computeError (G2oTypes.cc:581-598) is
    # restated here on tests/inertial_ref.py's smooth deltas (the same expressions in double), and shown to be the
    # oracle's residual up to that float step.
    pre = np.asarray(prob["preint"], np.float32).reshape(-1, 292)
    dt = pre[:, inertial_ref.DT].astype(np.float64)[:, None]
    g = np.array([0.0, 0.0, -inertial_ref.G])

    def residuals(d, kind="smooth"):
        bg, ba = fiba_ref.shared_value(G, st)
        bg, ba = bg + d[:3], ba + d[3:]
        dR, dV, dP, _ = inertial_ref.deltas(pre, bg, ba, kind)
        R1, R2 = st["Rwb"][G.k1], st["Rwb"][G.k2]
        er = inertial_ref.log_so3(np.einsum("eji,ekj,ekl->eil", dR, R1, R2))
        ev = np.einsum("eji,ej->ei", R1, st["vel"][G.k2] - st["vel"][G.k1] - g * dt) - dV
        ep = np.einsum("eji,ej->ei", R1, st["twb"][G.k2] - st["twb"][G.k1] - st["vel"][G.k1] * dt - g * dt * dt / 2) - dP
        return np.concatenate([np.concatenate([er, ev, ep], axis=1).reshape(-1), 0.0 - bg, 0.0 - ba])

    assert np.abs(residuals(np.zeros(6))[:9 * G.NI] - ev_["imu_err"].reshape(-1)).max() <= 1e-6
    num = np.zeros_like(J)
    for q in range(6):
        h = np.zeros(6)
        h[q] = 1e-5
        num[:, q] = (residuals(h) - residuals(-h)) / 2e-5
    assert np.abs(J).max() > 0.1
    assert np.abs(num - J).max() <= 1e-7 * max(1.0, np.abs(J).max()), np.abs(num - J).max()


# ---- the priors -------------------------------------------------------------------------------------------------------------
def test_prior_chi2(oracle):
    prob = fiba_cases.problem("eval_shared")
    G = fiba_ref.Graph(prob)
    st = fiba_ref.start_of(prob)
    ch = fiba_ref.chi2_of(G, st, fiba_ref.evaluate(G, st, oracle))
    bg, ba = np.asarray(prob["bg0"]), np.asarray(prob["ba0"])
    assert np.allclose(ch["prior"], [prob["prior_g"] * (bg @ bg), prob["prior_a"] * (ba @ ba)], rtol=1e-15, atol=0)
    zero = fiba_ref.chi2_of(fiba_ref.Graph(dict(prob, prior_g=0.0, prior_a=0.0)), st, fiba_ref.evaluate(G, st, oracle))
    assert ch["total"] - zero["total"] == pytest.approx(ch["prior"].sum(), rel=1e-9)


def test_planted_bias_is_recovered_and_a_stiff_prior_holds_it(oracle):
    """A noise-free planted problem (bFixLocal, exact observations, points and poses, weak priors): started from a
    disturbed pair the optimisation returns to the pair it reaches from the planted one -- the disturbance is undone to
    1e-3 of its size.  (The planted zero itself is not the optimum to that accuracy: the generator's preintegration is
    float32 at 400 Hz, and the planted state leaves the inertial edges a residual.)  And with prior_g = prior_a = 1e10 the
    pair does not move."""
    kw = dict(n_kf=8, n_pts=200, seed=13, fix_last=True, shared_bias=True, prior_g=1e-3, prior_a=1e-3, obs_noise=0.0,
              pt_noise=0.0, rot_noise_deg=0.0, trans_noise=0.0, bias_sigma=(0.0, 0.0))
    planted = synth_fiba.make_fiba_problem(**kw)
    assert not planted["bg0"].any() and not planted["ba0"].any()
    dg, da = np.array([2e-2, -1e-2, 1.5e-2]), np.array([2e-1, 1e-1, -3e-1])

    def run(prob):
        G = fiba_ref.Graph(prob)
        return fiba_ref.optimize(G, fiba_ref.start_of(prob), oracle, iterations=12)

    def disturbed(prob):
        k = np.asarray(prob["kf_imu"], bool)[:, None]
        return dict(prob, bg0=dg, ba0=da, bg=np.where(k, dg, 0.0), ba=np.where(k, da, 0.0))

    _, s0 = run(planted)
    r1, s1 = run(disturbed(planted))
    assert r1["err_end"] < 1e-3 * r1["err"]
    assert np.abs(s1["bg"][0] - s0["bg"][0]).max() <= 1e-3 * np.abs(dg).max()
    assert np.abs(s1["ba"][0] - s0["ba"][0]).max() <= 1e-3 * np.abs(da).max()
    # The priors' mean is zero.  On a noisy problem started at a zero pair the data move the pair under weak priors; under
    # prior_g = prior_a = 1e10 (against the data's 1e4 .. 1e7 of information on it) it stays: below 1e-2 of that move.
    noisy = synth_fiba.make_fiba_problem(**dict(kw, obs_noise=0.7, pt_noise=0.05, rot_noise_deg=0.5, trans_noise=0.02))
    _, sw = run(noisy)
    _, ss = run(dict(noisy, prior_g=1e10, prior_a=1e10))
    for k in ("bg", "ba"):
        assert np.abs(sw[k][0]).max() > 0 and np.abs(ss[k][0]).max() <= 1e-2 * np.abs(sw[k][0]).max(), (k, ss[k][0], sw[k][0])
        assert (ss[k] == ss[k][0]).all()   # every bImu keyframe holds the pair


# ---- no marginal decision in the cases the device is compared on ------------------------------------------------------
@pytest.mark.parametrize("name", fiba_cases.OPTIMIZE)
def test_no_marginal_decision(name, oracle):
    """On the reference alone: every |rho| above 1e-6, the stop rule's two sides more than 1e-6 relative apart -- and, as
    the chi2 is a step function at the 1e-5 level (the camera models project through float), the iteration and trial
    counts unchanged when the reduced system is eliminated in the reverse order and when the inputs move by one ulp.  A
    case that fails is reseeded in fiba_cases.py, not excused."""
    runs = [fiba_cases.reference(name, oracle, **kw) for kw in (dict(), dict(order="reverse"), dict(ulp=True))]
    r = runs[0][2]
    assert np.abs(r["rhos"]).min() > 1e-6, r["rhos"]
    for gain, ini in r["stops"]:
        assert abs(gain - ini) > 1e-6 * abs(ini), (gain, ini)
    counts = [(x[2]["iterations"], x[2]["trials"]) for x in runs]
    assert len(set(counts)) == 1, counts
    for x in runs[1:]:
        assert abs(x[2]["err_end"] - r["err_end"]) <= 1e-5 * r["err_end"]
