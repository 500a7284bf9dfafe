"""GPU parity of the device FullInertialBA (omv_fiba, openmavis_amd/csrc/lba.hip) against the float64 reference
(tests/fiba_ref.py), on the cases of tests/fiba_cases.py.

Bars (those of tests/test_lba_gpu.py):
  residuals      |gpu - ref| <= 1e-9; Jacobians 1e-9 relative
  reduced system packed S, rhs and x of one solve at lambda = 1: 1e-9 of the largest entry, the shared block included
  LM outcome     identical iteration / trial counts; err, err_end within 1e-5 relative
  final state    poses / velocities / biases within 1e-5 of the reference's own step (floor 1e-3); points in their
                 information metric <= 1e-3 -- in plain coordinates with a fixed keyframe, in gauge-invariant quantities
                 (fiba_ref.gauge_invariant) without one
  the shared pair every bImu keyframe holds the same bias, bit for bit
  determinism    two runs agree bit for bit; a handle reused for a problem of another size gives a fresh handle's bits
"""
import numpy as np
import pytest

import fiba_cases
import fiba_ref
from openmavis_amd.optimizer import FullInertialBA

pytestmark = pytest.mark.gpu


def _solver(prob):
    return FullInertialBA(max_kf=prob["n_kf"], max_cams=prob["n_cams"], max_pts=len(prob["pts"]),
                          max_edges=len(prob["mono_pt"]) + int(prob.get("n_stereo", 0)),
                          max_imu=max(1, len(prob["imu_kf1"])))


_REF = {}


def _reference(name, oracle):
    """The reference's solution of a case, computed once for the module."""
    if name not in _REF:
        _REF[name] = fiba_cases.reference(name, oracle)
    return _REF[name]


# ---- evaluate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eval_shared", "eval_per_kf"])
def test_evaluate(name, oracle):
    prob = fiba_cases.problem(name)
    assert prob["n_kf"] == 6 and prob["n_cams"] == 5 and len(prob["pts"]) == 150
    G = fiba_ref.Graph(prob)
    st = fiba_ref.start_of(prob)
    r = fiba_ref.evaluate(G, st, oracle)
    g = _solver(prob).set_problem(prob).evaluate()
    assert G.m_in.all()
    assert np.abs(g["mono_err"] - r["mono_err"]).max() <= 1e-9
    assert np.abs(g["imu_err"] - r["imu_err"]).max() <= 1e-9
    for k in ("mono_jx", "mono_jp"):
        d = np.abs(g[k].reshape(r[k].shape) - r[k]).max()
        assert d <= 1e-9 * np.abs(r[k]).max(), (k, d)
    bg, ba = fiba_ref.shared_value(G, st)
    want = np.concatenate([0.0 - bg, 0.0 - ba]) if G.shared else np.zeros(6)
    assert np.array_equal(g["prior_err"], want)


# ---- one reduced-system solve -------------------------------------------------------------------------------------------
def _check_debug_solve(prob, oracle, mode):
    G = fiba_ref.Graph(prob)
    st = fiba_ref.start_of(prob)
    ev = fiba_ref.evaluate(G, st, oracle)
    H, b = fiba_ref.build_system(G, st, ev, fiba_ref.chi2_of(G, st, ev))
    S, rhs, ip, _ = fiba_ref.reduce_system(G, H, b, 1.0)
    S16, r16, at = fiba_ref.device_layout(G, S, rhs, ip, 1.0)
    d = _solver(prob).set_problem(prob).debug_solve(1.0)
    assert d["fail"] == 0 and d["mode"] == mode, (d["fail"], d["mode"], d["n_slots"], d["n_lds"])
    assert d["S"].shape == S16.shape
    big = np.abs(S16).max()
    assert np.abs(d["S"] - S16).max() <= 1e-9 * big, np.abs(d["S"] - S16).max() / big
    assert np.abs(d["rhs"] - r16).max() <= 1e-9 * np.abs(r16).max()
    if G.shared:
        x = np.linalg.solve(S16, r16)
        assert np.abs(d["x"] - x).max() <= 1e-9 * np.abs(x).max(), np.abs(d["x"] - x).max() / np.abs(x).max()
    else:
        # The per-keyframe form's random-walk informations (1e12 and more beside lambda = 1) put the system's condition
        # where numpy's own solution is 1e-6 from the exact one: x against the refined solution of the returned system,
        # at the conditioning-aware bound of tests/test_linalg_gpu.py (the solver's existing path, its existing bar).
        import linalg_ref as ref
        core = at
        Sc, bc = d["S"][np.ix_(core, core)], d["rhs"][core]
        terms, _ = ref.refine_solve(Sc, bc)
        _, exact = ref.sum_terms(terms)
        kappa = ref.rayleigh_cond_lower_bound(Sc)
        e, e_ref = ref.forward_error(d["x"][core], exact), ref.forward_error(np.linalg.solve(Sc, bc), exact)
        print(f"per-keyframe form: forward error {e:.3e} (numpy {e_ref:.3e}), kappa >= {kappa:.3e}")
        assert e <= ref.solve_bound(len(core), kappa, e_ref), (e, e_ref, kappa)
    if G.shared:   # the shared block: rows 9..14 of block n_opt carry the pair, the rest of it is padding
        o = 16 * G.n_opt
        pad = [o + r for r in range(16) if not 9 <= r < 15]
        assert np.array_equal(d["x"][pad], np.zeros(len(pad))) and np.abs(d["x"][o + 9:o + 15]).min() > 0
        assert np.abs(d["S"][o + 9:o + 15, :o]).max() > 0   # the border


@pytest.mark.parametrize("name", ["eval_shared", "eval_per_kf"])
def test_debug_solve_all_blocks_in_lds(name, oracle):
    _check_debug_solve(fiba_cases.problem(name), oracle, mode=1)


def test_debug_solve_hybrid_storage(oracle):
    """K = 20, every landmark seen by every keyframe: 231 blocks do not fit the solver's LDS (use_lds == 2)."""
    prob = fiba_cases.problem("dense20")
    seen = np.zeros((len(prob["pts"]), prob["n_kf"]), bool)
    seen[prob["mono_pt"], prob["mono_kf"]] = True
    assert seen.mean() > 0.95
    _check_debug_solve(prob, oracle, mode=2)


# ---- optimize ------------------------------------------------------------------------------------------------------------
def _points_in_reference_frame(prob, sg, sr):
    """The device's points where the reference's gauge puts them (the identity with a fixed keyframe)."""
    if not fiba_cases.free_gauge(prob):
        return sg["pts"]
    body = fiba_ref.gauge_invariant(sg)["pts"]
    return body @ sr["Rwb"][0].T + sr["twb"][0]


def _points_maha(prob, G, sg, sr, oracle):
    """The points' differences in the landmark's information metric at the reference's final state (test_lba_gpu.py)."""
    d = _points_in_reference_frame(prob, sg, sr) - sr["pts"]
    ev = fiba_ref.evaluate(G, sr, oracle)
    Hl = np.zeros((G.P, 3, 3))
    np.add.at(Hl, G.m_pt[G.m_in], G.m_w[G.m_in, None, None] * np.einsum("eri,erj->eij", ev["mono_jx"][G.m_in], ev["mono_jx"][G.m_in]))
    np.add.at(Hl, G.s_pt[G.s_in], G.s_w[G.s_in, None, None] * np.einsum("eri,erj->eij", ev["stereo_jx"][G.s_in], ev["stereo_jx"][G.s_in]))
    return d, np.sqrt(np.maximum(np.einsum("pi,pij,pj->p", d, Hl, d), 0))


def _compare(name, prob, G, rg, sg, rr, sr, oracle):
    assert (rg["iterations"], rg["trials"]) == (rr["iterations"], rr["trials"]), (rg["iterations"], rg["trials"], rr)
    for k in ("err", "err_end"):
        assert abs(rg[k] - rr[k]) <= 1e-5 * abs(rr[k]), (k, rg[k], rr[k])
    sg = {k: np.asarray(v, np.float64) for k, v in sg.items()}
    sg["Rwb"] = sg["Rwb"].reshape(-1, 3, 3)
    vg, vr, v0 = fiba_cases.views(prob, sg), fiba_cases.views(prob, sr), fiba_cases.views(prob, fiba_ref.start_of(prob))
    for k in vr:
        step = np.abs(vr[k] - v0[k]).max()
        bar = 1e-5 * max(step, 1e-3)
        err = np.abs(vg[k] - vr[k]).max()
        print(f"{name} {k}: |gpu - ref| {err:.3e} step {step:.3e} bar {bar:.3e}")
        assert err <= bar, (k, err, step, bar)
    d, maha = _points_maha(prob, G, sg, sr, oracle)
    print(f"{name} pts: maha {maha.max():.3e} plain {np.abs(d).max():.3e} bar 1e-3")
    assert maha.max() <= 1e-3, (maha.max(), int(np.argmax(maha)))
    assert np.array_equal(sg["pts"][~G.pt_vertex], np.asarray(prob["pts"], np.float64)[~G.pt_vertex])
    tol = 1e-6 * rr["mono_chi2"] + 2e-3 * np.sqrt(rr["mono_chi2"]) + 1e-6   # test_lba_gpu.py's _chi2_tol
    bad = np.abs(rg["mono_chi2"] - rr["mono_chi2"]) > tol
    assert not bad.any(), (int(bad.sum()), rg["mono_chi2"][bad][:5], rr["mono_chi2"][bad][:5])


def _shared_pair_is_everywhere(prob, sg):
    imu = np.asarray(prob["kf_imu"], bool)
    for k in ("bg", "ba"):
        v = np.asarray(sg[k]).view(np.uint64)
        assert (v[imu] == v[imu][0]).all(), k
        assert np.array_equal(np.asarray(sg[k])[~imu], np.asarray(prob[k], np.float64)[~imu])


@pytest.mark.parametrize("name", fiba_cases.OPTIMIZE)
def test_optimize(name, oracle):
    """opt_shared: K = 12, 300 points, priors 1e2 / 1e5, 15 iterations, no fixed keyframe.  opt_per_kf_fix: per-keyframe
    biases with bFixLocal.  The ragged cases (K = 10): a first keyframe that is not bImu, a broken mPrevKF chain, a Pinhole
    rig with stereo edges, 5 points seen by the fixed keyframe only.  wide (K = 40): 20 landmarks seen by more than 32
    keyframes, the one-landmark build path."""
    prob, G, rr, sr = _reference(name, oracle)
    ba = _solver(prob).set_problem(prob)
    rg, sg = ba.optimize(iterations=fiba_cases.iterations_of(name), lambda_init=1e-5, max_trials=10)
    _compare(name, prob, G, rg, sg, rr, sr, oracle)
    if prob["shared_bias"]:
        _shared_pair_is_everywhere(prob, sg)
    if name == "fixed_only_pts":
        assert (~G.pt_vertex).sum() == 5
        assert np.array_equal(sg["pts"][:5], np.asarray(prob["pts"], np.float64)[:5])
        assert (rg["mono_chi2"][~G.m_in] == 0).all() and (~G.m_in).sum() >= 5
    if name == "wide":
        n_kfs = np.array([len(set(G.m_kf[(G.m_pt == p) & (G.m_kf < G.n_opt)].tolist())) for p in range(20)])
        # each past kGrpW = 32 optimisable keyframes: a group of its own on build_big_kernel (test_fiba_plan_cpu.py)
        assert (n_kfs > 32).sum() == 20, n_kfs
    if name == "pinhole_stereo":
        assert prob["n_stereo"] > 100


def test_optimum_of_the_kb8_free_gauge_case(oracle):
    """KannalaBrandt8 cameras and no fixed keyframe, the configuration of InitializeIMU's own call: the late LM decisions
    differ between correct solvers there (fiba_cases), so the optimum is compared, not the path -- err_end and the
    gauge-invariant state, at the larger of test_lba_gpu.py's bar and ten times the reference's own spread."""
    name = "opt_shared_kb8"
    prob, G, rr, sr = _reference(name, oracle)
    assert fiba_cases.free_gauge(prob) and "cam_model" not in prob
    spread, pts_spread, end_spread = fiba_cases.spread_of(name, oracle, sr, rr["err_end"],
                                                          lambda st: _points_maha(prob, G, st, sr, oracle)[1].max())
    rg, sg = _solver(prob).set_problem(prob).optimize(iterations=fiba_cases.iterations_of(name))
    assert abs(rg["err"] - rr["err"]) <= 1e-5 * rr["err"]
    bar = max(1e-5 * rr["err_end"], 10 * end_spread)
    print(f"{name} err_end: |gpu - ref| {abs(rg['err_end'] - rr['err_end']):.3e} spread {end_spread:.3e} bar {bar:.3e}")
    assert abs(rg["err_end"] - rr["err_end"]) <= bar, (rg["err_end"], rr["err_end"], end_spread)
    sg = {k: np.asarray(v, np.float64) for k, v in sg.items()}
    sg["Rwb"] = sg["Rwb"].reshape(-1, 3, 3)
    vg, vr, v0 = fiba_cases.views(prob, sg), fiba_cases.views(prob, sr), fiba_cases.views(prob, fiba_ref.start_of(prob))
    for k in vr:
        step = np.abs(vr[k] - v0[k]).max()
        bar = max(1e-5 * max(step, 1e-3), 10 * spread[k])
        err = np.abs(vg[k] - vr[k]).max()
        print(f"{name} {k}: |gpu - ref| {err:.3e} step {step:.3e} spread {spread[k]:.3e} bar {bar:.3e}")
        assert err <= bar, (k, err, step, spread[k])
    # (a point whose depth the views do not fix sits tens of metres apart in two runs of the reference itself: the
    # information metric is the comparison, as everywhere)
    _, maha = _points_maha(prob, G, sg, sr, oracle)
    bar = max(1e-3, 10 * pts_spread)
    print(f"{name} pts: maha {maha.max():.3e} spread {pts_spread:.3e} bar {bar:.3e}")
    assert maha.max() <= bar, (maha.max(), pts_spread)
    _shared_pair_is_everywhere(prob, sg)


def test_more_inertial_edges_than_the_lead_block_has_threads(oracle):
    """K = 260: 259 inertial edges, past the 256 that err_kernel's lead block takes one per thread; imu_err_rest_kernel
    takes the others.  Every edge's residual, the initial chi2 (all Huber terms and the priors) and -- what the build reads
    the residuals for -- the pair's diagonal block and gradient, which sum over every edge, against the reference; then
    three LM iterations through the captured step, bit for bit twice."""
    prob = fiba_cases.problem("many_edges")
    G = fiba_ref.Graph(prob)
    assert G.NI == 259
    st = fiba_ref.start_of(prob)
    ev = fiba_ref.evaluate(G, st, oracle)
    ch = fiba_ref.chi2_of(G, st, ev)
    ba = _solver(prob).set_problem(prob)
    g = ba.evaluate()
    assert np.abs(ev["imu_err"][256:]).max(axis=1).min() > 1e-6
    assert np.abs(g["imu_err"] - ev["imu_err"]).max() <= 1e-9
    r, _ = ba.optimize(iterations=0)
    assert abs(r["err"] - ch["total"]) <= 1e-9 * ch["total"], (r["err"], ch["total"])
    assert ch["imu"][1][256:].sum() > 1e-6 * ch["total"]   # the edges past the lead block count
    d = ba.reset().debug_solve(1.0)
    assert d["fail"] == 0
    o = 16 * G.n_opt + 9
    bg, bacc = fiba_ref.shared_value(G, st)
    Hs = np.diag([G.prior_g] * 3 + [G.prior_a] * 3) + np.eye(6)   # the priors and lambda = 1
    bs = np.concatenate([G.prior_g * (0.0 - bg), G.prior_a * (0.0 - bacc)])
    for i in range(G.NI):
        J, W, r1 = ev["imu_jac"][i][:, 9:15], G.info9[i], ch["imu"][2][i]
        Hs += r1 * (J.T @ W @ J)
        bs -= r1 * (J.T @ (W @ ev["imu_err"][i]))
    assert np.abs(d["S"][o:o + 6, o:o + 6] - Hs).max() <= 1e-9 * np.abs(Hs).max()
    assert np.abs(d["rhs"][o:o + 6] - bs).max() <= 1e-9 * np.abs(bs).max()
    r2, s2 = ba.reset().optimize(iterations=3)
    assert r2["err_end"] < 0.1 * r2["err"] and np.isfinite(r2["err_end"])
    _shared_pair_is_everywhere(prob, s2)
    # the trial's chi2 went through the same sum: the last computed errors at the final state, by the reference
    sf = {k: np.asarray(v, np.float64) for k, v in s2.items()}
    sf["Rwb"], sf["Rcw"], sf["tcw"] = sf["Rwb"].reshape(-1, 3, 3), sf["Rcw"].reshape(G.K, -1, 3, 3), sf["tcw"].reshape(G.K, -1, 3)
    ch_end = fiba_ref.chi2_of(G, sf, fiba_ref.evaluate(G, sf, oracle))
    if r2["trials"] == r2["iterations"]:   # (no rejected trial: the last errors are the final state's)
        assert abs(r2["err_end"] - ch_end["total"]) <= 1e-9 * ch_end["total"], (r2["err_end"], ch_end["total"])
    r3, s3 = ba.reset().optimize(iterations=3)
    assert r3["err_end"] == r2["err_end"] and np.array_equal(s3["twb"].view(np.uint64), s2["twb"].view(np.uint64))


def test_bitwise_identical_and_handle_reuse():
    """Two runs of one case agree bit for bit; a second set_problem of another size on the same handle gives what a
    fresh handle gives."""
    a, b = fiba_cases.problem("opt_shared"), fiba_cases.problem("no_imu_first")
    big = _solver(a)
    r1, s1 = big.set_problem(a).optimize(iterations=6)
    r2, s2 = big.set_problem(a).optimize(iterations=6)
    r3, s3 = big.set_problem(b).optimize(iterations=6)
    r4, s4 = _solver(b).set_problem(b).optimize(iterations=6)
    for (ra, sa), (rb, sb) in (((r1, s1), (r2, s2)), ((r3, s3), (r4, s4))):
        for k in ("err", "err_end", "lambda_", "iterations", "trials"):
            assert ra[k] == rb[k], (k, ra[k], rb[k])
        assert np.array_equal(ra["mono_chi2"].view(np.uint64), rb["mono_chi2"].view(np.uint64))
        for k in fiba_ref.STATE:
            assert np.array_equal(np.asarray(sa[k]).view(np.uint64), np.asarray(sb[k]).view(np.uint64)), k


def test_reset_and_timing_mode():
    """reset() restores the uploaded state; the per-stage timing mode (direct launches) makes the same decisions."""
    prob = fiba_cases.problem("no_imu_first")
    ba = _solver(prob).set_problem(prob)
    r1, s1 = ba.optimize(iterations=5)
    r2, s2 = ba.reset().enable_timing(True).optimize(iterations=5)
    assert (r1["iterations"], r1["trials"]) == (r2["iterations"], r2["trials"])
    assert abs(r1["err_end"] - r2["err_end"]) <= 1e-9 * abs(r1["err_end"])
    t = ba.stage_ms()
    assert t["trials"] == r2["trials"] and t["solve"] > 0


def test_rejected_before_any_launch():
    from openmavis_amd import _lib
    prob = fiba_cases.problem("eval_shared")
    with pytest.raises(_lib.OmvError):   # n_kf > max_kf
        FullInertialBA(max_kf=5, max_cams=5, max_pts=150, max_edges=2000, max_imu=8).set_problem(prob)
    with pytest.raises(_lib.OmvError):
        _solver(prob).set_problem(dict(prob, prior_a=-1.0))
    with pytest.raises(_lib.OmvError):   # no bImu keyframe
        _solver(prob).set_problem(dict(prob, kf_imu=np.zeros(6, np.uint8)))
    with pytest.raises(_lib.OmvError):
        _solver(prob).optimize()
