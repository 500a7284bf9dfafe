"""GPU parity of the visual bundle adjustment (LocalBundleAdjustment on the visual kind of openmavis_amd/csrc/lba.hip)
against the numpy reference tests/vba_ref.py, on the windows of tests/vba_cases.py.

Bar (tests/test_lba_gpu.py's, restated):
  residuals            within 1e-9 px
  JXi, JXj             within 1e-9 of their largest entry
  first system         H blocks, b and the first trial's x within 1e-9 of their largest entry (debug_solve)
  computeLambdaInit    within 1e-9 relative
  LM outcome           iterations and trials identical; err, err_end within 1e-5 relative
  keyframes            q as a rotation matrix and t within 1e-5 of the reference's own step (floor 1e-3)
  points               in their information metric <= 1e-3; 99 % within 1e-3 of their step and all within 1e-2
  per-edge chi2        within vba_cases.chi2_tol
  flags                identical except edges whose chi2 lies within that tolerance of its threshold
tests/test_vba_ref_cpu.py asserts on the reference alone that no LM decision of these windows is marginal and that at
most 1 % of the edges (and no depth-planted one) sit that close to a threshold.
"""
import numpy as np
import pytest

import vba_cases
import vba_ref
from openmavis_amd import _lib
from openmavis_amd.optimizer import LocalBundleAdjustment

pytestmark = pytest.mark.gpu

NAMES = list(vba_cases.CASES)


def _solver(prob, **over):
    kw = dict(max_kf=prob["n_kf"], max_cams=prob["n_cams"], max_pts=len(prob["pts"]),
              max_edges=len(prob["mono_pt"]) + len(prob["stereo_pt"]))
    kw.update(over)
    return LocalBundleAdjustment(**kw)


def _rot(q):
    return np.array([vba_ref.q_to_mat(x) for x in q])


def _compare_state(G, st0, sg, so, first_call=True, rel=1e-5):
    for a, b, init in ((_rot(sg["q_cw"]), _rot(so["q"]), _rot(st0["q"])), (sg["t_cw"], so["t"], st0["t"])):
        step, err = np.abs(b - init).max(), np.abs(a - b).max()
        assert err <= rel * max(step, 1e-3), (err, step)
    assert np.abs(sg["q_cw"][G.n_opt:] - st0["q"][G.n_opt:]).max() <= 1e-15     # the fixed keyframes stay
    assert np.array_equal(sg["t_cw"][G.n_opt:], st0["t"][G.n_opt:])
    # points in their own information metric (what the residuals see): sqrt(dX^T Hll dX), Hll = sum w JXi^T JXi over the
    # active edges at the reference's final state
    d = sg["pts"] - so["pts"]
    JXi, _ = vba_ref.jacobians(G, so)
    w = np.where(G.level == 0, G.w, 0.0)
    H = np.zeros((G.P, 3, 3))
    np.add.at(H, G.pt, w[:, None, None] * np.einsum("eri,erj->eij", JXi, JXi))
    maha = np.sqrt(np.maximum(np.einsum("pi,pij,pj->p", d, H, d), 0))
    assert maha.max() <= 1e-3, (maha.max(), int(np.argmax(maha)))
    step = np.abs(so["pts"] - st0["pts"]).max(axis=1)
    r = np.abs(d).max(axis=1) / np.maximum(step, 1e-2)
    assert np.quantile(r, 0.99) <= 1e-3 and r.max() <= 1e-2, (r.max(), np.quantile(r, [0.5, 0.9, 0.99]))
    if first_call:   # no active edge: not a vertex, does not move
        still = np.bincount(G.pt[G.level == 0], minlength=G.P) == 0
        assert still.any() and np.array_equal(sg["pts"][still], st0["pts"][still])


def _compare_result(G, rg, ro, behind=()):
    assert (rg["iterations"], rg["trials"]) == (ro["iterations"], ro["trials"]), (rg["iterations"], rg["trials"], ro["rhos"])
    for k in ("err", "err_end"):
        assert abs(rg[k] - ro[k]) <= 1e-5 * abs(ro[k]), (k, rg[k], ro[k])
    chi2 = np.concatenate([rg["mono_chi2"], rg["stereo_chi2"]])
    flags = np.concatenate([rg["mono_outlier"], rg["stereo_outlier"]])
    tol = vba_cases.chi2_tol(ro["chi2"])
    bad = np.abs(chi2 - ro["chi2"]) > tol
    assert not bad.any(), (int(bad.sum()), chi2[bad][:5], ro["chi2"][bad][:5])
    diff = flags != ro["outlier"]
    assert vba_cases.band(G, ro["chi2"])[diff].all(), (int(diff.sum()), ro["chi2"][diff][:5], ro["depth"][diff][:5])
    assert not diff[np.asarray(behind, np.int64)].any()


@pytest.mark.parametrize("name", NAMES)
def test_residuals_and_jacobians(oracle, name):
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    st = vba_ref.start_of(prob)
    g = _solver(prob).set_problem(prob).evaluate()
    e, _, _ = vba_ref.errors(G, st)
    JXi, JXj = vba_ref.jacobians(G, st)
    EM = G.EM
    print(name, "residual diff", np.abs(g["mono_err"] - e[:EM, :2]).max())
    assert np.abs(g["mono_err"] - e[:EM, :2]).max() <= 1e-9
    for key, J in (("mono_jxi", JXi[:EM, :2]), ("mono_jxj", JXj[:EM, :2])):
        print(name, key, np.abs(g[key] - J).max() / np.abs(J).max())
        assert np.abs(g[key] - J).max() <= 1e-9 * np.abs(J).max(), key
    if G.ES:
        assert np.abs(g["stereo_err"] - e[EM:]).max() <= 1e-9
        for key, J in (("stereo_jxi", JXi[EM:]), ("stereo_jxj", JXj[EM:])):
            assert np.abs(g[key] - J).max() <= 1e-9 * np.abs(J).max(), key


@pytest.mark.parametrize("name", NAMES)
def test_first_system(oracle, name):
    """buildSystem, the Schur complement and the first trial's solve at the reference's own lambda_0."""
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    st = vba_ref.start_of(prob)
    hub = (vba_ref.HUBER_MONO, vba_ref.HUBER_STEREO)
    e, chi2, _ = vba_ref.errors(G, st)
    sys_ = vba_ref.build_system(G, st, e, chi2, hub)
    lam = vba_ref.lambda_init(sys_)
    S, rhs, _, _ = vba_ref.reduce_system(sys_, lam)
    x = np.linalg.solve(S, rhs)
    g = _solver(prob).set_problem(prob).debug_solve(lam)
    assert g["fail"] == 0
    n = G.n_opt
    idx = (16 * np.arange(n)[:, None] + np.arange(6)[None]).reshape(-1)
    for what, a, b in (("S", g["S"][np.ix_(idx, idx)], S), ("rhs", g["rhs"][idx], rhs), ("x", g["x"][idx], x)):
        print(name, what, np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), what
    pad = np.setdiff1d(np.arange(16 * n), idx)
    assert not g["x"][pad].any()


@pytest.mark.parametrize("lam", vba_cases.LAMBDAS)
@pytest.mark.parametrize("name", NAMES)
def test_optimize(oracle, name, lam):
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    ro, so = vba_cases.reference(name, lam)
    rg, sg = _solver(prob).set_problem(prob).optimize(10, lambda_init=lam)
    print(name, lam, "lambda_init", rg["lambda_init"], ro["lambda_init"], "its/trials", rg["iterations"], rg["trials"],
          ro["iterations"], ro["trials"], "err_end", rg["err_end"], ro["err_end"])
    assert abs(rg["lambda_init"] - ro["lambda_init"]) <= 1e-9 * ro["lambda_init"]
    _compare_result(G, rg, ro, prob["behind"])
    _compare_state(G, vba_ref.start_of(prob), sg, so)


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_two_rounds_with_levels(oracle, name):
    """optimize(5), exclude the flagged edges and drop both robust kernels, optimize(10): the state stays on the device
    in between; counts and state as the reference run the same way; an excluded edge's chi2 is still reported."""
    prob = vba_cases.problem(name)
    G = vba_ref.Graph(prob)
    r1, r2, so = vba_cases.reference_two_rounds(name)
    ba = _solver(prob).set_problem(prob)
    g1, _ = ba.optimize(5)
    _compare_result(G, g1, r1, prob["behind"])
    flagged = np.concatenate([g1["mono_outlier"], g1["stereo_outlier"]])
    if not np.array_equal(flagged, r1["outlier"]):   # a band edge flipped: the reference's mask, so both runs solve one problem
        flagged = r1["outlier"]
    ba.set_levels(flagged[:G.EM], flagged[G.EM:])
    g2, sg = ba.optimize(10, huber_mono=0.0, huber_stereo=0.0)
    G.set_levels(r1["outlier"][:G.EM], r1["outlier"][G.EM:])
    assert G.level.sum() > (10 if name == "mixed" else -1)   # `small` has no outlier to exclude: the mask is empty there
    _compare_result(G, g2, r2)
    _compare_state(G, vba_ref.start_of(prob), sg, so, first_call=False)
    chi2 = np.concatenate([g2["mono_chi2"], g2["stereo_chi2"]])
    assert (chi2[G.level == 1] > 0).all()


def test_bitwise_repeatable_and_reset(oracle):
    """Fixed-order sums, no float atomics: two identical calls agree bit for bit, and reset + optimize reproduces the
    first run."""
    prob = vba_cases.problem("mixed")
    ba = _solver(prob).set_problem(prob)
    r0, s0 = ba.optimize(10)
    r1, s1 = _solver(prob).set_problem(prob).optimize(10)
    r2, s2 = ba.reset().optimize(10)
    for r, s in ((r1, s1), (r2, s2)):
        for k in ("err", "err_end", "lambda_", "lambda_init", "iterations", "trials"):
            assert r[k] == r0[k], (k, r[k], r0[k])
        for k in ("mono_chi2", "stereo_chi2"):
            assert np.array_equal(r[k].view(np.uint64), r0[k].view(np.uint64)), k
        for k in LocalBundleAdjustment.STATE:
            assert np.array_equal(s[k].view(np.uint64), s0[k].view(np.uint64)), k


def test_handle_rules(oracle):
    prob = vba_cases.problem("small")
    lib = _lib.load()
    ba = _solver(prob)
    for call in (ba.optimize, ba.evaluate, lambda: ba.debug_solve(1.0), ba.set_levels):   # no problem: no launch
        with pytest.raises(_lib.OmvError):
            call()
    import ctypes
    from openmavis_amd.synth_vba import as_vba_struct
    s, keep = as_vba_struct(prob, _lib.VbaProblem)
    o, r = _lib.VbaOpts(10, 0.0, 10, 2.0, 2.0), _lib.VbaResult()
    assert lib.omv_vba_optimize(ba._h, ctypes.byref(o), ctypes.byref(s), ctypes.byref(r)) == _lib.OMV_ERR_ARG
    assert lib.omv_vba_reset(ba._h) == _lib.OMV_ERR_ARG
    assert lib.omv_lba_set_comm(ba._h, 0, 1, None, None) == _lib.OMV_ERR_ARG      # single rank only
    ba.set_problem(prob)
    r0, s0 = ba.optimize(3, lambda_init=100.0)
    bad = dict(prob, mono_kf=np.where(np.arange(len(prob["mono_kf"])) == 5, prob["n_kf"], prob["mono_kf"]))
    big = dict(prob, pts=np.concatenate([prob["pts"], np.zeros((1, 3))]))
    for p, code in ((bad, "bad argument"), (big, "capacity")):
        with pytest.raises(_lib.OmvError, match=code):
            ba.set_problem(p)
    r1, s1 = ba.reset().optimize(3, lambda_init=100.0)   # the previous problem is still there
    assert r1["trials"] == r0["trials"] and np.array_equal(s1["pts"], s0["pts"])
    with pytest.raises(_lib.OmvError, match="capacity"):
        _solver(prob, max_edges=10).set_problem(prob)
    with pytest.raises(_lib.OmvError, match="capacity"):
        _solver(prob, max_kf=3).set_problem(prob)
    n0 = ctypes.c_int64(0)
    lib.omv_debug_live_allocations(ctypes.byref(n0))
    for _ in range(4):
        h = _solver(prob).set_problem(prob)
        h.optimize(1, lambda_init=100.0)
        del h
    n1 = ctypes.c_int64(0)
    lib.omv_debug_live_allocations(ctypes.byref(n1))
    assert n1.value == n0.value
