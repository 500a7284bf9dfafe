"""The device pose graphs (openmavis_amd.optimizer.EssentialGraph, openmavis_amd/csrc/essgraph.hip) against the float64
numpy restatement tests/essgraph_ref.py on the cases of tests/essgraph_cases.py.

Bars.  Errors and composed measurements: 1e-12 times the largest pose entry.  Jacobians: the device and the reference both
form g2o's central difference at delta = 1e-9, so they differ by the rounding of an error evaluation divided by 2e-9; the
bar is ten times the reference's own spread -- the largest distance of its g2o-form Jacobian from its near-exact one (delta
= 1e-6) -- measured from the near-exact Jacobian.  The first system carries the same spread, propagated through J^T Omega J
and J^T Omega e.  The LM takes the reference's iteration and trial counts; err within 1e-9 relative, err_end and the final
vertices within max(1e-9 relative, 10 x the distance between the reference's own two runs).  Measured figures: DESIGN 6."""
import ctypes

import numpy as np
import pytest

import essgraph_cases
import essgraph_ref as ref
from openmavis_amd import _lib
from openmavis_amd.optimizer import EssentialGraph, essgraph_struct

pytestmark = pytest.mark.gpu

NAMES = list(essgraph_cases.CASES)
KIND = {ref.SIM3: "sim3", ref.DOF4: "4dof"}
_cache = {}


def case(name):
    """The problem, the reference's two runs and its first system, computed once and left unchanged."""
    if name not in _cache:
        kind, prob = essgraph_cases.make(name)
        K = ref.make_kind(kind, prob)
        H, b, chi2, e, Ji, Jj = ref.build_system(K, K.state0)
        He, be, _, _, Jie, Jje = ref.build_system(K, K.state0, delta=1e-6)
        _cache[name] = dict(kind=kind, prob=prob, K=K, H=H, b=b, chi2=chi2, e=e, Ji=Ji, Jj=Jj, He=He, be=be, Jie=Jie, Jje=Jje,
                            run=ref.optimize(kind, prob), run_exact=ref.optimize(kind, prob, delta=1e-6))
    return _cache[name]


def graph(c, **kw):
    p = c["prob"]
    return EssentialGraph(KIND[c["kind"]], max_vertices=kw.get("max_vertices", len(p["vertices"])),
                          max_edges=kw.get("max_edges", len(p["edge_i"]))).set_problem(p)


def pose_scale(c):
    return max(1.0, float(np.abs(c["prob"]["vertices"]).max()), float(np.abs(c["prob"]["S_a"]).max()))


@pytest.mark.parametrize("name", NAMES)
def test_errors_measurements_and_jacobians(name):
    c = case(name)
    ev = graph(c).evaluate()
    tol = 1e-12 * pose_scale(c)
    print(f"{name}: |err - ref| {np.abs(ev['err'] - c['e']).max():.3g} |meas - ref| {np.abs(ev['meas'] - c['K'].meas).max():.3g} "
          f"(bar {tol:.3g})")
    assert np.abs(ev["meas"] - c["K"].meas).max() <= tol
    assert np.abs(ev["err"] - c["e"]).max() <= tol
    assert np.abs(ev["chi2"] - c["chi2"]).max() <= 1e-9 * max(1.0, c["chi2"].max())
    spread = max(np.abs(c["Ji"] - c["Jie"]).max(), np.abs(c["Jj"] - c["Jje"]).max())
    dist = max(np.abs(ev["jac_i"] - c["Jie"]).max(), np.abs(ev["jac_j"] - c["Jje"]).max())
    print(f"{name}: Jacobian spread of the reference {spread:.3g}, device distance {dist:.3g}")
    assert spread > 0 and dist <= 10 * spread
    fixed = c["K"].fixed
    assert not ev["jac_i"][fixed[c["K"].ei]].any() and not ev["jac_j"][fixed[c["K"].ej]].any()   # a fixed vertex: no block
    if c["prob"].get("fix_scale"):
        assert not ev["jac_i"][:, :, 6].any() and not ev["jac_j"][:, :, 6].any()   # exactly zero scale columns


@pytest.mark.parametrize("name", NAMES)
def test_first_system(name):
    c = case(name)
    d = graph(c).debug_solve(1.0)
    K = c["K"]
    _, _, _, real = ref.layout(K)
    n = len(real)
    assert d["S"].shape == (n, n) and d["fail"] == 0
    Href = c["He"] + np.diag(np.where(real, 1.0, 0.0))
    # the reference's own spread, as it reaches H and b: |H(1e-9) - H(1e-6)|, relative to the largest entry
    sH = np.abs(c["H"] - c["He"]).max() / np.abs(c["He"]).max()
    sb = np.abs(c["b"] - c["be"]).max() / np.abs(c["be"]).max()
    dH = np.abs(d["S"] - Href).max() / np.abs(c["He"]).max()
    db = np.abs(d["rhs"] - c["be"]).max() / np.abs(c["be"]).max()
    print(f"{name}: mode {d['mode']} slots {d['n_slots']} in LDS {d['n_lds']} levels {d['n_lev']}; H spread {sH:.3g} device {dH:.3g}; "
          f"b spread {sb:.3g} device {db:.3g}")
    assert dH <= 10 * sH and db <= 10 * sb
    # pad rows: exactly identity / zero, and nothing of them in a real row
    pad = np.flatnonzero(~real)
    for r in pad:
        row = d["S"][r].copy()
        assert row[r] == 1.0
        row[r] = 0.0
        assert not row.any() and not d["S"][:, r][np.arange(n) != r].any()
    assert not d["rhs"][pad].any() and not d["x"][pad].any()
    # x solves the returned system: against its refined solution, 1e-9 relative
    x0 = np.linalg.solve(d["S"], d["rhs"])
    x0 += np.linalg.solve(d["S"], d["rhs"] - d["S"] @ x0)
    assert np.abs(d["x"] - x0).max() <= 1e-9 * np.abs(x0).max()
    if c["prob"].get("fix_scale"):
        rows = np.flatnonzero(real).reshape(-1, 7)[:, 6]
        assert not d["x"][rows].any() and not d["rhs"][rows].any()
        assert all(d["S"][r, r] == 1.0 and np.count_nonzero(d["S"][r]) == 1 for r in rows)   # lambda alone
    want_mode = {"c_sim3": 2}.get(name, 1)
    assert d["mode"] == want_mode
    if name.startswith("b_"):
        assert d["n_lev"] >= 3 and d["n_slots"] > 2 * len(real) // 16 - 1   # fill and several levels


def test_fix_scale_rows_at_the_reference_lambda():
    """lambda_0 = 1e-16: the scale rows' diagonal is lambda alone, their step exactly 0, finite, and no failure flag."""
    c = case("a_sim3_fix_scale")
    d = graph(c).debug_solve(1e-16)
    _, _, _, real = ref.layout(c["K"])
    rows = np.flatnonzero(real).reshape(-1, 7)[:, 6]
    assert d["fail"] == 0 and np.isfinite(d["x"]).all()
    assert all(d["S"][r, r] == 1e-16 for r in rows) and not d["x"][rows].any()
    assert np.abs(d["x"]).max() > 0


@pytest.mark.parametrize("name", NAMES)
def test_levenberg_marquardt(name):
    c = case(name)
    a, b = c["run"], c["run_exact"]
    assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])   # test_essgraph_ref_cpu.py's condition
    g = graph(c)
    r = g.optimize(20, 10)
    own_v = np.abs(a["vertices"] - b["vertices"]).max()
    own_e = abs(a["err_end"] - b["err_end"])
    dv = np.abs(r["vertices"] - a["vertices"]).max()
    print(f"{name}: device {r['iterations']} it {r['trials']} tr err {r['err']:.12g} -> {r['err_end']:.12g} lambda {r['lambda_']:.3g}; "
          f"reference {a['iterations']} it {a['trials']} tr -> {a['err_end']:.12g} (near-exact {b['err_end']:.12g}); "
          f"|v - ref| {dv:.3g}, the reference's own two runs differ by {own_v:.3g} (err_end {own_e:.3g})")
    assert r["solver_failed"] == 0
    assert (r["iterations"], r["trials"]) == (a["iterations"], a["trials"])
    assert abs(r["err"] - a["err"]) <= 1e-9 * a["err"]
    assert abs(r["err_end"] - a["err_end"]) <= max(1e-9 * a["err_end"], 10 * own_e)
    assert dv <= max(1e-9 * np.abs(a["vertices"]).max(), 10 * own_v)
    assert r["err_end"] < r["err"]
    if name == "d_4dof":
        assert a["n_acc"] >= 6   # the normalisation fired in the reference, and the device followed it


@pytest.mark.parametrize("name,mode", [("a_sim3", "loop"), ("e_sim3_merge", "merge"), ("a_4dof", "4dof"), ("b_sim3", "loop")])
def test_recovery(name, mode):
    c = case(name)
    p = c["prob"]
    g = graph(c)
    r = g.optimize(20, 10)
    poses, pts = g.recover(mode, p["points"], p["point_ref"])
    # the numpy restatement from the device's own final state (the LM's distance is test_levenberg_marquardt's)
    K = c["K"]
    if c["kind"] == ref.SIM3:
        state = r["vertices"]
    else:
        v = r["vertices"]
        state = np.concatenate([np.zeros((len(v), 9)), v[:, 12:21], v[:, 21:24], v[:, 0:9], v[:, 9:12]], -1)
    want_poses, want_pts = ref.recover(c["kind"], p, state, mode, p["points"], p["point_ref"])

    def ulps(x, y):
        return np.abs(x.astype(np.float64) - y.astype(np.float64)) / np.spacing(np.maximum(np.abs(x), np.abs(y)).astype(np.float32))

    print(f"{name}: poses {ulps(poses, want_poses).max():.2f} ulp, points {ulps(pts, want_pts).max():.2f} ulp")
    assert ulps(poses, want_poses).max() <= 1.0
    assert ulps(pts, want_pts).max() <= 1.0
    untouched = np.asarray(p["point_ref"]) < 0
    assert untouched.any() and np.array_equal(pts[untouched], p["points"][untouched])
    assert not np.array_equal(pts[~untouched], p["points"][~untouched])
    assert np.abs(np.linalg.norm(poses[:, :4], axis=1) - 1).max() < 1e-6


def test_repeats_are_bitwise_identical():
    c = case("b_sim3")
    g = graph(c)
    r0, d0 = g.optimize(20, 10), None
    g.reset()
    d0 = g.debug_solve(1.0)
    r1 = g.optimize(20, 10)
    g2 = graph(c)
    d2 = g2.debug_solve(1.0)
    r2 = g2.optimize(20, 10)
    for r in (r1, r2):
        assert (r["iterations"], r["trials"], r["err"], r["err_end"], r["lambda_"]) == \
               (r0["iterations"], r0["trials"], r0["err"], r0["err_end"], r0["lambda_"])
        assert np.array_equal(r["vertices"], r0["vertices"])
    assert np.array_equal(d0["S"], d2["S"]) and np.array_equal(d0["x"], d2["x"]) and np.array_equal(d0["rhs"], d2["rhs"])


def test_handle_reuse_with_a_smaller_and_a_larger_problem():
    big, small = case("b_sim3"), case("a_sim3")
    g = EssentialGraph("sim3", max_vertices=64, max_edges=512)
    first = g.set_problem(big["prob"]).optimize(20, 10)
    s = g.set_problem(small["prob"]).optimize(20, 10)
    again = g.set_problem(big["prob"]).optimize(20, 10)
    fresh = graph(small).optimize(20, 10)
    assert np.array_equal(s["vertices"], fresh["vertices"]) and s["trials"] == fresh["trials"]
    assert np.array_equal(first["vertices"], again["vertices"]) and first["err_end"] == again["err_end"]


def _live():
    n = ctypes.c_int64(-1)
    _lib.check(_lib.load().omv_debug_live_allocations(ctypes.byref(n)), "omv_debug_live_allocations")
    return n.value


def test_rejected_problems_and_allocations():
    lib = _lib.load()
    c = case("a_sim3")
    p = c["prob"]
    g = graph(c)
    before = g.optimize(20, 10)
    live = _live()

    def status(**over):
        s, keep = essgraph_struct(dict(p, **over))
        return lib.omv_essgraph_set_problem(g._h, ctypes.byref(s))

    ej = p["edge_j"].copy()
    ej[1] = len(p["vertices"])
    assert status(edge_j=ej) == _lib.OMV_ERR_ARG                               # a vertex that is not there
    ej = p["edge_j"].copy()
    ej[2] = p["edge_i"][2]
    assert status(edge_j=ej) == _lib.OMV_ERR_ARG                               # i == j
    assert status(fixed=np.ones(len(p["vertices"]), np.uint8)) == _lib.OMV_ERR_ARG   # no optimisable vertex
    et = p["edge_table"].copy()
    et[0] = 2
    assert status(edge_table=et) == _lib.OMV_ERR_ARG
    bigger = essgraph_cases.make("b_sim3")[1]
    s, keep = essgraph_struct(bigger)
    assert lib.omv_essgraph_set_problem(g._h, ctypes.byref(s)) == _lib.OMV_ERR_ARG   # beyond the handle's capacities
    assert _live() == live
    # the previous problem is kept
    g.reset()
    after = g.optimize(20, 10)
    assert np.array_equal(after["vertices"], before["vertices"])
    # 4DoF without the rig, the wrong recover mode, set_comm
    g4 = EssentialGraph("4dof", 8, 16)
    p4 = dict(essgraph_cases.make("a_4dof")[1], Rcb=None, tcb=None)
    s, keep = essgraph_struct(p4)
    assert lib.omv_essgraph_set_problem(g4._h, ctypes.byref(s)) == _lib.OMV_ERR_ARG
    r = _lib.EssGraphResult()
    assert lib.omv_essgraph_optimize(g4._h, 20, 10, ctypes.byref(r)) == _lib.OMV_ERR_ARG   # no problem: before any launch
    assert lib.omv_essgraph_recover(g._h, _lib.ESSGRAPH_RECOVER_4DOF, None, 0, None, None) == _lib.OMV_ERR_ARG
    assert lib.omv_essgraph_set_comm(g._h, 0, 2, None, None) == _lib.OMV_ERR_ARG
    h = ctypes.c_void_p()
    assert lib.omv_essgraph_create(5, 8, 8, ctypes.byref(h)) == _lib.OMV_ERR_ARG
    assert lib.omv_essgraph_create(0, 0, 8, ctypes.byref(h)) == _lib.OMV_ERR_ARG
    # a failed create leaks nothing
    del g4
    live = _live()
    for nth in (1, 2):
        _lib.check(lib.omv_debug_fail_allocation(nth), "omv_debug_fail_allocation")
        assert lib.omv_essgraph_create(0, 8, 8, ctypes.byref(h)) == _lib.OMV_ERR_HIP
        assert _live() == live
    # a failed upload leaves no problem and leaks nothing
    g5 = EssentialGraph("sim3", 8, 16)
    live = _live()
    _lib.check(lib.omv_debug_fail_allocation(4), "omv_debug_fail_allocation")
    s, keep = essgraph_struct(p)
    assert lib.omv_essgraph_set_problem(g5._h, ctypes.byref(s)) == _lib.OMV_ERR_HIP
    assert _live() == live
    assert lib.omv_essgraph_optimize(g5._h, 20, 10, ctypes.byref(r)) == _lib.OMV_ERR_ARG
    _lib.check(lib.omv_debug_fail_allocation(0), "omv_debug_fail_allocation")
