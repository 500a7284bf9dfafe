"""tests/inertial_ref.py on the CPU: the reference the device InertialOptimization is tested against, and the parts of
the feature that need no GPU (the exported symbols, the Python signatures, the adapter's compile)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import inertial_cases as cases
import inertial_ref as ref
from openmavis_amd import _lib, inertial_init as ii, synth_inertial as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, BIAS, GS = ii.FULL, ii.BIAS, ii.GS


# ---- Jacobians ---------------------------------------------------------------------------------------------------------
def _numeric_jacobian(P, st, delta=1e-6):
    """Central differences of the smooth error through the vertices' oplus: [E][9][3K + 9]."""
    N = 3 * P.K + 9
    J = np.zeros((P.E, 9, N))
    for q in range(N):
        x = np.zeros(N)
        x[q] = delta
        J[:, :, q] = (P.error(P.oplus(st, x)) - P.error(P.oplus(st, -x))) / (2 * delta)
    return J


@pytest.mark.parametrize("scale", [1.0, 1.3])
def test_analytic_jacobians_against_central_differences(oracle, scale):
    """All six free blocks of every edge.  Central differences with delta 1e-6 on the smooth float64 error carry about
    u |e| / delta = 1e-10 of rounding noise and delta^2 |e'''| = 1e-12 of truncation on entries up to ~10: the bar is
    1e-7 of max(1, the Jacobian's largest entry).  At scale 1 the analytic scale column is the derivative; at scale 1.3
    the derivative of s exp(u) carries a factor s the reference's Jacobian (G2oTypes.cc:741-745) does not have: the
    numeric column is exactly s times the analytic one."""
    worst = 0.0
    for seed in (3, 4):
        job = si.make_job(6, seed, FULL, True, 1e2, 1e5)
        job["scale"] = scale
        job["bg0"] = job["truth_bg"] * 0.5          # away from the records' bias: dbg != 0, the right Jacobian acts
        job["ba0"] = job["truth_ba"] * 0.5
        P = ref.Problem(job, "smooth")
        st = P.state0(job)
        e, Ja = P.error(st, True)
        Jn = _numeric_jacobian(P, st)
        idx = P.index()
        tol = 1e-7 * max(1.0, float(np.abs(Ja).max()))
        for ed in range(P.E):
            num = Jn[ed][:, idx[ed]]
            ana = Ja[ed].copy()
            ana[:, 14] *= scale
            worst = max(worst, float(np.abs(num - ana).max()))
            assert np.abs(num - ana).max() <= tol, (seed, ed, np.abs(num - ana).max())
            other = np.ones(3 * P.K + 9, bool)
            other[idx[ed]] = False
            assert np.abs(Jn[ed][:, other]).max() <= tol      # an edge touches nothing else
            if scale != 1.0:   # the quirk is visible: the analytic column itself is not the derivative
                assert np.abs(num[:, 14] - Ja[ed][:, 14]).max() > 0.1 * np.abs(Ja[ed][:, 14]).max()
    print(f"[inertial ref] scale {scale}: worst |numeric - analytic| {worst:.3g}")


# ---- planted problems (sanity, not accuracy bars) -------------------------------------------------------------------------
def _angle(Rwg, job):
    a, b = np.asarray(Rwg).reshape(3, 3) @ [0, 0, -1.0], job["truth_Rwg"] @ [0, 0, -1.0]
    return float(np.arccos(np.clip(a @ b, -1, 1)))


@pytest.mark.parametrize("mono", [False, True])
def test_planted_full_problem_improves(oracle, mono):
    job = si.make_job(24, 31 + mono, FULL, mono, 1e2, 1e5)
    r = ref.optimize(job)
    assert r["log"][-1]["chi2"] < r["first"]["chi2"]
    assert _angle(r["Rwg"], job) < _angle(job["Rwg"], job)
    assert np.linalg.norm(r["bg"] - job["truth_bg"]) < np.linalg.norm(job["bg0"] - job["truth_bg"])
    assert np.linalg.norm(r["ba"] - job["truth_ba"]) < np.linalg.norm(job["ba0"] - job["truth_ba"])
    if mono:
        assert job["truth_scale"] == 1.1 and abs(r["scale"] - 1.1) < abs(job["scale"] - 1.1)
    else:
        assert r["scale"] == job["scale"]


def test_planted_bias_and_gs_problems_improve(oracle):
    job = si.make_job(24, 41, BIAS, False, 1.0, 1e5)
    r = ref.optimize(job)
    assert r["log"][-1]["chi2"] < r["first"]["chi2"]
    assert np.linalg.norm(r["bg"] - job["truth_bg"]) < np.linalg.norm(job["bg0"] - job["truth_bg"])
    assert np.array_equal(r["Rwg"], np.asarray(job["Rwg"]).reshape(3, 3)) and r["scale"] == job["scale"]
    job = si.make_job(24, 42, GS, False, 0, 0)
    r = ref.optimize(job)
    assert r["iterations"] == 10 and _angle(r["Rwg"], job) < _angle(job["Rwg"], job)
    assert np.array_equal(r["vel"], job["vel"]) and np.array_equal(r["bg"], job["bg0"])
    assert not r["reintegrate"].any()


# ---- the tolerance precondition of the GPU outcome test ---------------------------------------------------------------------
def test_dense_and_structured_solves_take_the_same_decisions(oracle):
    """On every job the GPU outcome test uses (and the chain test's), the reference's dense and structured runs end at the
    same iteration with the same exit reason and agree within 1e-9 in every output; no keyframe's bias norm lies inside
    the band round 0.01, and both flag values occur."""
    worst, flags = 0.0, set()
    for name, jobs in (("main", cases.make()), ("chain", cases.chain_jobs())):
        n_band = n_kf = 0
        for i, job in enumerate(jobs):
            a, b = ref.optimize(job, "literal", "dense"), ref.optimize(job, "literal", "structured")
            assert (a["iterations"], a["exit"]) == (b["iterations"], b["exit"]), (name, i)
            assert [l["trials"] for l in a["log"]] == [l["trials"] for l in b["log"]], (name, i)
            assert a["iterations"] <= 200 and all(l["trials"] <= 10 for l in a["log"])
            for k in ("Rwg", "scale", "bg", "ba", "vel"):
                if np.size(a[k]):
                    d = float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max())
                    worst = max(worst, d)
                    assert d <= 1e-9, (name, i, k, d)
            assert np.array_equal(a["reintegrate"], b["reintegrate"])
            if job["mode"] != GS:
                n = a["bias_norm"].astype(np.float64)
                n_band += int(np.sum(np.abs(n - 0.01) <= 0.01 * cases.BAND))
                n_kf += len(n)
                flags |= set(a["reintegrate"].tolist())
        assert n_band == 0, (name, n_band, n_kf)
    assert flags == {0, 1}
    print(f"[inertial ref] dense vs structured: worst output difference {worst:.3g}")


def test_nan_record_rejects_every_trial(oracle):
    job = si.make_job(65, 77, FULL, False, 1e2, 1e5)
    job["preint"] = job["preint"].copy()
    job["preint"][20, 10] = np.nan
    r = ref.optimize(job)
    assert (r["iterations"], r["trials"], r["exit"]) == (200, 200, "max_iterations")
    assert np.array_equal(r["vel"], job["vel"]) and np.array_equal(r["bg"], job["bg0"]) and r["scale"] == job["scale"]
    assert np.array_equal(r["Rwg"].reshape(-1), np.asarray(job["Rwg"]).reshape(-1))


# ---- the feature's host side -------------------------------------------------------------------------------------------------
def test_select_edges_and_initial_guess():
    # keyframes 0..5; 3 is bad (no edge into it, but the edge 3 -> 4 stays); 5 is newer than maxKFid
    keep, k1, k2 = ii.select_edges(prev=[-1, 0, 1, 2, 3, 4], kf_id=[0, 1, 2, 3, 4, 9], is_bad=[0, 0, 0, 1, 0, 0], max_kf_id=4)
    assert keep.tolist() == [0, 1, 2, 3, 4] and k1.tolist() == [0, 1, 3] and k2.tolist() == [1, 2, 4]
    job = si.make_job(12, 9, FULL, False, 1e2, 1e5)
    g = ii.initial_guess(job)
    assert g["vel"].shape == (12, 3) and np.array_equal(g["vel"], g["vel"].astype(np.float32))
    assert _angle(g["Rwg"], job) < np.radians(10) and abs(np.linalg.det(g["Rwg"]) - 1) < 1e-5
    assert np.abs(g["vel"] - job["truth_vel"]).max() < 0.3


def test_exported_symbols_and_python_signatures():
    names = ["omv_inertial_opt_create", "omv_inertial_opt_destroy", "omv_inertial_optimization", "omv_inertial_opt_debug",
             "omv_inertial_opt_plan"]
    assert all(n in _lib.SIGNATURES for n in names)
    header = open(os.path.join(ROOT, "include", "omv.h")).read()
    assert all(f"omv_status {n}(" in header for n in names)
    assert f"#define OMV_INERTIAL_MAX_KF {ii.MAX_KF}" in header and ii.MAX_KF >= 300
    assert os.path.exists(_lib.LIB_PATH), "libomv_hip.so not built"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert list(inspect.signature(ii.InertialOptimization).parameters) == ["jobs", "mode", "mono", "priorG", "priorA",
                                                                           "optimizer"]
    assert list(inspect.signature(si.make_job).parameters)[:8] == ["K", "seed", "mode", "mono", "priorG", "priorA",
                                                                    "breaks", "isolated"]


def test_adapter_and_consumer_compile():
    """omv_adapt::InertialOptimization and tests/cpp/inertial_opt_consumer.cpp compile with g++ -Wall -Werror against
    omv.h and the HIP runtime headers alone (run on the GPU by tests/test_inertial_gpu.py)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    assert shutil.which("g++") is not None and os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h"))
    src = os.path.join(ROOT, "tests", "cpp", "inertial_opt_consumer.cpp")
    assert os.path.exists(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                        os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-fsyntax-only", src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
