"""tests/optsim3_ref.py on the CPU: the reference the device OptimizeSim3 is tested against, and the parts of the feature
that need no GPU (the exported symbols, the Python signatures, the adapter's compile)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import optsim3_ref as ref
from openmavis_amd import _lib, synth_optsim3 as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB8, PIN = 0, 1


# ---- i. analytic against numeric Jacobians ---------------------------------------------------------------------------
@pytest.mark.parametrize("models", [(KB8, KB8), (PIN, PIN), (KB8, PIN), (PIN, KB8)])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_analytic_jacobians_against_g2o_numeric(oracle, models, fix_scale):
    """Each 2 x 7 block of both edges, at the start value and after one oplus, within 1e-5 of the block's largest entry
    (central differences with delta 1e-9 carry about u |proj| / delta = 1e-4 px of noise on entries of 1e2 .. 1e4).
    Both schemes run on the smooth float64 projection.  Measured maximum over these cases: 5.0e-7 (a KB8 side), 2.5e-7
    (Pinhole on both sides)."""
    worst = 0.0
    for seed in (5, 6, 7):
        job = so.make_job(60, seed, model1=models[0], model2=models[1], fix_scale=fix_scale, no_kp2_share=0.1)
        pre = ref.prepare(job)
        S = ref.start_of(job)
        for S in (S, ref.oplus(S, [0.01, -0.02, 0.015, 0.03, -0.01, 0.02, 0.05], fix_scale)):
            Ja = ref.jacobians(job, pre, S, fix_scale, "analytic", "smooth")
            Jn = ref.jacobians(job, pre, S, fix_scale, "numeric", "smooth")
            for a, n in zip(Ja, Jn):
                rel = np.abs(a - n).max(axis=(1, 2)) / np.abs(a).max(axis=(1, 2))
                worst = max(worst, rel[pre["edge"]].max())
                if fix_scale:
                    assert not a[:, :, 6].any() and not n[:, :, 6].any()
            # e12's scale column vanishes up to rounding (a projection ignores the length of S12 X2); e21's does not
            assert fix_scale or (np.abs(Ja[0][:, :, 6]).max() < 1e-9 and np.abs(Ja[1][:, :, 6]).max() > 1)
    print(f"[optsim3 ref i] models {models} fix {fix_scale}: worst block difference {worst:.3g}")
    assert worst <= 1e-5


def test_literal_projection_is_the_float_quantised_one(oracle):
    """KannalaBrandt8::project(Vector3d) takes its two angles through atan2f: the literal projection differs from the
    smooth one by float rounding of the angles (about 1e-5 px), and a 1e-9 step does not move it."""
    job = so.make_job(60, 5, model1=KB8, model2=KB8)
    pre = ref.prepare(job)
    X = pre["X2"][pre["edge"]]
    a, b = ref.project(KB8, job["cam1"], X, "literal"), ref.project(KB8, job["cam1"], X, "smooth")
    assert 1e-8 < np.abs(a - b).max() < 1e-3
    assert np.array_equal(ref.project(PIN, so.ss.PINHOLE, X, "literal"), ref.project(PIN, so.ss.PINHOLE, X, "smooth"))
    assert (ref.project(KB8, job["cam1"], X + 1e-9, "literal") == a).mean() > 0.9


# ---- ii. Sim3(update), *, inverse ------------------------------------------------------------------------------------
def _closed_form(u):
    """exp of the sim(3) element by its series: (R, t, s) from the 4 x 4 matrix exponential's blocks."""
    w, v, sig = np.array(u[:3], np.float64), np.array(u[3:6], np.float64), float(u[6])
    A = np.zeros((4, 4))
    A[:3, :3] = ref.skew(w) + sig * np.eye(3)
    A[:3, 3] = v
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 40):
        term = term @ A / k
        E = E + term
    s = np.exp(sig)
    return E[:3, :3] / s, E[:3, 3], s


@pytest.mark.parametrize("u", [
    [0.3, -0.2, 0.4, 0.5, -1.0, 0.25, 0.2],        # the general branch
    [0.3, -0.2, 0.4, 0.5, -1.0, 0.25, 1e-7],       # |sigma| < eps
    [3e-6, -2e-6, 4e-6, 0.5, -1.0, 0.25, 0.2],     # theta < eps
    [3e-6, -2e-6, 4e-6, 0.5, -1.0, 0.25, -2e-6],   # both
    [0, 0, 0, 0, 0, 0, 0]])
def test_sim3_exp_against_matrix_exponential(u):
    q, t, s = ref.sim3_exp(u)
    R, t_exp, s_exp = _closed_form(u)
    # the reference's branches below eps = 1e-5 are truncations: R = I + Omega + Omega^2 (the exact series has
    # Omega^2 / 2: off by theta^2 / 2), C = 1 for (s - 1) / sigma (off by |sigma| / 2) and A = 1 / 2, B = 1 / 6 without
    # their first-order terms in sigma and theta; the translation is off by at most (|sigma| + theta) |upsilon|
    theta, sigma, ups = np.linalg.norm(u[:3]), abs(u[6]), np.linalg.norm(u[3:6])
    cut_t, cut_s = (theta if theta < 1e-5 else 0.0), (sigma if sigma < 1e-5 else 0.0)
    assert np.abs(ref.q_to_mat(q) - R).max() <= cut_t * cut_t + 1e-14
    assert np.abs(t - t_exp).max() <= (cut_t + cut_s) * ups + 1e-14 and abs(s - s_exp) <= 1e-15
    if not any(u):
        assert q.tolist() == [0, 0, 0, 1] and t.tolist() == [0, 0, 0] and s == 1.0


def test_sim3_group_operations():
    rng = np.random.default_rng(2)
    for _ in range(20):
        S = ref.sim3_exp(rng.normal(0, 0.4, 7))
        T = ref.sim3_exp(rng.normal(0, 0.4, 7))
        X = rng.normal(0, 3, (5, 3))
        I = ref.sim3_mul(S, ref.sim3_inverse(S))
        assert np.abs(ref.q_to_mat(I[0]) - np.eye(3)).max() < 1e-14 and np.abs(I[1]).max() < 1e-14 and abs(I[2] - 1) < 1e-14
        assert np.abs(ref.sim3_map(ref.sim3_mul(S, T), X) - ref.sim3_map(S, ref.sim3_map(T, X))).max() < 1e-12
        assert np.abs(ref.sim3_map(ref.sim3_inverse(S), ref.sim3_map(S, X)) - X).max() < 1e-12
        R = ref.q_to_mat(S[0])
        assert np.abs(ref.q_from_mat(R) * np.sign(ref.q_from_mat(R)[3] * S[0][3]) - S[0]).max() < 1e-14
        assert np.abs(ref.q_rot(S[0], X) - X @ R.T).max() < 1e-13


# ---- iii. the quirks --------------------------------------------------------------------------------------------------
def test_point_behind_camera_two_keeps_status_zero(oracle):
    job = so.make_job(80, 11, model1=PIN, model2=KB8, behind_share=0.2)
    r = ref.optimize_sim3(job)
    assert 5 < job["behind"].sum() and np.array_equal(~r["pre"]["edge"], job["behind"])
    assert (r["status"][job["behind"]] == ref.NOT_EDGE).all() and (r["status"][~job["behind"]] != ref.NOT_EDGE).all()
    assert r["n_in"] == (r["status"] == ref.INLIER).sum() > 30


def test_fewer_than_ten_survivors_returns_zero_unchanged(oracle):
    job = so.make_job(12, 709, outlier_share=0.0, model1=PIN, model2=PIN, noise_px=0.2)
    job["obs1"][:3] += np.float32(150.0)
    r = ref.optimize_sim3(job)
    assert r["n_in"] == 0 and r["dbg"]["n_removed_1"] == 3
    assert r["dbg"]["iterations"][0] >= 1 and len(r["dbg"]["iterations"]) == 1
    assert r["q"].tobytes() == np.asarray(job["q"], np.float64).tobytes() and r["t"].tobytes() == job["t"].tobytes()
    assert r["s"] == job["s"] and r["status"].tolist() == [2, 2, 2] + [0] * 9
    job["obs1"][2] -= np.float32(150.0)   # ten survivors: the second round runs and the estimate is written back
    r = ref.optimize_sim3(job)
    assert r["n_in"] == 10 and r["status"].tolist() == [2, 2] + [1] * 10 and len(r["dbg"]["iterations"]) == 2
    assert r["t"].tobytes() != job["t"].tobytes() and not r["H_acum"].any()


@pytest.mark.parametrize("models", [(KB8, PIN), (PIN, PIN)])
def test_fix_scale_leaves_s_bitwise_and_zeroes_row_six(oracle, models):
    job = so.make_job(70, 21, model1=models[0], model2=models[1], fix_scale=True)
    job["s"] = 1.0371   # any value: the update's scale factor is exp(0) = 1
    for jac in ("analytic", "numeric"):
        r = ref.optimize_sim3(job, jac, "smooth")
        assert r["s"] == 1.0371 and r["n_in"] > 30 and r["t"].tobytes() != job["t"].tobytes()
        H, b = r["dbg"]["H"], r["dbg"]["b"]
        assert not H[6].any() and not H[:, 6].any() and b[6] == 0 and r["dbg"]["x"][6] == 0 and H[5, 5] > 0


def test_nan_pair_is_kept_and_counted(oracle):
    job = so.make_job(40, 31, model1=PIN, model2=PIN)
    job["q"], job["t"], job["s"] = so.synth.quat_from_R(job["R12"]), job["t12"].copy(), job["s12"]
    k = int(np.nonzero(job["inlier"])[0][0])
    job["Xw2"][k] = np.float32(np.nan)
    r = ref.optimize_sim3(job)
    assert r["status"][k] == ref.INLIER and r["n_in"] == (r["status"] == ref.INLIER).sum() > 10
    assert r["q"].tobytes() == job["q"].tobytes() and r["dbg"]["max_trials"] == [1, 1] and r["dbg"]["iterations"] == [10, 10]


# ---- iv. a planted similarity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("models,fix_scale", [((KB8, KB8), False), ((PIN, KB8), True), ((PIN, PIN), False)])
def test_planted_similarity_with_outliers(oracle, models, fix_scale):
    for seed in (41, 42):
        job = so.make_job(150, seed, outlier_share=0.3, model1=models[0], model2=models[1], fix_scale=fix_scale,
                          no_kp2_share=0.1, behind_share=0.03)
        r = ref.optimize_sim3(job)
        gross = ~job["inlier"] & ~job["behind"]
        assert gross.sum() > 25 and (r["status"][gross] >= ref.REMOVED_1).all()
        assert r["n_in"] == (r["status"] == ref.INLIER).sum() >= 0.85 * (job["inlier"].sum())
        assert all(1 <= i <= 10 for i in r["dbg"]["iterations"]) and all(m <= 10 for m in r["dbg"]["max_trials"])
        # the refinement ends nearer the planted similarity than it started
        err = lambda q, t: (np.abs(ref.q_to_mat(np.asarray(q)) - job["R12"]).max(), np.abs(np.asarray(t) - job["t12"]).max())
        assert err(r["q"], r["t"])[0] < err(job["q"], job["t"])[0] and err(r["q"], r["t"])[0] < 3e-3
        assert abs(r["s"] - job["s12"]) < 0.01 * job["s12"]
        rn = ref.optimize_sim3(job, "numeric", "smooth")
        assert np.array_equal(rn["status"], r["status"]) and np.abs(rn["t"] - r["t"]).max() < 1e-4


# ---- v. the feature's host side ------------------------------------------------------------------------------------------
def test_exported_symbols_and_python_signatures():
    from openmavis_amd import optimizer
    names = ["omv_optimize_sim3_create", "omv_optimize_sim3_destroy", "omv_optimize_sim3", "omv_optimize_sim3_debug"]
    assert all(n in _lib.SIGNATURES for n in names)
    header = open(os.path.join(ROOT, "include", "omv.h")).read()
    assert all(f"omv_status {n}(" in header for n in names)
    assert os.path.exists(_lib.LIB_PATH), "libomv_hip.so not built"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert list(inspect.signature(optimizer.OptimizeSim3).parameters)[:1] == ["jobs"]
    assert list(inspect.signature(optimizer.select_sim3_edges).parameters) == [
        "matched", "cam_of_kp1", "cameraID1", "mp1_ok", "mp2_ok", "i2", "bAllPoints"]
    # the graph-side filter of :2522-2589 on arrays
    idx, has = optimizer.select_sim3_edges(matched=[1, 1, 0, 1, 1, 1, 1], cam_of_kp1=[0, 0, 0, 1, 0, 0, 0], cameraID1=0,
                                           mp1_ok=[1, 1, 1, 1, 0, 1, 1], mp2_ok=[1, 1, 1, 1, 1, 0, 1],
                                           i2=[4, -1, 3, 2, 1, 0, 9])
    assert idx.tolist() == [0, 6] and has.tolist() == [True, True]
    idx, has = optimizer.select_sim3_edges([1, 1, 0, 1, 1, 1, 1], [0, 0, 0, 1, 0, 0, 0], 0, [1, 1, 1, 1, 0, 1, 1],
                                           [1, 1, 1, 1, 1, 0, 1], [4, -1, 3, 2, 1, 0, 9], bAllPoints=True)
    assert idx.tolist() == [0, 1, 6] and has.tolist() == [True, False, True]


def test_adapter_and_consumer_compile():
    """omv_adapt::OptimizeSim3 and tests/cpp/optimize_sim3_consumer.cpp compile with g++ -Wall -Werror against omv.h and
    the HIP runtime headers alone (run on the GPU by tests/test_optsim3_gpu.py)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("g++ or HIP headers absent")
    src = os.path.join(ROOT, "tests", "cpp", "optimize_sim3_consumer.cpp")
    assert os.path.exists(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                        os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-fsyntax-only", src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
