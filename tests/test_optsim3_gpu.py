"""The device OptimizeSim3 (openmavis_amd/csrc/optsim3.hip through openmavis_amd/optimizer.py) against
tests/optsim3_ref.py.

a. first system  the debug hook's initial e12 / e21, H, b, chi2, lambda_init and x against the analytic reference at the
                 input S12: residuals within 1e-9 px; H, b, x within 1e-9 of their largest entry; row and column 6 of H
                 exactly zero under fix_scale
b. outcome       per case of >= 20 jobs e_num(q), q in {R(q), t, s}: the largest difference over the case's jobs between
                 the reference's numeric (g2o's +-1e-9 central differences) and analytic runs; every job's device result
                 must be within e_num(q) of the analytic run.  The numeric / analytic pair runs on the smooth float64
                 projection (central differences through KannalaBrandt8's atan2f-quantised projection are meaningless),
                 the analytic run the device is compared with on the literal one the device restates; for Pinhole the
                 two projections are the same function.  LM counts are bounded, not compared.
c. statuses      with the device's returned S12 the float64 reference errors decide every pair whose two chi2 are outside
                 th2 (1 +- 2^-10); round one by the reference's own round-one chi2; decided pairs match exactly, n_in is
                 the number of status-1 entries, at most 1 % of a case's pairs inside the band
d. return 0      9 survivors, N = 0, N = 1: n_in 0, S12 bitwise unchanged, the round-one removals reported
e. fix_scale     s out bitwise s in
f. NaN           one NaN world point in a job of 65: OMV_OK, S12 bitwise unchanged, statuses by the literal comparisons
g. determinism   two calls give bitwise identical S12, statuses and debug sums
h. argument errors
i. chain         Sim3Solver.find -> OptimizeSim3 from its T12 equals the reference from the same start under b's bound;
                 the C++ consumer gives the Python call's nIn, statuses and S12

Measured on an MI355X (pytest -s prints the figures): see DESIGN.md section 6."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import optsim3_ref as ref
from openmavis_amd import _lib, build as omv_build, optimizer, sim3solver, synth_optsim3 as so, synth_sim3solver as ss

pytestmark = pytest.mark.gpu

DELTA = 2.0 ** -10
KB8, PIN = 0, 1
MODELS = [(KB8, KB8), (PIN, PIN), (KB8, PIN), (PIN, KB8)]

# ragged calls of 24 and 20 jobs: N = 0, 1, the wavefront edges 63 / 64 / 65, two and five passes (130, 300)
NS_MIX = (0, 1, 63, 64, 65, 130, 300, 20, 33, 100, 64, 65, 12, 47, 128, 129, 200, 63, 90, 10, 30, 64, 150, 75)
NS_KB8 = (65, 64, 130, 40, 100, 63, 25, 80, 300, 50, 64, 129, 70, 35, 110, 65, 90, 45, 160, 60)
CASES = {
    "mix": dict(ns=NS_MIX, seed=101, models=[MODELS[j % 4] for j in range(len(NS_MIX))],
                fix_scale=[(j // 4) % 2 == 1 for j in range(len(NS_MIX))], no_kp2_share=0.15, behind_share=0.05),
    "kb8": dict(ns=NS_KB8, seed=301, models=[(KB8, KB8)] * len(NS_KB8), fix_scale=[j % 5 == 0 for j in range(len(NS_KB8))],
                no_kp2_share=0.0, behind_share=0.0),
    "pin_fix": dict(ns=NS_KB8, seed=501, models=[(PIN, PIN)] * len(NS_KB8), fix_scale=[True] * len(NS_KB8),
                    no_kp2_share=0.1, behind_share=0.02),
}


def _jobs(name):
    c = CASES[name]
    return so.make_jobs(list(c["ns"]), seed=c["seed"], models=c["models"], fix_scale=c["fix_scale"],
                        no_kp2_share=c["no_kp2_share"], behind_share=c["behind_share"])


def _run(jobs):
    """One device call -> (n_in, q, t, s, status, debug per job)."""
    opt = optimizer.Sim3Optimizer(max(len(jobs), 1), sum(len(j["index1"]) for j in jobs))
    code, n_in, q, t, s, status = opt.run(jobs)
    assert code == _lib.OMV_OK
    return n_in, q, t, s, status, [opt.debug(j) for j in range(len(jobs))]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(jobs, device result, the reference's analytic run on the literal projection per job) -- computed once."""
    jobs = _jobs(name)
    return jobs, _run(jobs), [ref.optimize_sim3(j, "analytic", "literal") for j in jobs]


@functools.lru_cache(maxsize=None)
def _e_num(name):
    """e_num(R), e_num(t), e_num(s) of a case: numeric against analytic, both on the smooth projection."""
    e = dict(R=0.0, t=0.0, s=0.0)
    for j in _jobs(name):
        a, b = ref.optimize_sim3(j, "numeric", "smooth"), ref.optimize_sim3(j, "analytic", "smooth")
        e["R"] = max(e["R"], np.abs(ref.q_to_mat(a["q"]) - ref.q_to_mat(b["q"])).max())
        e["t"] = max(e["t"], np.abs(a["t"] - b["t"]).max())
        e["s"] = max(e["s"], abs(a["s"] - b["s"]))
    return e


def _bits(*a):
    return b"".join(np.ascontiguousarray(x, np.float64).tobytes() for x in a)


# ---- a. the first system ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix", "kb8"])
def test_first_system_against_analytic_reference(torch_cuda, name):
    jobs, (n_in, q, t, s, status, dbg), refs = _case(name)
    worst = dict(e=0.0, H=0.0, b=0.0, x=0.0, chi2=0.0, lam=0.0)
    n_sys = 0
    for j, (job, d, r) in enumerate(zip(jobs, dbg, refs)):
        pre = r["pre"]
        edge = pre["edge"]
        e12, e21 = r["dbg"]["e12_0"], r["dbg"]["e21_0"]
        if edge.any():
            worst["e"] = max(worst["e"], np.abs(d["e12"][edge] - e12[edge]).max(), np.abs(d["e21"][edge] - e21[edge]).max())
            assert np.abs(d["e12"][edge] - e12[edge]).max() <= 1e-9 and np.abs(d["e21"][edge] - e21[edge]).max() <= 1e-9, j
        assert not d["e12"][~edge].any() and not d["e21"][~edge].any()
        if not edge.any():
            assert not d["H"].any() and d["iterations"].tolist() == [0, 0]
            continue
        n_sys += 1
        rd = r["dbg"]
        for k, got, exp in (("H", d["H"], rd["H"]), ("b", d["b"], rd["b"]), ("x", d["x"], rd["x"])):
            rel = np.abs(got - exp).max() / np.abs(exp).max()
            worst[k] = max(worst[k], rel)
            assert rel <= 1e-9, (j, k, rel)
        worst["chi2"] = max(worst["chi2"], abs(d["chi2"] - rd["chi2"]) / rd["chi2"])
        worst["lam"] = max(worst["lam"], abs(d["lambda_init"] - rd["lambda_init"]) / rd["lambda_init"])
        assert abs(d["chi2"] - rd["chi2"]) <= 1e-9 * rd["chi2"]
        assert abs(d["lambda_init"] - rd["lambda_init"]) <= 1e-9 * rd["lambda_init"]
        assert np.array_equal(d["H"], d["H"].T)
        if job["fix_scale"]:
            assert not d["H"][6].any() and not d["H"][:, 6].any() and d["b"][6] == 0 and d["x"][6] == 0
        else:
            assert d["H"][6, 6] > 0
    print(f"[optsim3 a] {name}: {n_sys} systems; worst residual error {worst['e']:.3g} px, relative H {worst['H']:.3g} "
          f"b {worst['b']:.3g} x {worst['x']:.3g} chi2 {worst['chi2']:.3g} lambda {worst['lam']:.3g}")
    assert n_sys >= 18


# ---- b. the outcome --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix", "kb8", "pin_fix"])
def test_outcome_within_differentiation_noise(torch_cuda, name):
    jobs, (n_in, q, t, s, status, dbg), refs = _case(name)
    e_num = _e_num(name)
    assert len(jobs) >= 20
    ratio = dict(R=0.0, t=0.0, s=0.0)
    fails = []
    for j, (job, d, r) in enumerate(zip(jobs, dbg, refs)):
        err = dict(R=np.abs(ref.q_to_mat(q[j]) - ref.q_to_mat(r["q"])).max(), t=np.abs(t[j] - r["t"]).max(),
                   s=abs(s[j] - r["s"]))
        for k in ratio:
            if err[k] > 0:
                ratio[k] = max(ratio[k], err[k] / e_num[k] if e_num[k] > 0 else np.inf)
            if not err[k] <= e_num[k]:
                fails.append((j, k, err[k], e_num[k]))
        # the LM loops are bounded; their counts are rounding noise at convergence and not compared
        removed = int((status[j] == ref.REMOVED_1).sum())
        assert 0 <= d["iterations"][0] <= 10 and 0 <= d["iterations"][1] <= (10 if removed else 5), (j, d["iterations"])
        assert (d["max_trials"] <= 10).all() and (d["trials"] <= 10 * d["iterations"]).all()
        assert (d["trials"] >= d["iterations"]).all()
    print(f"[optsim3 b] {name}: e_num R {e_num['R']:.3g} t {e_num['t']:.3g} s {e_num['s']:.3g}; worst e / e_num "
          f"R {ratio['R']:.3g} t {ratio['t']:.3g} s {ratio['s']:.3g}")
    assert not fails, fails


# ---- c. statuses -----------------------------------------------------------------------------------------------------
def _band(c, th2):
    return (c >= th2 * (1 - DELTA)) & (c <= th2 * (1 + DELTA))


@pytest.mark.parametrize("name", ["mix", "kb8", "pin_fix"])
def test_statuses_decided_by_reference_errors(torch_cuda, name):
    jobs, (n_in, q, t, s, status, dbg), refs = _case(name)
    tot = in_band = 0
    seen = set()
    for j, (job, r) in enumerate(zip(jobs, refs)):
        pre, st = r["pre"], status[j]
        th2 = pre["th2"]
        assert len(st) == len(job["index1"]) and n_in[j] == (st == ref.INLIER).sum()
        assert (st[~pre["edge"]] == ref.NOT_EDGE).all()   # z < 0: no edge, the match kept
        seen |= set(st.tolist())
        with np.errstate(all="ignore"):
            c12, c21 = r["dbg"]["chi2_round1"]
            band1 = (_band(c12, th2) | _band(c21, th2)) & pre["edge"]
            bad1 = pre["edge"] & ((c12 > th2) | (c21 > th2))
            ok = ~band1 & pre["edge"]
            assert np.array_equal((st == ref.REMOVED_1)[ok], bad1[ok]), j
            tot += int(pre["edge"].sum())
            in_band += int(band1.sum())
            if r["n_in"] == 0 and (r["status"] == ref.INLIER).sum() == 0 and not band1.any():   # the return-0 path
                assert n_in[j] == 0 and not (st == ref.INLIER).any() and not (st == ref.REMOVED_2).any(), j
                continue
            S = (q[j], t[j], s[j])
            f12, f21 = ref.chi2_of(pre, *ref.errors(job, pre, S, "literal"))
            kept = pre["edge"] & (st != ref.REMOVED_1)
            band2 = (_band(f12, th2) | _band(f21, th2)) & kept
            ok = kept & ~band2
            assert np.array_equal((st == ref.REMOVED_2)[ok], ((f12 > th2) | (f21 > th2))[ok]), j
            in_band += int(band2.sum())
        # every gross outlier of the planted problem ends removed
        gross = ~job["inlier"] & pre["edge"]
        assert (st[gross] >= ref.REMOVED_1).all() or r["n_in"] == 0, j
    print(f"[optsim3 c] {name}: {in_band} of {tot} pairs inside the band ({in_band / max(tot, 1):.4%}); "
          f"statuses seen {sorted(seen)}")
    assert in_band <= 0.01 * tot
    assert {ref.INLIER, ref.REMOVED_1} <= seen


# ---- d. the return-0 path --------------------------------------------------------------------------------------------
def _survivor_job(n_good, n_gross, seed, model, fix):
    """n_good clean pairs (0.2 px noise, no outliers) and n_gross pairs whose KF1 keypoint is 150 px off."""
    job = so.make_job(n_good + n_gross, seed, outlier_share=0.0, model1=model, model2=model, fix_scale=fix, noise_px=0.2)
    job["obs1"][:n_gross] += np.float32(150.0)
    return job


@functools.lru_cache(maxsize=None)
def _survivor_case():
    jobs = [_survivor_job(g, 12 - g, 700 + g, (KB8, PIN)[g % 2], g == 10) for g in (9, 10, 11)]
    jobs += [so.make_job(n, 720 + n, model1=PIN, model2=KB8) for n in (0, 1)]
    return jobs, _run(jobs), [ref.optimize_sim3(j, "analytic", "literal") for j in jobs]


def test_fewer_than_ten_survivors_returns_zero(torch_cuda):
    jobs, (n_in, q, t, s, status, dbg), refs = _survivor_case()
    # the cases are what they are named for (the reference, on the CPU)
    survivors = [int(r["pre"]["edge"].sum()) - r["dbg"]["n_removed_1"] for r in refs]
    assert survivors[:4] == [9, 10, 11, 0] and survivors[4] <= 1
    assert [r["dbg"]["n_removed_1"] for r in refs[:3]] == [3, 2, 1]
    for j in (0, 3, 4):   # 9 survivors, N = 0, N = 1
        assert n_in[j] == 0 == refs[j]["n_in"]
        assert _bits(q[j], t[j], s[j]) == _bits(jobs[j]["q"], jobs[j]["t"], jobs[j]["s"]), j
        assert np.array_equal(status[j], refs[j]["status"]) and not (status[j] == ref.INLIER).any()
        assert dbg[j]["iterations"][1] == 0
    assert (status[0] == ref.REMOVED_1).sum() == 3 and (status[0][:3] == ref.REMOVED_1).all()
    for j in (1, 2):   # 10 and 11 survivors: the second round runs
        assert n_in[j] == refs[j]["n_in"] == survivors[j] and np.array_equal(status[j], refs[j]["status"])
        assert _bits(q[j], t[j], s[j]) != _bits(jobs[j]["q"], jobs[j]["t"], jobs[j]["s"])
        assert dbg[j]["iterations"][1] >= 1
        assert np.abs(t[j] - refs[j]["t"]).max() < 1e-6


# ---- e. fixed scale --------------------------------------------------------------------------------------------------
def test_fix_scale_leaves_s_bitwise(torch_cuda):
    n_fixed = 0
    for name in ("mix", "pin_fix"):
        jobs, (n_in, q, t, s, status, dbg), refs = _case(name)
        for j, job in enumerate(jobs):
            if job["fix_scale"]:
                assert _bits(s[j]) == _bits(job["s"]), (name, j)
                n_fixed += n_in[j] > 0
            elif n_in[j] > 0:
                assert s[j] != job["s"]
    assert n_fixed >= 20


# ---- f. NaN ----------------------------------------------------------------------------------------------------------
def test_nan_world_point_rejects_every_trial(torch_cuda):
    from openmavis_amd.synth import quat_from_R
    job = so.make_job(65, 801, model1=KB8, model2=PIN)
    job["q"], job["t"], job["s"] = quat_from_R(job["R12"]), job["t12"].copy(), job["s12"]   # no trial will move it
    k = int(np.nonzero(job["inlier"])[0][3])
    job["Xw2"][k] = np.float32(np.nan)
    n_in, q, t, s, status, dbg = _run([job])   # OMV_OK is asserted there
    r = ref.optimize_sim3(job, "analytic", "literal")
    assert _bits(q[0], t[0], s[0]) == _bits(job["q"], job["t"], job["s"]) == _bits(r["q"], r["t"], r["s"])
    # the literal comparisons: a NaN chi2 is not > th2, so the pair is kept and counted
    assert status[0][k] == ref.INLIER and np.array_equal(status[0], r["status"]) and n_in[0] == r["n_in"] > 10
    assert (status[0] == ref.REMOVED_1).any()
    assert np.isnan(dbg[0]["chi2"]) and (dbg[0]["max_trials"] == 1).all() and dbg[0]["iterations"].tolist() == [10, 10]
    assert dbg[0]["iterations"].tolist() == r["dbg"]["iterations"]


# ---- g. determinism --------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_identical(torch_cuda):
    jobs = _jobs("mix")
    a, b = _run(jobs), _run(jobs)
    assert _bits(a[1], a[2], a[3]) == _bits(b[1], b[2], b[3]) and np.array_equal(a[0], b[0])
    for j in range(len(jobs)):
        assert np.array_equal(a[4][j], b[4][j])
        for k in ("H", "b", "x", "e12", "e21"):
            assert a[5][j][k].tobytes() == b[5][j][k].tobytes(), (j, k)
        assert _bits(a[5][j]["chi2"], a[5][j]["lambda_init"]) == _bits(b[5][j]["chi2"], b[5][j]["lambda_init"])
        assert a[5][j]["trials"].tolist() == b[5][j]["trials"].tolist()


# ---- h. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    jobs = so.make_jobs([10, 12], seed=61, models=(PIN, PIN))
    opt = optimizer.Sim3Optimizer(2, 22)
    assert opt.run(jobs)[0] == _lib.OMV_OK
    for key, bad in (("model1", 2), ("model2", -1)):
        keep, jobs[1][key] = jobs[1][key], bad
        assert opt.run(jobs)[0] == _lib.OMV_ERR_ARG, key
        jobs[1][key] = keep
    assert optimizer.Sim3Optimizer(1, 22).run(jobs)[0] == _lib.OMV_ERR_ARG   # more jobs than the handle holds
    assert optimizer.Sim3Optimizer(2, 21).run(jobs)[0] == _lib.OMV_ERR_ARG   # more entries
    lib = _lib.load()
    z = np.zeros(64, np.float32)
    d = np.zeros(8)
    i32 = np.zeros(4, np.int32)
    u8 = np.zeros(64, np.uint8)

    def call(n_jobs, start, first=z, last=u8):
        pin = np.ones(4, np.int32)   # both models Pinhole
        return lib.omv_optimize_sim3(opt._h, n_jobs, _lib.ptr(np.asarray(start, np.int32)), _lib.ptr(first),
                                     *[_lib.ptr(z)] * 3, _lib.ptr(u8), *[_lib.ptr(z)] * 6, _lib.ptr(pin), _lib.ptr(pin),
                                     _lib.ptr(i32), _lib.ptr(z), _lib.ptr(d), _lib.ptr(d), _lib.ptr(d), _lib.ptr(i32),
                                     _lib.ptr(last), opt._stream())

    assert call(-1, [0, 0]) == _lib.OMV_ERR_ARG               # a negative size
    assert call(2, [0, 5, 3]) == _lib.OMV_ERR_ARG             # entry_start not ascending
    assert call(2, [1, 2, 3]) == _lib.OMV_ERR_ARG             # entry_start[0] != 0
    assert call(1, [0, 4], first=None) == _lib.OMV_ERR_ARG    # a null pointer with a non-zero size
    assert call(1, [0, 4], last=None) == _lib.OMV_ERR_ARG
    assert call(1, [0, 0], first=None, last=None) == _lib.OMV_OK   # no entries: the entry arrays may be null
    assert call(0, [0]) == _lib.OMV_OK
    assert lib.omv_optimize_sim3_debug(opt._h, 3, *[None] * 10, opt._stream()) == _lib.OMV_ERR_ARG
    h = optimizer.ctypes.c_void_p()
    assert lib.omv_optimize_sim3_create(0, 10, optimizer.ctypes.byref(h)) == _lib.OMV_ERR_ARG
    assert lib.omv_optimize_sim3_create(1, -1, optimizer.ctypes.byref(h)) == _lib.OMV_ERR_ARG


# ---- i. the chain ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain():
    """Sim3Solver.find on 20 planted jobs, then OptimizeSim3 from its estimate on the device and in the reference."""
    n_jobs = 20
    jobs = so.make_jobs([100] * n_jobs, seed=901, models=[MODELS[j % 4] for j in range(n_jobs)], outlier_share=0.3)
    sj = [dict(j, sigma2_1=(np.float32(1) / j["inv_sigma2_1"]), sigma2_2=(np.float32(1) / j["inv_sigma2_2"])) for j in jobs]
    solver = sim3solver.Sim3Solver(sj, max_hyp=300)
    solver.SetRansacParameters(0.99, 20, 300)
    solver.find(solver.draw(np.random.default_rng(5), int(solver.max_its.max())))
    assert (solver.flags.cpu().numpy()[:n_jobs] == sim3solver.CONVERGE).all()
    from openmavis_amd.synth import quat_from_R
    for j, job in enumerate(jobs):
        job["q"] = quat_from_R(solver.GetEstimatedRotation(j).astype(np.float64))
        job["t"] = solver.GetEstimatedTranslation(j).astype(np.float64)
        job["s"] = float(solver.GetEstimatedScale(j))
    return jobs, optimizer.OptimizeSim3(jobs), [ref.optimize_sim3(j, "analytic", "literal") for j in jobs]


def test_chain_sim3solver_then_optimize_sim3(torch_cuda):
    jobs, out, refs = _chain()
    e_num = dict(R=0.0, t=0.0, s=0.0)
    for j in jobs:
        a, b = ref.optimize_sim3(j, "numeric", "smooth"), ref.optimize_sim3(j, "analytic", "smooth")
        e_num["R"] = max(e_num["R"], np.abs(ref.q_to_mat(a["q"]) - ref.q_to_mat(b["q"])).max())
        e_num["t"] = max(e_num["t"], np.abs(a["t"] - b["t"]).max())
        e_num["s"] = max(e_num["s"], abs(a["s"] - b["s"]))
    ratio = dict(R=0.0, t=0.0, s=0.0)
    for j, (job, (n_in, S, m), r) in enumerate(zip(jobs, out, refs)):
        assert n_in == r["n_in"] > 40 and m.sum() == (r["status"] < ref.REMOVED_1).sum()
        assert len(m) == job["index1"].max() + 1
        assert not m[job["index1"][~job["inlier"]]].any()   # every gross outlier's match is nulled
        err = dict(R=np.abs(ref.q_to_mat(S["q"]) - ref.q_to_mat(r["q"])).max(), t=np.abs(S["t"] - r["t"]).max(),
                   s=abs(S["s"] - r["s"]))
        for k in ratio:
            ratio[k] = max(ratio[k], err[k] / e_num[k])
        # near the planted similarity: a sanity check, not an accuracy bar (reprojection errors see the scale only
        # through the translation's parallax)
        assert np.abs(S["t"] - job["t12"]).max() < 0.1 and abs(S["s"] - job["s12"]) < 0.1 * job["s12"]
    print(f"[optsim3 i] chain: e_num R {e_num['R']:.3g} t {e_num['t']:.3g} s {e_num['s']:.3g}; worst e / e_num "
          f"R {ratio['R']:.3g} t {ratio['t']:.3g} s {ratio['s']:.3g}")
    assert max(ratio.values()) <= 1.0, ratio


def test_cpp_adapter_consumer_matches_python(torch_cuda, tmp_path):
    """tests/cpp/optimize_sim3_consumer.cpp (omv_adapt::OptimizeSim3, LoopClosing's call shape) as a child process on a
    job file: the same nIn, statuses, matches and S12 as the Python call."""
    if not os.path.exists(omv_build.OPTSIM3_CONSUMER_BIN):
        pytest.fail(f"{omv_build.OPTSIM3_CONSUMER_BIN} not built (python -m openmavis_amd.build)")
    job = so.make_job(100, 951, model1=KB8, model2=PIN, no_kp2_share=0.1, behind_share=0.05)
    n = len(job["index1"])
    path = tmp_path / "job.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<5if", n, job["mN1"], job["model1"], job["model2"], int(job["fix_scale"]), float(job["th2"])))
        for k, dt in (("pose1", np.float32), ("pose2", np.float32), ("cam1", np.float32), ("cam2", np.float32),
                      ("q", np.float64), ("t", np.float64), ("s", np.float64), ("index1", np.int32), ("Xw1", np.float32),
                      ("Xw2", np.float32), ("obs1", np.float32), ("obs2", np.float32), ("inv_sigma2_1", np.float32),
                      ("inv_sigma2_2", np.float32), ("has_kp2", np.uint8)):
            f.write(np.ascontiguousarray(job[k], dt).tobytes())
    r = subprocess.run([omv_build.OPTSIM3_CONSUMER_BIN, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip()[:200])
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    w = r.stdout.split()
    n_in, q, t, s, status, _ = _run([job])
    matches = np.zeros(job["mN1"], bool)
    matches[job["index1"]] = True
    (py_n, py_S, py_m), = optimizer.OptimizeSim3([job], vpMatches1=[matches])
    assert int(w[1]) == n_in[0] == py_n > 40 and w[3] == "".join(str(int(v)) for v in status[0])
    assert w[5] == "".join(str(int(v)) for v in py_m) and len(py_m) == job["mN1"]
    got = np.array([float(v) for v in w[7:11] + w[12:15] + [w[16]]])
    assert _bits(got) == _bits(q[0], t[0], s[0]) == _bits(py_S["q"], py_S["t"], py_S["s"])
    assert {0, 1, 2} <= set(status[0].tolist())
