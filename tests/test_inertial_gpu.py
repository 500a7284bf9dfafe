"""The device InertialOptimization (openmavis_amd/csrc/inertial.hip through openmavis_amd/inertial_init.py) against
tests/inertial_ref.py (float64 numpy, dense matrices, "literal" float32 deltas, dense Cholesky).

  a  the first system from the debug hook: residuals within 1e-9; every H block and b within 1e-9 of its largest entry;
     chi2 and lambda_init within 1e-9 relative (exactly 1e3 where the reference sets it); fixed unknowns' rows and
     columns exactly zero; the first trial's x by its residual in the reference's own system,
     max |(H + lambda I) x - b| <= 1e-9 (max |H + lambda I| max |x| + max |b|)
  b  the outcome: Rwg, scale, bg, ba, velocities within 1e-7 of the reference (the project's state bar for the
     pose-inertial kernels); the Levenberg counts bounded, not compared.  tests/test_inertial_ref_cpu.py shows that the
     reference's own dense and structured solves take the same decisions on these jobs.
  c  the epilogue: float velocities the casts of the double ones; the Reintegrate() flags against the float test with the
     device's bg outside a 2^-10 band round 0.01
  d  fixed things stay fixed bitwise; e degenerate jobs; f a NaN record; g determinism; h argument errors; i the chain
     device preintegration -> initial_guess -> InertialOptimization -> re-integration, and the C++ consumer.

Measured on an MI355X (this file, 23 + 20 jobs): see DESIGN.md section 6, "InertialOptimization"."""
import ctypes
import os
import subprocess
import struct

import numpy as np
import pytest

import inertial_cases as cases
import inertial_ref as ref
from openmavis_amd import _lib, build as omv_build, imu, inertial_init as ii, synth_inertial as si

pytestmark = pytest.mark.gpu
FULL, BIAS, GS = ii.FULL, ii.BIAS, ii.GS
OUT = ("Rwg", "scale", "bg", "ba", "vel")


@pytest.fixture(scope="module")
def main(torch_cuda):
    """(jobs, device results, debug dicts, reference runs) of the main call, computed once."""
    jobs = cases.make()
    opt = ii.InertialOptimizer(len(jobs), sum(len(j["Rwb"]) for j in jobs), sum(len(j["kf1"]) for j in jobs))
    got = ii.InertialOptimization(jobs, optimizer=opt)
    dbg = [opt.debug(i) for i in range(len(jobs))]
    want = [ref.optimize(j, "literal", "dense") for j in jobs]
    return jobs, got, dbg, want, opt


def _blocks(job, H, b):
    """The reference's dense system cut into the hook's blocks."""
    K, E = len(job["Rwb"]), len(job["kf1"])
    k1, k2 = np.asarray(job["kf1"], np.int64).reshape(-1), np.asarray(job["kf2"], np.int64).reshape(-1)
    Hvv = np.stack([H[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(K)]) if K else np.zeros((0, 3, 3))
    Hvoff = np.stack([H[3 * a:3 * a + 3, 3 * c:3 * c + 3] for a, c in zip(k1, k2)]) if E else np.zeros((0, 3, 3))
    return dict(Hvv=Hvv, Hvoff=Hvoff, border=H[:3 * K, 3 * K:].reshape(K, 3, 9), bv=b[:3 * K].reshape(K, 3),
                corner=H[3 * K:, 3 * K:], bc=b[3 * K:])


def test_a_first_system(main):
    jobs, got, dbg, want, _ = main
    worst = dict(e=0.0, H=0.0, chi2=0.0, lam=0.0, x=0.0)
    for i, (job, d, w) in enumerate(zip(jobs, dbg, want)):
        f = w["first"]
        K, E = len(job["Rwb"]), len(job["kf1"])
        if E:
            err = float(np.abs(d["e0"] - f["e0"]).max())
            worst["e"] = max(worst["e"], err)
            assert err <= 1e-9, (i, err)
        if job["mode"] == GS and E == 0:
            continue   # optimize() returns before any system is built
        B = _blocks(job, f["H"], f["b"])
        if job["mode"] == GS:   # the velocities are fixed: their rows are absent in the reference, zero on the device
            for k in ("Hvv", "Hvoff", "border", "bv"):
                assert not d[k].any(), (i, k)
            names = ("corner", "bc")
        else:
            names = ("Hvv", "Hvoff", "border", "bv", "corner", "bc")
        for k in names:
            if not B[k].size:
                continue
            scale = float(np.abs(B[k]).max())
            err = float(np.abs(d[k] - B[k]).max()) / scale if scale else float(np.abs(d[k]).max())
            worst["H"] = max(worst["H"], err)
            assert err <= 1e-9, (i, k, err)
        # rows and columns of fixed unknowns: exactly zero
        fixed = ~w["free"][3 * K:]
        assert not d["corner"][fixed].any() and not d["corner"][:, fixed].any() and not d["bc"][fixed].any(), i
        assert not d["border"][:, :, fixed].any(), i
        c = abs(d["chi2"] - f["chi2"]) / max(abs(f["chi2"]), 1e-300) if f["chi2"] else abs(d["chi2"])
        worst["chi2"] = max(worst["chi2"], c)
        assert c <= 1e-9, (i, d["chi2"], f["chi2"])
        if job["mode"] != GS:
            user = job["mode"] == BIAS or float(job["priorG"]) != 0.0
            if user:
                assert f["lambda_init"] == 1e3 and d["lambda_init"] == 1e3, i
            else:
                lam = abs(d["lambda_init"] - f["lambda_init"]) / f["lambda_init"]
                worst["lam"] = max(worst["lam"], lam)
                assert lam <= 1e-9, (i, lam)
        # the first trial's x, by its residual in the reference's own system
        x = np.concatenate([d["xv"].reshape(-1), d["xc"]])
        act = w["free"]
        assert not x[~act].any(), i
        A = f["H"][np.ix_(act, act)] + f["lambda_init"] * np.eye(int(act.sum()))
        if A.size:
            res = float(np.abs(A @ x[act] - f["b"][act]).max())
            bound = float(np.abs(A).max() * np.abs(x[act]).max() + np.abs(f["b"][act]).max())
            worst["x"] = max(worst["x"], res / bound if bound else res)
            assert res <= 1e-9 * bound, (i, res, bound)
    print(f"[inertial a] {len(jobs)} systems: worst residual error {worst['e']:.3g}, relative H / b block {worst['H']:.3g}, "
          f"chi2 {worst['chi2']:.3g}, lambda_init {worst['lam']:.3g}, solve residual / bound {worst['x']:.3g}")


def _compare(jobs, got, want, tag):
    worst = {k: 0.0 for k in OUT}
    for i, (job, g, w) in enumerate(zip(jobs, got, want)):
        for k in OUT:
            if np.size(w[k]):
                d = float(np.abs(np.asarray(g[k]) - np.asarray(w[k])).max())
                worst[k] = max(worst[k], d)
                assert d <= 1e-7, (tag, i, k, d)
        limit = 10 if job["mode"] == GS else 200
        assert 0 <= g["iterations"] <= limit and g["iterations"] <= g["trials"] <= 10 * max(g["iterations"], 1), (tag, i)
    print(f"[inertial b] {tag}: worst differences " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_b_outcome(main):
    jobs, got, dbg, want, _ = main
    _compare(jobs, got, want, "main")
    for d, g in zip(dbg, got):
        assert d["max_trials"] <= 10 and d["iterations"] == g["iterations"] and d["trials"] == g["trials"]


def test_c_epilogue(main):
    jobs, got, _, want, _ = main
    n_band = n_kf = 0
    seen = set()
    for i, (job, g) in enumerate(zip(jobs, got)):
        assert g["vel_f32"].dtype == np.float32 and np.array_equal(g["vel_f32"].view(np.uint32),
                                                                    g["vel"].astype(np.float32).view(np.uint32)), i
        if job["mode"] == GS:
            assert not g["reintegrate"].any()
            continue
        flag, n = ref.reintegrate_flags(job, g["bg"])
        band = np.abs(n.astype(np.float64) - 0.01) <= 0.01 * cases.BAND
        n_band += int(band.sum())
        n_kf += len(n)
        assert np.array_equal(g["reintegrate"][~band], flag[~band]), i
        seen |= set(g["reintegrate"].tolist())
    assert n_band <= cases.BAND_CAP * n_kf and seen == {0, 1}
    print(f"[inertial c] {n_band} of {n_kf} keyframes inside the band")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_d_fixed_things_stay_fixed_bitwise(main):
    jobs, got, _, _, _ = main
    n = [0, 0, 0]
    for job, g in zip(jobs, got):
        if job["mode"] == FULL and not job["mono"]:
            assert np.array_equal(_bits(g["scale"]), _bits(job["scale"]))
            n[0] += 1
        if job["mode"] == BIAS:
            assert np.array_equal(_bits(g["Rwg"].reshape(-1)), _bits(np.asarray(job["Rwg"]).reshape(-1)))
            assert np.array_equal(_bits(g["scale"]), _bits(job["scale"]))
            n[1] += 1
        if job["mode"] == GS:
            assert np.array_equal(_bits(g["bg"]), _bits(job["bg0"])) and np.array_equal(_bits(g["ba"]), _bits(job["ba0"]))
            assert np.array_equal(_bits(g["vel"]), _bits(job["vel"]))
            n[2] += 1
    assert min(n) >= 2


def test_e_degenerate_jobs(main, torch_cuda):
    jobs, got, _, want, opt = main
    # K = 1 in FULL and BIAS: only the priors act (compared with the reference under b); E = 0 in GS: untouched
    ks = [i for i, j in enumerate(jobs) if len(j["Rwb"]) == 1]
    assert {jobs[i]["mode"] for i in ks} == {FULL, BIAS, GS}
    for i in ks:
        if jobs[i]["mode"] == GS:
            assert got[i]["iterations"] == 0
            assert np.array_equal(_bits(got[i]["Rwg"].reshape(-1)), _bits(np.asarray(jobs[i]["Rwg"]).reshape(-1)))
            assert np.array_equal(_bits(got[i]["scale"]), _bits(jobs[i]["scale"]))
            assert np.array_equal(_bits(got[i]["vel"]), _bits(jobs[i]["vel"]))
        else:
            assert np.abs(got[i]["bg"] - want[i]["bg"]).max() <= 1e-7 and np.abs(got[i]["ba"] - want[i]["ba"]).max() <= 1e-7
    code, _ = opt.run([])
    assert code == _lib.OMV_OK


def test_f_nan_record(torch_cuda):
    good = cases.make(cases.MAIN[5:9])
    bad = si.make_job(65, 77, FULL, False, 1e2, 1e5)
    bad["preint"] = bad["preint"].copy()
    bad["preint"][20, 10] = np.nan
    opt = ii.InertialOptimizer(8, 256, 256)
    with_bad = ii.InertialOptimization(good[:2] + [bad] + good[2:], optimizer=opt)
    without = ii.InertialOptimization(good, optimizer=opt)
    g = with_bad[2]
    r = ref.optimize(bad)
    assert (g["iterations"], g["trials"]) == (r["iterations"], r["trials"]) == (200, 200)
    assert np.array_equal(_bits(g["vel"]), _bits(bad["vel"])) and np.array_equal(_bits(g["bg"]), _bits(bad["bg0"]))
    assert np.array_equal(_bits(g["ba"]), _bits(bad["ba0"])) and np.array_equal(_bits(g["scale"]), _bits(bad["scale"]))
    assert np.array_equal(_bits(g["Rwg"].reshape(-1)), _bits(np.asarray(bad["Rwg"]).reshape(-1)))
    for a, b in zip(with_bad[:2] + with_bad[3:], without):
        for k in OUT + ("vel_f32", "reintegrate"):
            assert np.array_equal(np.asarray(a[k]).tobytes(), np.asarray(b[k]).tobytes()), k
        assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])


def test_g_determinism(main):
    jobs, got, dbg, _, opt = main
    again = ii.InertialOptimization(jobs, optimizer=opt)
    for i, (a, b) in enumerate(zip(got, again)):
        for k in OUT + ("vel_f32", "reintegrate"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (i, k)
        assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])
        d = opt.debug(i)
        for k in ("e0", "Hvv", "Hvoff", "border", "bv", "corner", "bc", "xv", "xc"):
            assert d[k].tobytes() == dbg[i][k].tobytes(), (i, k)
        assert d["chi2"] == dbg[i]["chi2"] or (np.isnan(d["chi2"]) and np.isnan(dbg[i]["chi2"]))


def test_h_argument_errors(torch_cuda):
    lib = _lib.load()
    opt = ii.InertialOptimizer(2, 8, 8)
    jobs = [si.make_job(4, 1, FULL, False, 1e2, 1e5), si.make_job(3, 2, BIAS, False, 1.0, 1e5)]
    a, _, _ = opt.pack(jobs)
    o = dict(Rwg=a["Rwg"].copy(), scale=a["scale"].copy(), bg=np.zeros((2, 3)), ba=np.zeros((2, 3)), vel=np.zeros((7, 3)),
             vel_f32=np.zeros((7, 3), np.float32), reintegrate=np.zeros(7, np.uint8), iterations=np.zeros(2, np.int32),
             trials=np.zeros(2, np.int32))

    def call(n_jobs=2, **kw):
        args = {**a, **o, **kw}
        order = opt._IN + tuple(o.keys())
        return lib.omv_inertial_optimization(opt._h, n_jobs, *[_lib.ptr(args[k]) if args[k] is not None else None for k in order],
                                             opt._stream())

    assert call() == _lib.OMV_OK
    E = _lib.OMV_ERR_ARG
    assert call(n_jobs=-1) == E and call(n_jobs=3) == E
    assert call(kf_start=np.array([0, 4, 3], np.int32)) == E            # a descending start array
    assert call(edge_start=np.array([0, 3, 2], np.int32)) == E
    assert call(kf_start=np.array([1, 4, 7], np.int32)) == E
    assert call(mode=np.array([0, 3], np.int32)) == E                   # an unknown mode
    assert call(kf_start=np.array([0, 4, 9], np.int32)) == E            # more keyframes than the handle holds
    assert call(edge_start=np.array([0, 3, 9], np.int32)) == E
    assert call(Rwb=None) == E and call(preint=None) == E and call(bg=None) == E and call(kf_start=None) == E
    assert call(kf1=np.array([0, 0, 2, 0, 1], np.int32)) == E           # keyframe 0 with two successors
    assert call(kf1=np.array([0, 1, 3, 0, 1], np.int32), kf2=np.array([1, 2, 2, 1, 2], np.int32)) == E   # two predecessors
    assert call(kf1=np.array([0, 1, 2, 0, 1], np.int32), kf2=np.array([1, 2, 0, 1, 2], np.int32)) == E   # a cycle
    assert call(kf2=np.array([1, 2, 4, 1, 2], np.int32)) == E           # an index outside the job
    big = ii.InertialOptimizer(1, ii.MAX_KF + 1, 4)
    K = ii.MAX_KF + 1
    st = lib.omv_inertial_optimization(
        big._h, 1, _lib.ptr(np.array([0, K], np.int32)), _lib.ptr(np.array([0, 0], np.int32)),
        _lib.ptr(np.tile(np.eye(3).reshape(9), (K, 1))), _lib.ptr(np.zeros((K, 3))), _lib.ptr(np.zeros((K, 3))),
        _lib.ptr(np.zeros((K, 3), np.float32)), None, None, None, _lib.ptr(np.zeros(3)), _lib.ptr(np.zeros(3)),
        _lib.ptr(np.zeros(1, np.int32)), _lib.ptr(np.zeros(1, np.int32)), _lib.ptr(np.zeros(1, np.float32)),
        _lib.ptr(np.zeros(1, np.float32)), _lib.ptr(np.eye(3).reshape(9).copy()), _lib.ptr(np.ones(1)),
        _lib.ptr(np.zeros(3)), _lib.ptr(np.zeros(3)), _lib.ptr(np.zeros((K, 3))), _lib.ptr(np.zeros((K, 3), np.float32)),
        _lib.ptr(np.zeros(K, np.uint8)), _lib.ptr(np.zeros(1, np.int32)), _lib.ptr(np.zeros(1, np.int32)), big._stream())
    assert st == E                                                       # more than OMV_INERTIAL_MAX_KF in one job
    h = ctypes.c_void_p()
    for args in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.omv_inertial_opt_create(*args, ctypes.byref(h)) == E
    assert lib.omv_inertial_opt_create(1, 8, 8, None) == E
    assert lib.omv_inertial_opt_debug(opt._h, 2, *[None] * 16, opt._stream()) == E
    assert lib.omv_inertial_opt_debug(opt._h, -1, *[None] * 16, opt._stream()) == E


def _write_job(path, job):
    K, E = len(job["Rwb"]), len(job["kf1"])
    with open(path, "wb") as f:
        f.write(struct.pack("<4i2f", K, E, int(job["mode"]), int(job["mono"]), float(job["priorG"]), float(job["priorA"])))
        for k, dt in (("bg0", "<f8"), ("ba0", "<f8"), ("Rwg", "<f8"), ("scale", "<f8"), ("Rwb", "<f8"), ("twb", "<f8"),
                      ("vel", "<f8"), ("old_bg", "<f4"), ("kf1", "<i4"), ("kf2", "<i4"), ("preint", "<f4")):
            f.write(np.ascontiguousarray(np.asarray(job[k], dt)).tobytes())


def test_i_chain(torch_cuda, oracle, tmp_path):
    """IMU samples -> device PreintegratedBatch -> initial_guess -> InertialOptimization (FULL, stereo) on 20 jobs; the
    flagged records re-integrated on the device against oracle.preintegrate with the new bias; the C++ consumer."""
    torch = torch_cuda
    jobs = cases.chain_jobs()
    dev_jobs, batches = [], []
    for job in jobs:
        E = len(job["kf1"])
        pre = imu.PreintegratedBatch(E, job["calib"]).Initialize(job["bias"])
        meas = torch.as_tensor(job["meas"], device="cuda")
        pre.IntegrateNewMeasurements(meas, torch.as_tensor(job["start"], device="cuda"))
        torch.cuda.synchronize()
        j = dict(job)
        j["preint"] = pre.rec.cpu().numpy()
        assert np.array_equal(j["preint"].view(np.uint32), job["preint"].view(np.uint32))   # the oracle's records
        g = ii.initial_guess(j)
        j["vel"], j["Rwg"], j["scale"] = g["vel"], g["Rwg"].reshape(9), 1.0
        dev_jobs.append(j)
        batches.append((pre, meas))
    got = ii.InertialOptimization(dev_jobs, mode=FULL, mono=False, priorG=1e2, priorA=1e5)
    want = [ref.optimize(j, "literal", "dense") for j in dev_jobs]
    _compare(dev_jobs, got, want, "chain")
    n_re = 0
    for job, g, (pre, meas) in zip(dev_jobs, got, batches):
        # a record is re-integrated when its keyframe (kf2) is flagged
        recs = np.nonzero(g["reintegrate"][np.asarray(job["kf2"], np.int64)])[0]
        if not len(recs):
            continue
        bias = np.concatenate([g["ba"], g["bg"]]).astype(np.float32)
        sub = ii.reintegrate(pre, recs, bias, meas, job["start"])
        torch.cuda.synchronize()
        b = dict(meas=np.concatenate([job["meas"][job["start"][r]:job["start"][r + 1]] for r in recs]),
                 start=np.concatenate([[0], np.cumsum([job["start"][r + 1] - job["start"][r] for r in recs])]).astype(np.int32),
                 bias=np.tile(bias, (len(recs), 1)))
        rec, _ = oracle.preintegrate(b, job["calib"].Cov, job["calib"].CovWalk)
        assert np.array_equal(sub.rec.cpu().numpy().view(np.uint32), rec.view(np.uint32))
        assert np.array_equal(pre.rec.cpu().numpy()[recs].view(np.uint32), rec.view(np.uint32))
        n_re += len(recs)
    assert n_re > 0
    # the C++ consumer prints the Python call's outputs bit for bit
    exe = omv_build.build_consumer(False, omv_build.INERTIAL_CONSUMER_SRC, omv_build.INERTIAL_CONSUMER_BIN)
    assert os.path.exists(exe)
    for i in (0, 5):
        path = str(tmp_path / f"job{i}.bin")
        _write_job(path, dev_jobs[i])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        g = got[i]
        tok = r.stdout.split()
        K = len(dev_jobs[i]["Rwb"])
        want_line = (["it", str(g["iterations"]), "tr", str(g["trials"]), "Rwg"] + ["%.17g" % v for v in g["Rwg"].reshape(-1)]
                     + ["scale", "%.17g" % g["scale"], "bg"] + ["%.17g" % v for v in g["bg"]] + ["ba"]
                     + ["%.17g" % v for v in g["ba"]] + ["vel"] + ["%.17g" % v for v in g["vel"].reshape(-1)] + ["velf"]
                     + ["%.9g" % v for v in g["vel_f32"].reshape(-1)] + ["re", "".join(str(int(v)) for v in g["reintegrate"])])
        assert len(tok) == len(want_line) and tok == want_line, (i, K)
    print(f"[inertial i] {len(jobs)} jobs, {n_re} records re-integrated")
