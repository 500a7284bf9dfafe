"""GPU parity of the LocalInertialBA inner loop (openmavis_amd/csrc/lba.hip) against the CPU oracle
(oracle/ba_oracle.cpp).

Bar (north star: 1e-5 relative for floating point):
  residuals            |gpu - oracle| <= 1e-9 px / 1e-9 (IMU)   (same formulas; f64 libm ulps only)
  Jacobians            relative 1e-9
  LM outcome           identical iteration / trial counts and status; err, err_end within 1e-5 relative
  final state          poses / velocities / biases within 1e-5 relative of the oracle's step
                       (|gpu - oracle| <= 1e-5 * max(|oracle - initial|, 1e-3)); points in their
                       information metric (see _compare_state)
  per-edge chi2        whitened residuals within 1e-3 (see _chi2_tol)
  outlier flags        identical except edges whose chi2 sits within that tolerance of a threshold
"""
import numpy as np
import pytest

from openmavis_amd import synth_ba
from openmavis_amd.optimizer import LocalInertialBA

pytestmark = pytest.mark.gpu

STATE = ("Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba", "pts")


@pytest.fixture(scope="module")
def small():
    return synth_ba.make_lba_problem(n_kf=20, n_opt=10, n_pts=1500, seed=11)


@pytest.fixture(scope="module")
def full():
    return synth_ba.make_lba_problem()   # 50 keyframes (25 optimisable), 5 cameras, 20k points


def _solver(prob):
    return LocalInertialBA(max_kf=prob["n_kf"], max_cams=prob["n_cams"], max_pts=len(prob["pts"]),
                           max_mono=len(prob["mono_pt"]) + int(prob.get("n_stereo", 0)),
                           max_imu=max(1, len(prob["imu_kf1"])))


def _compare_state(prob, st_g, st_o, oracle, rel=1e-5):
    for k in STATE[:-1]:
        a, b, init = st_g[k], st_o[k], np.asarray(prob[k], np.float64).reshape(st_o[k].shape)
        step = np.abs(b - init).max()
        err = np.abs(a - b).max()
        assert err <= rel * max(step, 1e-3), (k, err, step)
    # Points: a landmark's depth along weakly-observed rays is ill-conditioned, and the float-cast
    # projection quantises chi2, so rounding-level differences move such a point along its weak
    # direction.  Compare in the landmark's own information metric (what the residuals see):
    # sqrt(dX^T Hll dX) with Hll = sum_e w JX^T JX at the oracle's final state, <= 1e-3 (whitened px);
    # in plain coordinates 99 % of the points within 1e-3 of their own step and all within 1e-2 (the
    # residual quantum of the float-cast projection, ~3e-5 px, over a weak direction's singular
    # value: measured median ~2e-7, p90 ~1e-5, p99 ~1e-4, max 3e-3; atomics make it vary run to run).
    d = st_g["pts"] - st_o["pts"]
    fin = dict(prob, **st_o)
    jx = oracle.lba_evaluate(fin)["mono_jx"].reshape(-1, 2, 3)
    w = np.asarray(prob["mono_inv_sigma2"], np.float64)
    H = np.zeros((len(d), 3, 3))
    np.add.at(H, prob["mono_pt"], w[:, None, None] * np.einsum("eri,erj->eij", jx, jx))
    if prob.get("n_stereo", 0):
        sx = oracle.lba_evaluate(fin)["stereo_jx"].reshape(-1, 3, 3)
        ws = np.asarray(prob["stereo_inv_sigma2"], np.float64)
        np.add.at(H, prob["stereo_pt"], ws[:, None, None] * np.einsum("eri,erj->eij", sx, sx))
    maha = np.sqrt(np.maximum(np.einsum("pi,pij,pj->p", d, H, d), 0))
    assert maha.max() <= 1e-3, (maha.max(), int(np.argmax(maha)))
    step = np.abs(st_o["pts"] - np.asarray(prob["pts"])).max(axis=1)
    r = np.abs(d).max(axis=1) / np.maximum(step, 1e-2)
    assert np.quantile(r, 0.99) <= 1e-3 and r.max() <= 1e-2, (r.max(), np.quantile(r, [0.5, 0.9, 0.99]))


def _compare_result(prob, rg, ro):
    assert rg["iterations"] == ro["iterations"] and rg["trials"] == ro["trials"], (rg, ro)
    assert rg["status"] == ro["status"]
    for k in ("err", "err_end"):
        assert abs(rg[k] - ro[k]) <= 1e-5 * abs(ro[k]), (k, rg[k], ro[k])
    c = ro["mono_chi2"]
    tol = _chi2_tol(c)
    bad = np.abs(rg["mono_chi2"] - c) > tol
    assert not bad.any(), (int(bad.sum()), rg["mono_chi2"][bad][:5], c[bad][:5])
    diff = rg["mono_outlier"] != ro["mono_outlier"]
    if diff.any():
        near = np.minimum(np.abs(c - 5.991), np.abs(c - 1.5 * 5.991)) <= tol
        assert near[diff].all(), (int(diff.sum()), c[diff & ~near][:5])
    if len(ro.get("stereo_chi2", ())):
        c = ro["stereo_chi2"]
        tol = _chi2_tol(c)
        bad = np.abs(rg["stereo_chi2"] - c) > tol
        assert not bad.any(), (int(bad.sum()), rg["stereo_chi2"][bad][:5], c[bad][:5])
        diff = rg["stereo_outlier"] != ro["stereo_outlier"]
        assert (np.abs(c[diff] - 7.815) <= tol[diff]).all()


def _chi2_tol(chi2):
    """Per-edge chi2 tolerance: the whitened residual sqrt(w) e may differ by <= 1e-3 (the bar of the
    point check in _compare_state; weakly observed points move along their weak direction, and
    KannalaBrandt8::project's float cast (KannalaBrandt8.cpp:30-31) quantises e by ~3e-5 px), so
    |d chi2| <= 2 sqrt(chi2) 1e-3 + 1e-6, plus 1e-6 relative."""
    return 1e-6 * chi2 + 2e-3 * np.sqrt(chi2) + 1e-6


def test_residuals_and_jacobians(small, oracle):
    ba = _solver(small).set_problem(small)
    g = ba.evaluate()
    o = oracle.lba_evaluate(small)
    assert np.abs(g["mono_err"] - o["mono_err"]).max() <= 1e-9
    assert np.abs(g["imu_err"] - o["imu_err"]).max() <= 1e-9
    for k in ("mono_jx", "mono_jp"):
        scale = np.abs(o[k]).max()
        assert np.abs(g[k] - o[k]).max() <= 1e-9 * scale, k


@pytest.mark.parametrize("large", [True, False])
def test_optimize_small(small, oracle, large):
    kw = dict(opt_it=4, lambda_init=1e-2) if large else dict(opt_it=10, lambda_init=1e0)
    ro, so, _ = oracle.lba_optimize(small, max_trials=10, large=large, **kw)
    rg, sg = _solver(small).set_problem(small).optimize(max_trials=10, large=large, **kw)
    _compare_result(small, rg, ro)
    _compare_state(small, sg, so, oracle)


@pytest.fixture(scope="module")
def small_pinhole():
    return synth_ba.make_lba_problem(n_kf=20, n_opt=10, n_pts=1500, seed=12, pinhole=True)


def test_pinhole_residuals_and_jacobians(small_pinhole, oracle):
    """A Pinhole rig (configs[3]'s camera model): Pinhole::project / projectJac in EdgeMono."""
    test_residuals_and_jacobians(small_pinhole, oracle)


@pytest.mark.parametrize("large", [True, False])
def test_optimize_small_pinhole(small_pinhole, oracle, large):
    test_optimize_small(small_pinhole, oracle, large)


@pytest.fixture(scope="module")
def small_st():
    return synth_ba.make_lba_problem(n_kf=20, n_opt=10, n_pts=1500, seed=11, stereo_frac=0.5)


def test_stereo_residuals_and_jacobians(small_st, oracle):
    """EdgeStereo (G2oTypes.cc:402-431) on the device vs the oracle: same bar as EdgeMono."""
    g = _solver(small_st).set_problem(small_st).evaluate()
    o = oracle.lba_evaluate(small_st)
    assert small_st["n_stereo"] > 500
    assert np.abs(g["stereo_err"] - o["stereo_err"]).max() <= 1e-9
    assert np.abs(g["mono_err"] - o["mono_err"]).max() <= 1e-9
    for k in ("stereo_jx", "stereo_jp", "mono_jx", "mono_jp"):
        assert np.abs(g[k] - o[k]).max() <= 1e-9 * np.abs(o[k]).max(), k


@pytest.mark.parametrize("large", [True, False])
def test_optimize_with_stereo_edges(small_st, oracle, large):
    kw = dict(opt_it=4, lambda_init=1e-2) if large else dict(opt_it=10, lambda_init=1e0)
    ro, so, _ = oracle.lba_optimize(small_st, max_trials=10, large=large, **kw)
    rg, sg = _solver(small_st).set_problem(small_st).optimize(max_trials=10, large=large, **kw)
    _compare_result(small_st, rg, ro)
    _compare_state(small_st, sg, so, oracle)


def test_optimize_visual_only_with_fixed_only_points(oracle):
    """No inertial edges (kf_imu off), 6-dof pose blocks only; some points seen only by fixed keyframes."""
    prob = synth_ba.visual_only_with_fixed_only_points(   # points 0..19: fixed views only
        synth_ba.make_lba_problem(n_kf=12, n_opt=4, n_pts=800, seed=3, n_cams=3))
    ro, so, _ = oracle.lba_optimize(prob, opt_it=10, lambda_init=1e0, max_trials=10, large=False)
    rg, sg = _solver(prob).set_problem(prob).optimize(opt_it=10, lambda_init=1e0, max_trials=10, large=False)
    _compare_result(prob, rg, ro)
    _compare_state(prob, sg, so, oracle)


def test_optimize_with_edgeless_points(small, oracle):
    """More than one build group's worth (> 256) of landmarks without edges, interleaved with observed ones: each
    still gets its (zero) Hll / bl, so the back-substitution and computeScale see no stale values."""
    n0, prob = len(small["pts"]), synth_ba.with_edgeless_points(small, extra=700)
    for large in (True, False):
        kw = dict(opt_it=4, lambda_init=1e-2) if large else dict(opt_it=10, lambda_init=1e0)
        ro, so, _ = oracle.lba_optimize(prob, max_trials=10, large=large, **kw)
        rg, sg = _solver(prob).set_problem(prob).optimize(max_trials=10, large=large, **kw)
        _compare_result(prob, rg, ro)
        _compare_state(prob, sg, so, oracle)
        assert np.array_equal(sg["pts"][n0:], np.asarray(prob["pts"], np.float64)[n0:])


def test_optimize_with_heavy_landmark(small, oracle):
    """A landmark with more edges than a build group holds (> 256: its observations repeated 60x with noise) goes to the
    scalar one-landmark path (build_big_kernel) beside the MFMA groups; same bar against the oracle."""
    prob = synth_ba.with_heavy_landmark(small, times=60)
    assert len(prob["mono_pt"]) - len(small["mono_pt"]) > 256
    for large in (True, False):
        kw = dict(opt_it=4, lambda_init=1e-2) if large else dict(opt_it=10, lambda_init=1e0)
        ro, so, _ = oracle.lba_optimize(prob, max_trials=10, large=large, **kw)
        rg, sg = _solver(prob).set_problem(prob).optimize(max_trials=10, large=large, **kw)
        _compare_result(prob, rg, ro)
        _compare_state(prob, sg, so, oracle)


def test_optimize_full_window(full, full_oracle, oracle):
    """The bench configuration: 25 optimisable + 25 fixed keyframes, 5 cameras, 20k points, 120k edges."""
    ro, so = full_oracle
    ba = _solver(full).set_problem(full)
    rg, sg = ba.optimize(opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    _compare_result(full, rg, ro)
    _compare_state(full, sg, so, oracle)
    assert rg["err_end"] < 1e-3 * rg["err"]
    t = ba.stage_ms()
    assert t["trials"] == rg["trials"]


@pytest.mark.parametrize("large", [True, False])
def test_device_lm_driver_matches_host_driver(small, oracle, large):
    """The device-resident LM control (one captured hipGraph per trial, one read-back per optimize) makes the
    host loop's decisions: same iterations / trials / status, err / err_end and state at the parity bar; the
    per-stage timing mode (direct launches) as well."""
    kw = dict(opt_it=10 if not large else 4, lambda_init=1e0 if not large else 1e-2, max_trials=10, large=large)
    ba = _solver(small).set_problem(small)
    rh, sh = ba.set_driver(True).optimize(**kw)
    rd, sd = ba.set_problem(small).set_driver(False).optimize(**kw)
    rt, st = ba.set_problem(small).enable_timing(True).optimize(**kw)
    ro, so, _ = oracle.lba_optimize(small, **kw)
    for r, s in ((rd, sd), (rt, st)):
        assert (r["iterations"], r["trials"], r["status"]) == (rh["iterations"], rh["trials"], rh["status"])
        for k in ("err", "err_end"):
            assert abs(r[k] - rh[k]) <= 1e-6 * abs(rh[k]), (k, r[k], rh[k])
        _compare_result(small, r, ro)
        _compare_state(small, s, so, oracle)
    t = ba.stage_ms()
    assert t["trials"] == rt["trials"] and t["solve"] > 0


@pytest.mark.parametrize("large", [True, False])
def test_device_driver_with_rejected_trials(small, oracle, large):
    """lambda_init 1e-9 makes half the trials fail (oracle: 6 iterations, 12 trials): the device driver's
    double-buffered state keeps the current state and its errors through each rejected trial, reports the last
    computed errors' chi (a rejected trial's, as g2o does) and matches the host driver and the oracle -- decisions
    exactly, err / err_end and the state at the parity bar -- in the graph and in the direct-launch mode."""
    kw = dict(opt_it=6, lambda_init=1e-9, max_trials=10, large=large)
    ro, so, _ = oracle.lba_optimize(small, **kw)
    assert ro["trials"] > ro["iterations"], ro   # the case exercises rejections
    ba = _solver(small).set_problem(small)
    rh, sh = ba.set_driver(True).optimize(**kw)
    rd, sd = ba.set_problem(small).set_driver(False).optimize(**kw)
    rt, st = ba.set_problem(small).enable_timing(True).optimize(**kw)
    for r, s in ((rd, sd), (rt, st)):
        assert (r["iterations"], r["trials"], r["status"]) == (rh["iterations"], rh["trials"], rh["status"])
        for k in ("err", "err_end"):
            assert abs(r[k] - rh[k]) <= 1e-6 * abs(rh[k]), (k, r[k], rh[k])
        _compare_result(small, r, ro)
        _compare_state(small, s, so, oracle)


def test_reoptimize_same_handle(small, oracle):
    """set_problem twice on one handle (workspace reuse) gives the same answer."""
    ba = _solver(small)
    r1, s1 = ba.set_problem(small).optimize(opt_it=4, lambda_init=1e-2, large=True)
    r2, s2 = ba.set_problem(small).optimize(opt_it=4, lambda_init=1e-2, large=True)
    assert r1["trials"] == r2["trials"]
    _compare_state(small, s2, s1, oracle)


@pytest.mark.parametrize("driver", ["device", "host"])
def test_bitwise_identical_run_to_run(full, driver):
    """Every device reduction is a fixed-order sum (no float atomics): two solves of the bench window — on
    fresh handles and on one reused handle — give bit-identical state, chi2, err / err_end and lambda."""
    kw = dict(opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    runs = []
    ba = _solver(full).set_driver(driver == "host")
    for h in (ba, ba, _solver(full).set_driver(driver == "host")):
        r, s = h.set_problem(full).optimize(**kw)
        runs.append((r, s))
    r0, s0 = runs[0]
    for r, s in runs[1:]:
        for k in ("err", "err_end", "lambda_", "iterations", "trials", "status"):
            assert r[k] == r0[k], (k, r[k], r0[k])
        assert np.array_equal(r["mono_chi2"].view(np.uint64), r0["mono_chi2"].view(np.uint64))
        for k in STATE:
            assert np.array_equal(np.asarray(s[k]).view(np.uint64), np.asarray(s0[k]).view(np.uint64)), k


def _run_shard(tmp_path, backend, driver, world, n_kf, n_opt, n_pts, seed):
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / f"shard_{backend}_{world}.npz"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "tools", "lba_shard_run.py"),
           "--out", str(out), "--backend", backend, "--n-kf", str(n_kf), "--n-opt", str(n_opt), "--n-pts", str(n_pts),
           "--seed", str(seed), "--host-driver", "1" if driver == "host" else "0"]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return dict(np.load(out))


def _check_shard(g, prob, ro, so, oracle, world, driver):
    assert int(g["world"]) == world and (g["owner"] >= 0).all() and len(set(g["owner"].tolist())) == world
    rg = {k: (g[k].item() if g[k].ndim == 0 else g[k]) for k in
          ("err", "err_end", "status", "iterations", "trials", "mono_chi2", "mono_outlier")}
    _compare_result(prob, rg, ro)
    _compare_state(prob, {k: g[k] for k in STATE}, so, oracle)
    trials, syncs = int(g["trials"]), int(g["host_syncs"])
    assert int(g["ar_calls"]) >= 2 * trials, (int(g["ar_calls"]), trials)   # the collectives really ran
    if driver == "device":
        assert syncs <= (trials + 3) // 4 + 1 and (trials < 2 or syncs < trials), (syncs, trials)
    else:
        assert syncs >= trials, (syncs, trials)


@pytest.mark.parametrize("backend,driver,world", [("gloo", "device", 2), ("gloo", "host", 2), ("gloo", "device", 4),
                                                  ("nccl", "device", 1), ("nccl", "device", 2)])
def test_landmark_sharded_ranks(oracle, tmp_path, backend, driver, world):
    """landmarks sharded over `world` ranks, one all-reduce of the partial Schur system and one of the LM
    scalars per step.  gloo: the ranks share this box's GPU, collectives through host memory (2 and 4 ranks).  nccl:
    RCCL on the handle's device buffer in place (LbaAllReduce "device") -- one rank on a one-GPU box runs the same
    call sequence, more ranks need as many GPUs.  The merged outcome meets the same bar against the oracle, and every
    rank holds the identical keyframe state (asserted inside the worker).  The device LM driver waits on the host
    once per batch of steps, never per trial (omv_lba_host_syncs)."""
    import torch
    if backend == "nccl" and torch.cuda.device_count() < world:
        pytest.skip(f"RCCL over {world} ranks needs {world} visible GPUs (one rank and the gloo cases run on one)")
    g = _run_shard(tmp_path, backend, driver, world, 20, 10, 3000, 11)
    prob = synth_ba.make_lba_problem(n_kf=20, n_opt=10, n_pts=3000, seed=11)
    ro, so, _ = oracle.lba_optimize(prob, opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    _check_shard(g, prob, ro, so, oracle, world, driver)


@pytest.fixture(scope="module")
def full_oracle(full, oracle):
    ro, so, _ = oracle.lba_optimize(full, opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    return ro, so


@pytest.mark.parametrize("world", [2, 4])
def test_landmark_sharded_config5_window(oracle, full, full_oracle, tmp_path, world):
    """The sharded path at the bench's size: configs[4]'s window (50 keyframes, 25 optimisable, 5 cameras, 20k points,
    120k edges) split over 2 and 4 gloo ranks sharing this box's GPU, against the oracle's unsharded solve at the same
    bar, with the device driver's host-sync bound (once per batch of steps) asserted."""
    g = _run_shard(tmp_path, "gloo", "device", world, 50, 25, 20000, 5)
    ro, so = full_oracle
    _check_shard(g, full, ro, so, oracle, world, "device")
