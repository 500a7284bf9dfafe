"""The device MLPnPsolver (openmavis_amd/csrc/pnp.hip through openmavis_amd/pnpsolver.py) against tests/mlpnp_ref.py.

a. sampling      the six sampled correspondences (debug hook) equal the replay of the swap-with-back list, exactly
b. computePose   the linear stage (R0, t0) and the final (R, t) per hypothesis against the float64 reference on the
                 device's bearings and sampled indices: |q_gpu - q_64|_inf <= C eps64 kappa max(1, |q_64|_inf), kappa =
                 sigma_max(A^T A) / (gap of its two smallest), times cond(Jac^T Jac) for the final pose.  C_LINEAR /
                 C_FINAL are 4 x the worst ratio measured on an MI355X.  A hypothesis is left out
                 of the value comparison only if the reference shows a decision within 2^-20 of its threshold or
                 kappa > 1e8 (at most 5 % of a case; tests/test_mlpnp_ref_cpu.py holds the case lists to that on the
                 reference alone); for every other one the planar flag, the iteration count and the exit reason match.
c. CheckInliers  with the device's own pose the float64 errors decide every (hypothesis, correspondence) outside
                 [t (1 - d), t (1 + d)], d = 2^-10: the mask agrees there exactly, count is the mask's popcount, at most
                 0.1 % of the entries are inside the band; a non-finite pose has no inliers.
d. selection     from the device's own counts and Refine records the Python replay of iterate gives exactly the device's
                 flags, nInliers, mnIterations, mnBestInliers, T (bitwise) and vbInliers, over two consecutive calls
e. end to end    planted pose, 40 % outliers: iterate -> PoseOptimization on the inliers
f. argument errors and capacity (tests/test_mlpnp_handles_gpu.py has the allocation tests)

Measured on an MI355X (pytest -s prints the figures): see DESIGN.md section 6."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mlpnp_cases as cases
import mlpnp_ref as ref
from openmavis_amd import _lib, build as omv_build, pnpsolver, synth_pnp

pytestmark = pytest.mark.gpu

KB8, PIN = 0, 1
EPS = ref.EPS
C_LINEAR, C_FINAL = 290.0, 530.0   # 4 x the worst measured ratios 71.6 and 131, see DESIGN.md section 6


def _draws_for(n, idx):
    """Raw draws that make the sampling pick idx[0..5]."""
    avail, r = list(range(n)), []
    for v in idx:
        p = avail.index(v)
        r.append(p)
        avail[p] = avail[-1]
        avail.pop()
    return r


@functools.lru_cache(maxsize=None)
def _case(case):
    """One handle over the case's jobs, one iterate on its draws with parameters that let every hypothesis be
    evaluated -> (jobs, draws, solver, H)."""
    jobs, draws = cases.make(case)
    H = draws.shape[1]
    s = pnpsolver.MLPnPsolver(jobs, max_hyp=H)
    return jobs, draws, s, H


def _hyps(case):
    """hypotheses(j) of every job of the case with every hypothesis of the draws evaluated: epsilon = 1 makes
    mRansacMinInliers = N, so a hypothesis qualifies only if every correspondence is an inlier, and the call never
    returns early because Refine's count cannot be strictly greater than N.  mRansacMaxIts is then 1; nIterations = H
    still runs H hypotheses through the OR."""
    jobs, draws, s, H = _case(case)
    s.SetRansacParameters(0.99, 6, 300, 6, 1.0, 5.991)
    assert (s.min_inliers == s.n).all() and (s.max_its == 1).all()
    s.iterate(H, draws)
    out = [s.hypotheses(j) for j in range(len(jobs))]
    assert all(len(o["count"]) == H for o in out)
    return jobs, draws, out, s


_hyps = functools.lru_cache(maxsize=None)(_hyps)


# ---- a. sampling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7, 64, 65])
def test_sampling_exact(torch_cuda, n):
    rng = np.random.default_rng(n)
    special = [[n - 1, n - 2, n - 3, n - 4, n - 5, n - 6], [0] * 6, [n - 2, n - 2, n - 3, n - 4, 0, 0],
               [1, 1, 1, 1, 1, 0], [0, n - 2, 0, n - 4, 0, 0], [n - 1, 0, n - 3, 0, n - 5, 0], [2, 2, 2, 2, 0, 0],
               [99, -3, 99, -3, 99, -3]]   # the back positions, repeated draws, out-of-range draws
    if n <= 7:   # every first-two-draw pattern, with the later draws both at the front and at the back
        allr = [[a, b, c, c, min(c, n - 5), 0] for a in range(n) for b in range(n - 1) for c in (0, n - 4, n - 3)]
    else:
        allr = [[int(rng.integers(0, n - i)) for i in range(6)] for _ in range(40)]
    draws = np.array(special + allr, np.int32)
    job = synth_pnp.make_job(n, seed=5, model=PIN)
    s = pnpsolver.MLPnPsolver([job], max_hyp=len(draws))
    s.SetRansacParameters(0.99, 6, 300, 6, 1.0, 5.991)
    s.iterate(len(draws), draws[None])
    idx = s.hypotheses(0)["idx"]
    assert len(idx) == len(draws)
    for k, r in enumerate(draws):
        assert idx[k].tolist() == ref.sample_literal(n, r.tolist()) == ref.sample_replay(n, r.tolist()), (k, r)
    assert any(r[1] == r[0] for r in allr)


# ---- b. computePose ----------------------------------------------------------------------------------------------
def _case_id(c):
    return f"N{'-'.join(map(str, c[0]))}-{c[3] if isinstance(c[3], str) else 'mixed'}-{c[6]}"


@pytest.mark.parametrize("case", cases.B_CASES, ids=_case_id)
def test_compute_pose_against_float64(torch_cuda, case):
    jobs, draws, hyps, s = _hyps(case)
    worst = {"lin": 0.0, "fin": 0.0}
    for j, (job, hy) in enumerate(zip(jobs, hyps)):
        prep = hy["prepared"]
        f_ref = ref.bearings(job)
        # the bearing is float32 arithmetic: the device's and the numpy restatement's agree to a few float ulps
        assert np.abs(prep[:, :3] - f_ref).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(f_ref).max())
        assert np.array_equal(prep[:, 2], np.ones(len(prep))) and np.array_equal(prep[:, 9:], job["Xw"].astype(np.float64))
        pre = ref.prepare(job, bearing=prep[:, :3])
        ns_dev = np.stack([prep[:, 3:6], prep[:, 6:9]], 2)
        assert np.abs(ns_dev - pre["ns"]).max() <= 4 * EPS     # the Householder reflector, a handful of operations
        left_out, H = 0, len(hy["idx"])
        for h in range(H):
            idx = hy["idx"][h]
            a = ref.compute_pose(pre["f"][idx], pre["ns"][idx], pre["Xw"][idx])
            if a["near"]:
                left_out += 1
                continue
            assert hy["planar"][h] == a["planar"], (j, h)
            assert (hy["its"][h], hy["reason"][h]) == (a["its"], a["reason"]), (j, h, a["kappa_final"])
            for q, kappa, key, c in (("R0", a["kappa"], "lin", C_LINEAR), ("t0", a["kappa"], "lin", C_LINEAR),
                                     ("R", a["kappa_final"], "fin", C_FINAL), ("t", a["kappa_final"], "fin", C_FINAL)):
                e = np.abs(hy[q][h] - a[q]).max()
                bound = EPS * kappa * max(1.0, np.abs(a[q]).max())
                worst[key] = max(worst[key], e / bound)
                print(f"[mlpnp b] job {j} hyp {h} {q}: e {e:.3g} e / (eps kappa max(1, |q|)) {e / bound:.3g}")
                assert e <= c * bound, (j, h, q, e, bound, kappa)
        assert left_out <= cases.LEFT_OUT_CAP * H, (j, left_out, H)
    print(f"[mlpnp b] {_case_id(case)}: worst ratio linear {worst['lin']:.3g}, final {worst['fin']:.3g}")


def test_rank_one_scene_takes_the_twelve_column_branch(torch_cuda):
    """The pose of a rank-1 scene is not observable (tests/test_mlpnp_ref_cpu.py); the device must take the 12-column
    branch and end cleanly."""
    job = synth_pnp.make_job(30, 4, PIN, "rank1", noise_px=0.0)
    s = pnpsolver.MLPnPsolver([job], max_hyp=16)
    s.SetRansacParameters(0.99, 6, 300, 6, 1.0, 5.991)
    s.iterate(16, s.draw(np.random.default_rng(1), 16))
    hy = s.hypotheses(0)
    assert len(hy["planar"]) == 16 and not hy["planar"].any()


# ---- c. CheckInliers ---------------------------------------------------------------------------------------------
def _band_check(job, pre, rec):
    """(entries, entries in the band, mismatches outside the band) for the poses of a hook record."""
    n_band = n_bad = 0
    for h in range(len(rec["count"])):
        assert rec["count"][h] == rec["mask"][h].sum() == sum(bin(int(w)).count("1") for w in rec["words"][h])
        if not (np.isfinite(rec["R"][h]).all() and np.isfinite(rec["t"][h]).all()):
            assert rec["count"][h] == 0
            continue
        with np.errstate(all="ignore"):
            e = ref.reprojection_errors(job, pre, rec["R"][h], rec["t"][h])
            band = np.abs(e - pre["max_err"]) <= cases.DELTA * pre["max_err"]
            inl = e < pre["max_err"]
        n_band += int(band.sum())
        n_bad += int(((inl != rec["mask"][h]) & ~band).sum())
    return rec["mask"].size, n_band, n_bad


@pytest.mark.parametrize("case", cases.C_CASES, ids=_case_id)
def test_check_inliers_with_device_poses(torch_cuda, case):
    jobs, draws, hyps, s = _hyps(case)
    tot = band = 0
    for job, hy in zip(jobs, hyps):
        pre = ref.prepare(job)
        assert np.array_equal(pre["max_err"], (job["sigma2"] * np.float32(5.991)).astype(np.float64))
        n, nb, bad = _band_check(job, pre, hy)
        assert bad == 0, (len(job["index"]), bad)
        tot, band = tot + n, band + nb
        assert hy["mask"].any()
    assert len({float(x) for job in jobs for x in job["sigma2"]}) == 8   # octaves 0-7
    print(f"[mlpnp c] {_case_id(case)}: {band} of {tot} entries in the band ({band / tot:.4%})")
    assert band <= cases.BAND_CAP * tot


def test_non_finite_pose_has_no_inliers(torch_cuda):
    """Tcw = I, noise-free: where the linear stage returns a rotation whose trace is >= 3, rot2rodrigues gives w == 0
    exactly, the Jacobian divides by zero as the reference's does (:797), the pose is non-finite and nothing is an
    inlier; the call returns OMV_OK."""
    job = synth_pnp.make_job(20, 6, PIN, "identity", noise_px=0.0)
    s = pnpsolver.MLPnPsolver([job], max_hyp=64)
    s.SetRansacParameters(0.99, 6, 300, 6, 1.0, 5.991)
    found, T, no_more, vb, n_inl = s.iterate(64, s.draw(np.random.default_rng(1), 64))
    hy = s.hypotheses(0)
    bad = ~np.isfinite(hy["t"]).all(1)
    print(f"[mlpnp c] identity pose: {int(bad.sum())} of {len(bad)} hypotheses end non-finite")
    assert bad.any() and (hy["count"][bad] == 0).all() and not hy["mask"][bad].any()
    assert (hy["reason"][bad] == pnpsolver.GN_NAN).all()
    good = np.isfinite(hy["t"]).all(1) & (hy["reason"] == pnpsolver.GN_EPSP)
    assert (hy["count"][good] == 20).all()


# ---- d. selection --------------------------------------------------------------------------------------------------
def _replay_calls(s, jobs, calls, params):
    """Run the iterate calls [(nIterations, draws)] and replay each from the device's counts and Refine records."""
    s.SetRansacParameters(*params)
    J = len(jobs)
    st = [ref.new_state() for _ in jobs]
    T_ref = [None] * J     # the kept Refine outcome
    T_best = [None] * J
    m_ref, m_best = [None] * J, [None] * J
    log = []
    for n_it, draws in calls:
        found, T, no_more, vb, n_inl = s.iterate(n_it, draws)
        found, T, no_more, n_inl = found.cpu().numpy(), T.cpu().numpy(), no_more.cpu().numpy(), n_inl.cpu().numpy()
        for j, job in enumerate(jobs):
            hy = s.hypotheses(j)
            rec = hy["refine"]
            k = [0]

            def refine(h):
                assert k[0] < len(rec["hyp"]) and rec["hyp"][k[0]] == h, (j, h, rec["hyp"])
                assert rec["n_in"][k[0]] == hy["count"][h] and rec["ok"][k[0]] == (rec["count"][k[0]] > s.min_inliers[j])
                T_ref[j], m_ref[j] = ref.pose32(rec["R"][k[0]], rec["t"][k[0]]), rec["mask"][k[0]]
                k[0] += 1
                return int(rec["count"][k[0] - 1]), bool(rec["ok"][k[0] - 1])

            out = ref.replay_call(st[j], hy["count"], refine, n_it, draws.shape[1], len(job["index"]),
                                  int(s.min_inliers[j]), int(s.max_its[j]))
            assert k[0] == len(rec["hyp"]) and out["done"] == len(hy["count"]), (j, out, len(hy["count"]))
            if out["bests"]:
                b = out["bests"][-1]
                T_best[j], m_best[j] = ref.pose32(hy["R"][b], hy["t"][b]), hy["mask"][b]
            flags = int(no_more[j]) * ref.NO_MORE + int(found[j]) * ref.FOUND
            assert flags == out["flags"], (j, flags, out)
            assert n_inl[j] == out["n_inliers"]
            T_exp = T_ref[j] if out["kind"] == 1 else (T_best[j] if out["kind"] == 2 else np.eye(4, dtype=np.float32))
            assert T[j].tobytes() == np.ascontiguousarray(T_exp).tobytes(), (j, out)
            vb_exp = np.zeros(job["mN"], bool)
            if out["kind"]:
                vb_exp[job["index"][m_ref[j] if out["kind"] == 1 else m_best[j]]] = True
            assert np.array_equal(s.job_inliers(j), vb_exp), (j, out)
            assert (hy["state"]["iterations"], hy["state"]["best"]) == (st[j]["iterations"], st[j]["best"])
            assert hy["state"]["out_kind"] == out["kind"]
            log.append((j, out, [(int(h), int(c), bool(o)) for h, c, o in zip(rec["hyp"], rec["count"], rec["ok"])]))
    return log, st


def test_selection_replay_two_calls_mixed_jobs(torch_cuda):
    """Mixed-size jobs in one handle under Tracking's parameters: the first iterate(5) runs the whole RANSAC (the OR),
    a second call goes on.  N = 7 has N < mRansacMinInliers (bNoMore, no work)."""
    ns = [130, 65, 7, 64, 63]
    jobs = synth_pnp.make_jobs(ns, seed=31, models=[PIN, KB8, PIN, KB8, PIN], scenes="centred", noise_px=0.5,
                               outlier_share=0.3, depth=(2.0, 6.0))
    s = pnpsolver.MLPnPsolver(jobs, max_hyp=64)
    rng = np.random.default_rng(32)
    calls = [(5, s.draw(rng, 64)), (5, s.draw(rng, 64))]
    log, st = _replay_calls(s, jobs, calls, ref.TRACKING)
    assert s.max_its.tolist() == [ref.ransac_parameters(n, *ref.TRACKING[:5])[0] for n in ns]
    assert s.min_inliers.tolist() == [65, 32, 10, 32, 31]
    by_job = {j: [o for jj, o, _ in log if jj == j] for j in range(len(ns))}
    assert all(o["flags"] == ref.NO_MORE and o["done"] == 0 for o in by_job[2])
    assert any(o["flags"] & ref.FOUND for j in (0, 1, 3, 4) for o in by_job[j])
    for j in (0, 1, 3, 4):   # the second call consumed at least one hypothesis and at most five once exhausted
        assert by_job[j][1]["done"] >= 1


def _two_pose_job(seed, model):
    """A job of 64 with 40 % outliers in which eight of the outliers agree with a second pose (the first one turned by
    0.2 rad and moved), to 0.05 px: a sample of six of them has exactly those eight as inliers."""
    from openmavis_amd.synth_sim3 import _rot
    job = synth_pnp.make_job(64, seed, model, "centred", noise_px=0.5, outlier_share=0.4, depth=(2.0, 6.0))
    rng = np.random.default_rng(seed + 1000)
    second = np.nonzero(~job["inlier"])[0][:8]
    RB, tB = _rot(rng, 0.2) @ job["Rcw"], job["tcw"] + np.array([0.3, -0.2, 0.1])
    P = synth_pnp.project(model, job["cam"], job["Xw"][second].astype(np.float64) @ RB.T + tB)
    job["P2D"][second] = (P + rng.normal(0, 0.05, P.shape)).astype(np.float32)
    job["second"] = second
    return job


def test_selection_refine_fails_then_succeeds_and_exhaustion(torch_cuda):
    """mRansacMinInliers = 8.  A sample from the eight correspondences of the second pose has count 8: it qualifies
    (>=) and becomes the best, and its Refine, over those eight, ends with 8 inliers, which is not strictly greater:
    Refine fails.  Job 0 later meets a sample of the main pose, whose Refine succeeds; job 1 never does and ends by
    exhaustion with the unrefined best; job 2 never qualifies.  The reference rates every sample first."""
    n = 64
    jobs = [_two_pose_job(41 + j, m) for j, m in enumerate((PIN, KB8, PIN))]
    params = (0.99, 8, 12, 6, 0.1, 5.991)     # mRansacMinInliers = 8, mRansacMaxIts = 12
    rng = np.random.default_rng(42)
    rows = []
    for j, job in enumerate(jobs):
        rs = ref.RefSolver(job)
        rs.SetRansacParameters(*params)
        assert (rs.max_its, rs.min_inliers) == (12, 8)
        inl = np.nonzero(job["inlier"])[0]
        outl = np.setdiff1d(np.nonzero(~job["inlier"])[0], job["second"])
        weak = _draws_for(n, job["second"][[0, 2, 3, 5, 6, 7]])
        h = rs.hypothesis(weak)
        r = rs.refine(h["mask"])
        assert h["count"] == 8 and np.array_equal(np.nonzero(h["mask"])[0], job["second"]) and r["count"] == 8, j
        good = bad = None
        for _ in range(200):
            if good is None:
                d = _draws_for(n, rng.choice(inl, 6, replace=False))
                h = rs.hypothesis(d)
                if h["count"] > 0.5 * n and rs.refine(h["mask"])["ok"]:
                    good = d
            if bad is None:
                d = _draws_for(n, rng.choice(outl, 6, replace=False))
                if rs.hypothesis(d)["count"] <= 4:
                    bad = d
            if good is not None and bad is not None:
                break
        assert good is not None and bad is not None, j
        row = [bad] * 12
        if j == 0:
            row[2], row[7] = weak, good
        elif j == 1:
            row[3] = weak
        rows.append(row)
    draws = np.array(rows, np.int32)
    s = pnpsolver.MLPnPsolver(jobs, max_hyp=12)
    log, st = _replay_calls(s, jobs, [(5, draws), (5, draws[:, :5])], params)
    first = {j: (o, r) for j, o, r in log[:3]}
    print("[mlpnp d]", [(j, o["flags"], o["done"], r) for j, o, r in log])
    o, r = first[0]
    assert [x[2] for x in r] == [False, True] and (o["flags"], o["kind"], o["done"]) == (ref.FOUND, 1, 8)
    o, r = first[1]
    assert [x[2] for x in r] == [False] and (o["flags"], o["kind"], o["done"]) == (ref.NO_MORE | ref.FOUND, 2, 12)
    o, r = first[2]
    assert r == [] and (o["flags"], o["kind"], o["done"]) == (ref.NO_MORE, 0, 12)
    second = {j: (o, r) for j, o, r in log[3:]}
    # the kept outcome answers job 0's second call at its first qualifying hypothesis without a new Refine
    assert second[0][1] == [] and second[0][0]["kind"] == 1 and second[0][0]["done"] == 3
    assert second[1][1] == [] and second[1][0]["kind"] == 2 and second[1][0]["done"] == 5


# ---- e. end to end ---------------------------------------------------------------------------------------------------
def test_relocalization_chain_pnp_then_pose_optimization(torch_cuda):
    """synth_pose's frames (pinhole, mono edges, 40 % of the observations moved by 8-40 px): MLPnPsolver with the header's
    default parameters (epsilon 0.4: 70 hypotheses, of which one samples six inliers with probability
    1 - (1 - 0.6^6)^70 = 97 % per frame; Tracking's epsilon 0.5 leaves 35 hypotheses and 81 %, and on these seeds the
    float64 reference itself exhausts them on one frame) on every frame's matches, then Optimizer::PoseOptimization on the inliers from the solver's pose.  The
    result is within tests/test_pose_oracle_cpu.py's 0.05 deg / 1 cm of the planted pose, and no planted outlier is
    among vbInliers.  That tolerance was set on frames with 180 inlier edges over a four-camera rig, or 100 mono and
    100 stereo edges of one camera; the mono edges of a single pinhole camera constrain the pose less, so a frame here
    has 400 matches, 240 of them inliers at 0.7 px (with 200 matches, 104 to 116 inliers, the optimised poses were
    measured at 0.023 and 0.056 deg: the accuracy of the estimate from that many edges, not of the solver)."""
    import torch
    from openmavis_amd import synth_pose
    from openmavis_amd.optimizer import PoseInertialOptimizer
    F = 3
    b = synth_pose.make_pose_only_batch(n_frames=F, n_pts=400, seed=5, outlier_frac=0.4, n_cams=1)
    jobs = []
    for f in range(F):
        m0, m1 = b["mono_start"][f], b["mono_start"][f + 1]
        jobs.append(dict(P2D=b["mono_obs"][m0:m1].astype(np.float32),
                         sigma2=(np.float32(1) / b["mono_inv_sigma2"][m0:m1]).astype(np.float32),
                         Xw=b["mono_xw"][m0:m1], index=b["mono_kp"][m0:m1].astype(np.int32), mN=int(b["kp_cap"]),
                         cam=np.asarray(b["cam"][0], np.float32)[:8], model=PIN))
    s = pnpsolver.MLPnPsolver(jobs, max_hyp=300)
    s.SetRansacParameters(*ref.DEFAULTS)
    assert s.max_its.tolist() == [70] * F and s.min_inliers.tolist() == [160] * F
    found, T, no_more, vb, n_inl = s.iterate(5, s.draw(np.random.default_rng(6), 300))
    found, T, n_inl = found.cpu().numpy(), T.cpu().numpy().astype(np.float64), n_inl.cpu().numpy()
    assert found.all() and (n_inl > s.min_inliers).all()
    keep = np.zeros(len(b["mono_cam"]), bool)
    for f in range(F):
        m0, m1 = b["mono_start"][f], b["mono_start"][f + 1]
        vbj = s.job_inliers(f)
        assert vbj.sum() == n_inl[f] and not vbj[b["mono_kp"][m0:m1][b["mono_is_outlier"][m0:m1]]].any(), f
        keep[m0:m1] = vbj[b["mono_kp"][m0:m1]]
        b["pose_q"][f] = synth_pose.quat_of(T[f, :3, :3])
        b["pose_t"][f] = T[f, :3, 3]
    counts = [int(keep[b["mono_start"][f]:b["mono_start"][f + 1]].sum()) for f in range(F)]
    for k in [k for k in b if k.startswith("mono_") and k != "mono_start"]:
        b[k] = np.ascontiguousarray(np.asarray(b[k])[keep])
    b["mono_start"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dev = "cuda:0"
    arrays = {k: torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in PoseInertialOptimizer.EDGE_KEYS}
    kpo = torch.full((F, int(b["kp_cap"])), 255, dtype=torch.uint8, device=dev)
    q = torch.tensor(np.asarray(b["pose_q"], np.float64), device=dev).contiguous()
    t = torch.tensor(np.asarray(b["pose_t"], np.float64), device=dev).contiguous()
    opt = PoseInertialOptimizer(max_frames=F, max_edges=max(len(b["mono_cam"]), 1))
    n_good = opt.PoseOptimization(b, arrays, q, t, kpo)
    torch.cuda.synchronize()
    q, t, n_good = q.cpu().numpy(), t.cpu().numpy(), n_good.cpu().numpy()
    for f in range(F):
        Rt, p = b["true_Rwb"][f], b["true_twb"][f]
        Rc = b["Rcb"][0] @ Rt.T
        tc = b["Rcb"][0] @ (-Rt.T @ p) + b["tcb"][0]
        for name, R, tt in (("pnp", T[f, :3, :3], T[f, :3, 3]), ("optimised", synth_pose.quat_mat(q[f]), t[f])):
            ang = np.degrees(np.arccos(np.clip((np.trace(R.T @ Rc) - 1) / 2, -1, 1)))
            print(f"[mlpnp e] frame {f} {name}: {ang:.4f} deg, {np.linalg.norm(tt - tc) * 100:.3f} cm, "
                  f"{n_inl[f]} inliers of {len(jobs[f]['index'])}, nGood {n_good[f]}")
        assert ang < 0.05 and np.linalg.norm(t[f] - tc) < 0.01
        assert n_good[f] >= 0.9 * n_inl[f]


def test_cpp_adapter_consumer(torch_cuda):
    """tests/cpp/mlpnp_consumer.cpp (omv_adapt::MLPnPsolver, Tracking::Relocalization's call shape) as a child process."""
    if not os.path.exists(omv_build.MLPNP_CONSUMER_BIN):
        pytest.fail(f"{omv_build.MLPNP_CONSUMER_BIN} not built (python -m openmavis_amd.build)")
    r = subprocess.run([omv_build.MLPNP_CONSUMER_BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


# ---- f. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_and_capacity(torch_cuda):
    import torch
    jobs = synth_pnp.make_jobs([10, 12], seed=61, models=PIN)
    s = pnpsolver.MLPnPsolver(jobs, max_hyp=20)
    assert s._set() == _lib.OMV_OK
    for min_set in (5, 7, 0):
        assert s._set(minSet=min_set) == _lib.OMV_ERR_ARG
    keep, jobs[1]["model"] = jobs[1]["model"], 2
    assert s._set() == _lib.OMV_ERR_ARG
    jobs[1]["model"] = keep
    keep = jobs[0]["index"].copy()
    for bad in (jobs[0]["mN"], -1):
        jobs[0]["index"][3] = bad
        assert s._set() == _lib.OMV_ERR_ARG
    jobs[0]["index"][:] = keep
    s.mN[1], keep = -1, s.mN[1]
    assert s._set() == _lib.OMV_ERR_ARG   # a negative size
    s.mN[1] = keep
    assert s._set() == _lib.OMV_OK
    lib = _lib.load()
    z = torch.zeros(21 * 2 * 6, dtype=torch.int32, device="cuda")
    args = (_lib.ptr(z), _lib.ptr(s.T), _lib.ptr(s.n_inliers), _lib.ptr(s.inliers), _lib.ptr(s.flags), s._stream())
    assert lib.omv_pnp_iterate(s._h, 5, 21, *args) == _lib.OMV_ERR_CAPACITY   # more draws than the handle's
    assert lib.omv_pnp_iterate(s._h, -1, 20, *args) == _lib.OMV_ERR_ARG
    assert lib.omv_pnp_iterate(s._h, 5, 20, None, *args[1:]) == _lib.OMV_ERR_ARG
    assert lib.omv_pnp_iterate(None, 5, 20, *args) == _lib.OMV_ERR_ARG
    small = pnpsolver.MLPnPsolver(jobs[:1], max_hyp=20)
    small.jobs, small.n_jobs = jobs, 2   # two jobs on a handle made for one
    small.corr_start, small.mN = s.corr_start, s.mN
    assert small._set() == _lib.OMV_ERR_CAPACITY
    small.jobs, small.n_jobs = [jobs[1]], 1   # 12 correspondences on a handle made for 10
    small.corr_start, small.mN = np.array([0, 12], np.int32), s.mN[1:]
    assert small._set() == _lib.OMV_ERR_CAPACITY
    n_hyp = np.zeros(1, np.int32)
    assert lib.omv_pnp_debug(s._h, 2, _lib.ptr(n_hyp), *([None] * 3), _lib.ptr(n_hyp), *([None] * 5), s._stream()) == \
        _lib.OMV_ERR_ARG
    assert lib.omv_pnp_create(0, 1, 1, None) == _lib.OMV_ERR_ARG and lib.omv_pnp_destroy(None) == _lib.OMV_ERR_ARG
    # the parameters come back as the reference computes them
    s.SetRansacParameters(*ref.TRACKING)
    assert s.max_its.tolist() == [ref.ransac_parameters(n, *ref.TRACKING[:5])[0] for n in (10, 12)]
    assert s.min_inliers.tolist() == [10, 10]
    torch.cuda.synchronize()
