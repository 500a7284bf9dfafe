"""The device Sim3Solver (openmavis_amd/csrc/sim3.hip through openmavis_amd/sim3solver.py) against tests/sim3_ref.py.

a. sampling      the sampled correspondences (debug hook) equal the replay of the swap-with-back list, exactly
b. ComputeSim3   R, s, t, T12, T21 per hypothesis against the float64 reference: for each quantity q
                 |q_gpu - q_64|_inf <= max(4 e_ref(q), 3 n u kappa_h max(1, |q_64|_inf)), n = 4, u = 2^-24,
                 kappa_h = |Pr1|_F |Pr2|_F / (lambda_1 - lambda_2) from the reference's eigenvalues, e_ref the error of
                 the float32 restatement (sim3_ref.compute_sim3_32).  Hypotheses with kappa_h > 1e4 are left out of this
                 comparison only, at most 2 % of a case.
c. CheckInliers  with the device's own T12 / T21 the float64 errors decide every (hypothesis, correspondence) whose two
                 errors are outside [t (1 - d), t (1 + d)], d = 2^-10: the device mask must agree there exactly, count
                 must be the mask's popcount, and at most 0.1 % of the entries may be inside the band.
d. selection     from the device's own counts the Python replay of iterate gives exactly the device's flags, nInliers,
                 mnIterations, mnBestInliers, chosen hypothesis, T12 (bitwise) and vbInliers
e. degenerate    coinciding points (s = NaN): count 0 everywhere, bNoMore after maxIts, identity, OMV_OK
f. end to end    planted similarity; the chain find -> to_sim3f -> ORBmatcher.SearchBySim3
g. argument errors

Measured on an MI355X (pytest -s prints the figures): see DESIGN.md section 6."""
import functools
import os
import subprocess

import numpy as np
import pytest

import sim3_ref as ref
from openmavis_amd import _lib, build as omv_build, sim3solver, synth_sim3solver as ss

pytestmark = pytest.mark.gpu

DELTA = 2.0 ** -10
KB8, PIN = 0, 1


def _draws_for(n, idx):
    """Raw draws that make the sampling pick idx[0], idx[1], idx[2]."""
    avail, r = list(range(n)), []
    for v in idx:
        p = avail.index(v)
        r.append(p)
        avail[p] = avail[-1]
        avail.pop()
    return r


@functools.lru_cache(maxsize=None)
def _case(ns, H, fix_scale, models, seed=11, min_inliers=None):
    """One handle over the jobs make_jobs(ns) gives, one iterate(H) on seeded draws -> (jobs, draws, hypotheses per job,
    solver).  minInliers defaults to 6 as the constructor sets it (1 for a job of three correspondences, which 6 would
    leave without work): the hook returns the whole chunk whether or not a hypothesis converges."""
    jobs = ss.make_jobs(list(ns), seed=seed, models=models, fix_scale=fix_scale)
    s = sim3solver.Sim3Solver(jobs, max_hyp=max(H, 1))
    s.SetRansacParameters(0.99, [1 if n <= 6 else 6 for n in ns] if min_inliers is None else min_inliers, 300)
    draws = s.draw(np.random.default_rng(seed + 100), H)
    s.iterate(H, draws)
    hyps = [s.hypotheses(j) for j in range(len(jobs))]
    return jobs, draws, hyps, s


# ---- a. sampling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 64, 65])
def test_sampling_exact(torch_cuda, n):
    rng = np.random.default_rng(n)
    special = [[r0, r0, min(r0, n - 3)] for r0 in range(min(n - 1, 4))]   # r1 == r0 (and r2 == r0 where in range)
    special += [[n - 1, n - 2, n - 3], [n - 2, n - 2, n - 3], [n - 1, 0, 0], [n - 2, 0, 0], [0, n - 2, 0],
                [0, 0, 0], [n - 3, n - 3, n - 3], [1, 0, 0], [0, 1, 0]]   # the back positions, r2 == r1, r2 == r0
    special = [[min(r[0], n - 1), min(r[1], n - 2), min(r[2], n - 3)] for r in special]
    allr = [[a, b, c] for a in range(n) for b in range(n - 1) for c in range(n - 2)] if n <= 4 else \
        [[int(rng.integers(0, n - i)) for i in range(3)] for _ in range(80)]
    draws = np.array(special + allr, np.int32)
    job = ss.make_job(n, seed=5, model1=PIN, model2=PIN)
    s = sim3solver.Sim3Solver([job], max_hyp=len(draws))
    s.SetRansacParameters(0.99, 1 if n <= 4 else 6, 300)
    assert s.max_its[0] >= len(draws)
    s.iterate(len(draws), draws[None])
    idx = s.hypotheses(0)["idx"]
    assert len(idx) == len(draws)
    for k, r in enumerate(draws):
        assert idx[k].tolist() == ref.sample_literal(n, r.tolist()) == ref.sample_replay(n, r.tolist()), (k, r)
    assert any(r[1] == r[0] for r in special) and any(r[2] == r[1] for r in special) and any(r[2] == r[0] for r in special)


# ---- b. ComputeSim3 ----------------------------------------------------------------------------------------------
B_CASES = [(3, 1, False, PIN), (3, 20, True, KB8), (65, 1, True, KB8), (65, 20, False, KB8), (65, 300, True, PIN),
           (130, 20, True, PIN), (130, 300, False, KB8), (130, 300, False, PIN)]


@pytest.mark.parametrize("n,H,fix_scale,model", B_CASES)
def test_compute_sim3_against_float64(torch_cuda, n, H, fix_scale, model):
    jobs, draws, hyps, s = _case((n,), H, fix_scale, (model, model))
    job, hy = jobs[0], hyps[0]
    assert len(hy["idx"]) == min(H, int(s.max_its[0])) == H
    pre = ref.prepare(job)
    X1, X2 = pre["X1"].astype(np.float32), pre["X2"].astype(np.float32)   # the device's float X3Dc up to rounding
    worst = {}
    left_out = 0
    nu = 4 * ref.U32
    for h in range(H):
        idx = hy["idx"][h]
        a = ref.compute_sim3_64(X1[idx].T, X2[idx].T, fix_scale)
        if not a["kappa"] <= 1e4:
            left_out += 1
            continue
        b = ref.compute_sim3_32(X1[idx].T, X2[idx].T, fix_scale)
        for q in ("R", "s", "t", "T12", "T21"):
            e = np.abs(np.asarray(hy[q][h], np.float64) - a[q]).max()
            e_ref = np.abs(np.asarray(b[q], np.float64) - a[q]).max()
            cond = nu * a["kappa"] * max(1.0, np.abs(a[q]).max())
            w = worst.setdefault(q, [0.0, 0.0])
            w[0] = max(w[0], e / cond)
            w[1] = max(w[1], e / max(e_ref, 1e-300) if e > 3 * cond else 0.0)
            assert e <= max(4 * e_ref, 3 * cond), (h, q, e, e_ref, cond, a["kappa"])
        if fix_scale:
            assert hy["s"][h] == 1.0
    print(f"[sim3 b] N {n} H {H} fix {fix_scale} model {model}: left out {left_out}; worst e/(n u kappa), and e/e_ref "
          f"where the first exceeds 3: " + ", ".join(f"{q} {w[0]:.3g} / {w[1]:.3g}" for q, w in worst.items()))
    assert left_out <= 0.02 * H


# ---- c. CheckInliers ---------------------------------------------------------------------------------------------
def _band_check(job, hy):
    """(entries, entries in the band, mismatches outside the band) for one job's hypotheses."""
    pre = ref.prepare(job)
    n_band = n_bad = 0
    with np.errstate(all="ignore"):
        for h in range(len(hy["idx"])):
            e1, e2 = ref.reprojection_errors(job, pre, hy["T12"][h], hy["T21"][h])
            band = ((e1 >= pre["e1"] * (1 - DELTA)) & (e1 <= pre["e1"] * (1 + DELTA))) | \
                   ((e2 >= pre["e2"] * (1 - DELTA)) & (e2 <= pre["e2"] * (1 + DELTA)))
            inl = (e1 < pre["e1"]) & (e2 < pre["e2"])
            n_band += int(band.sum())
            n_bad += int(((inl != hy["mask"][h]) & ~band).sum())
            assert hy["count"][h] == hy["mask"][h].sum() == sum(bin(int(w)).count("1") for w in hy["words"][h])
    return hy["mask"].size, n_band, n_bad


C_CASES = [((63, 64, 65), 300, False, (KB8, KB8)), ((63, 64, 65), 300, True, (PIN, PIN)),
           ((130, 3, 65), 300, False, (KB8, PIN)), ((130,), 300, False, (PIN, PIN))]


@pytest.mark.parametrize("ns,H,fix_scale,models", C_CASES)
def test_check_inliers_with_device_transforms(torch_cuda, ns, H, fix_scale, models):
    jobs, draws, hyps, s = _case(ns, H, fix_scale, models)
    octaves = set()
    tot = band = 0
    for job, hy in zip(jobs, hyps):
        pre = ref.prepare(job)
        octaves |= set(np.unique(job["sigma2_1"]).tolist())
        assert (pre["e1"] != 9.210 * job["sigma2_1"].astype(np.float64)).any()   # the truncation is at work
        n, nb, bad = _band_check(job, hy)
        assert bad == 0, (len(job["index1"]), bad)
        tot, band = tot + n, band + nb
        assert hy["mask"].any() or len(job["index1"]) == 3
    assert len(ns) == 1 or len(octaves) == 8   # octaves 0-7
    print(f"[sim3 c] N {ns} fix {fix_scale} models {models}: {band} of {tot} entries in the band ({band / tot:.4%})")
    assert band <= 1e-3 * tot


# ---- d. selection --------------------------------------------------------------------------------------------------
def _scenario():
    """Six jobs in one handle (ragged N = 5 / 64 / 130 among them) with draws arranged from triplets the float64
    reference rates good (planted inliers, many inliers) or bad (outliers, few)."""
    ns = [5, 64, 130, 65, 64, 10]
    min_inl = [5, 20, 20, 20, 45, 12]   # == N (maxIts 1) | converge first | middle | last | never, ties | N < minInliers
    jobs = ss.make_jobs(ns, seed=31, models=[(PIN, PIN), (KB8, KB8), (KB8, PIN), (PIN, KB8), (KB8, KB8), (PIN, PIN)])
    max_its = [ref.ransac_max_its(0.99, m, n, 300) for m, n in zip(min_inl, ns)]
    H = max(max_its)
    rng = np.random.default_rng(9)
    draws = np.zeros((len(ns), H, 3), np.int32)
    for j, (job, n) in enumerate(zip(jobs, ns)):
        rs = ref.RefSolver(job)
        inl, out = np.nonzero(job["inlier"])[0], np.nonzero(~job["inlier"])[0]
        good, bad = [], []
        while len(good) < 2 or len(bad) < 6:
            g, b = rng.choice(inl, 3, replace=False), (rng.choice(out, 3, replace=False) if len(out) >= 3 else None)
            if len(good) < 2 and rs.hypothesis(_draws_for(n, g))["mask"].sum() > 0.4 * n:
                good.append(_draws_for(n, g))
            if b is None:
                bad.append(_draws_for(n, rng.choice(n, 3, replace=False)))
            elif rs.hypothesis(_draws_for(n, b))["mask"].sum() < 0.1 * n:
                bad.append(_draws_for(n, b))
        row = [bad[k % 5] for k in range(H)]
        if j == 1:
            row[0] = good[0]
        elif j == 2:
            row[27] = good[0]
        elif j == 3:
            row[max_its[j] - 1] = good[0]
        elif j == 4:   # the same triplet three times: equal counts, the latest becomes best; later ones stay below it
            row[3] = row[7] = row[8] = good[1]
        draws[j] = row
    return jobs, min_inl, max_its, draws


def _replay_and_compare(s, jobs, min_inl, max_its, draws, step):
    """Run iterate(step) until every job is finished; after each call replay it in Python from the device's counts."""
    J = len(jobs)
    st = [ref.new_state(len(j["index1"]), m, mi) for j, m, mi in zip(jobs, min_inl, max_its)]
    T_exp = [np.eye(4, dtype=np.float32) for _ in range(J)]
    vb_exp = [np.zeros(j["mN1"], bool) for j in jobs]
    best_exp = [dict(R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), s=np.float32(1)) for _ in range(J)]
    events = []
    H = draws.shape[1]
    for c0 in range(0, H + step, step):   # one extra call: finished jobs are untouched
        chunk_draws = np.zeros((J, step, 3), np.int32)
        part = draws[:, c0:c0 + step]
        chunk_draws[:, :part.shape[1]] = part
        T12, no_more, vb, n_inl, conv = s.iterate(step, chunk_draws)
        T12, no_more, n_inl, conv = T12.cpu().numpy(), no_more.cpu().numpy(), n_inl.cpu().numpy(), conv.cpu().numpy()
        for j in range(J):
            was_done = st[j]["flags"] != 0
            hy = s.hypotheses(j)
            chosen, chunk = ref.select(st[j], hy["count"], step)
            assert len(hy["count"]) == chunk, (j, c0)
            if chosen is not None:
                T_exp[j] = hy["T12"][chosen]
                best_exp[j] = dict(R=hy["R"][chosen], t=hy["t"][chosen], s=hy["s"][chosen])
                if st[j]["flags"] & ref.CONVERGE:
                    vb_exp[j][:] = False
                    vb_exp[j][jobs[j]["index1"][hy["mask"][chosen]]] = True
                    events.append((j, c0 + chosen, "converge"))
            flags = int(no_more[j]) * ref.NO_MORE + int(conv[j]) * ref.CONVERGE
            assert flags == st[j]["flags"], (j, c0, flags, st[j])
            assert n_inl[j] == (st[j]["n_inliers"] if conv[j] else 0)
            assert T12[j].tobytes() == np.ascontiguousarray(T_exp[j]).tobytes(), (j, c0, was_done)
            assert np.array_equal(s.job_inliers(j), vb_exp[j]), (j, c0)
            assert s.best_inliers_and_iterations(j) == (st[j]["best_inliers"], st[j]["iterations"]), (j, c0)
            R, t, sc = s.GetEstimatedRotation(j), s.GetEstimatedTranslation(j), s.GetEstimatedScale(j)
            assert R.tobytes() == np.ascontiguousarray(best_exp[j]["R"]).tobytes()
            assert t.tobytes() == np.ascontiguousarray(best_exp[j]["t"]).tobytes()
            assert np.float32(sc).tobytes() == np.float32(best_exp[j]["s"]).tobytes()
    assert all(x["flags"] for x in st)
    return st, T_exp, vb_exp, best_exp, events


def test_selection_replay_chunks_and_find(torch_cuda):
    jobs, min_inl, max_its, draws = _scenario()
    H = draws.shape[1]
    s = sim3solver.Sim3Solver(jobs, max_hyp=H)
    s.SetRansacParameters(0.99, min_inl, 300)
    assert s.max_its.tolist() == max_its and max_its[0] == 1 and H == 300
    st, T_exp, vb_exp, best_exp, events = _replay_and_compare(s, jobs, min_inl, max_its, draws, 20)   # 15 calls + 1
    # every case is the one it is named for
    assert (st[0]["flags"], st[0]["iterations"]) == (ref.NO_MORE, 1)                    # minInliers == N
    assert (st[1]["flags"], st[1]["iterations"]) == (ref.CONVERGE, 1)                   # converged at the first
    assert (st[2]["flags"], st[2]["iterations"]) == (ref.CONVERGE, 28)                  # in the middle (second call)
    assert (st[3]["flags"], st[3]["iterations"]) == (ref.CONVERGE, max_its[3])          # at the last hypothesis
    assert (st[4]["flags"], st[4]["iterations"]) == (ref.NO_MORE, max_its[4])           # never
    assert (st[5]["flags"], st[5]["iterations"]) == (ref.NO_MORE, 0)                    # N < minInliers: no work
    assert np.array_equal(T_exp[5], np.eye(4)) and np.array_equal(T_exp[0][3], [0, 0, 0, 1])
    assert sorted(e[:2] for e in events) == [(1, 0), (2, 27), (3, max_its[3] - 1)]
    # job 4: the tie of the best count went to the latest of the three equal hypotheses
    s4 = sim3solver.Sim3Solver([jobs[4]], max_hyp=H)
    s4.SetRansacParameters(0.99, min_inl[4], 300)
    s4.iterate(20, draws[4:5, :20])
    c = s4.hypotheses(0)["count"]
    assert len(c) == max_its[4] >= 9 and c.max() <= min_inl[4]
    assert c[3] == c[7] == c[8] == c.max() and (c == c.max()).sum() == 3
    assert s4.T12[0].cpu().numpy().tobytes() == s4.hypotheses(0)["T12"][8].tobytes()
    # one find on the same draws ends in the same state
    s.SetRansacParameters(0.99, min_inl, 300)
    T12, vb, n_inl = s.find(draws)
    T12, n_inl, flags = T12.cpu().numpy(), n_inl.cpu().numpy(), s.flags.cpu().numpy()
    for j in range(len(jobs)):
        conv = bool(st[j]["flags"] & ref.CONVERGE)
        assert flags[j] == st[j]["flags"] and n_inl[j] == (st[j]["n_inliers"] if conv else 0)
        assert T12[j].tobytes() == (np.ascontiguousarray(T_exp[j]) if conv else np.eye(4, dtype=np.float32)).tobytes()
        assert np.array_equal(s.job_inliers(j), vb_exp[j])
        assert s.best_inliers_and_iterations(j) == (st[j]["best_inliers"], st[j]["iterations"])
        assert s.GetEstimatedRotation(j).tobytes() == np.ascontiguousarray(best_exp[j]["R"]).tobytes()
        assert np.float32(s.GetEstimatedScale(j)).tobytes() == np.float32(best_exp[j]["s"]).tobytes()


def test_selection_ragged_batch_other_chunking(torch_cuda):
    """The 3-job ragged batch N = 5 / 64 / 130 in one handle, random draws, chunks of 64 + 1 (the select kernel's word
    edge) and of 7."""
    ns, min_inl = [5, 64, 130], [3, 25, 45]
    jobs = ss.make_jobs(ns, seed=41, models=[(KB8, KB8), (PIN, KB8), (KB8, PIN)])
    max_its = [ref.ransac_max_its(0.99, m, n, 300) for m, n in zip(min_inl, ns)]
    for step in (65, 7):
        s = sim3solver.Sim3Solver(jobs, max_hyp=step)
        s.SetRansacParameters(0.99, min_inl, 300)
        draws = s.draw(np.random.default_rng(step), max(max_its))
        _replay_and_compare(s, jobs, min_inl, max_its, draws, step)


# ---- e. degenerate input -------------------------------------------------------------------------------------------
def test_coinciding_points_end_cleanly(torch_cuda):
    n = 20
    job = ss.make_job(n, seed=2, model1=PIN, model2=KB8)
    # every point the same, with coordinates whose centroid is exact in float: Pr1 = Pr2 = 0, den = 0, s = NaN
    job["pose1"] = job["pose2"] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    job["Xw1"] = np.tile(np.array([1.5, -0.75, 8.0], np.float32), (n, 1))
    job["Xw2"] = np.tile(np.array([1.25, 0.5, 6.0], np.float32), (n, 1))
    s = sim3solver.Sim3Solver([job])
    assert s._set(0.99, 6, 300) == _lib.OMV_OK
    H = int(s.max_its[0])
    assert H == ref.ransac_max_its(0.99, 6, n, 300) and 1 < H <= 300
    T12, vb, n_inl = s.find(s.draw(np.random.default_rng(1), H))
    hy = s.hypotheses(0)
    assert len(hy["count"]) == H and (hy["count"] == 0).all() and not hy["mask"].any()
    assert np.isnan(hy["s"]).all()
    assert int(s.flags[0]) == ref.NO_MORE and int(n_inl[0]) == 0 and not s.job_inliers(0).any()
    assert np.array_equal(T12[0].cpu().numpy(), np.eye(4, dtype=np.float32))
    assert s.best_inliers_and_iterations(0) == (0, H)


# ---- f. end to end ---------------------------------------------------------------------------------------------------
def test_planted_similarity_end_to_end(torch_cuda):
    seeds, agree = (51, 52, 53, 54), 0
    jobs = [ss.make_job(100, seed=sd, inlier_share=0.6, model1=m[0], model2=m[1])
            for sd, m in zip(seeds, ((KB8, KB8), (PIN, PIN), (KB8, PIN), (PIN, KB8)))]
    s = sim3solver.Sim3Solver(jobs, max_hyp=300)
    s.SetRansacParameters(0.99, 20, 300)
    assert (s.max_its == 300).all()
    draws = s.draw(np.random.default_rng(77), 300)
    T12, vb, n_inl = s.find(draws)
    T12, n_inl = T12.cpu().numpy(), n_inl.cpu().numpy()
    for j, job in enumerate(jobs):
        assert int(s.flags[j]) == ref.CONVERGE and n_inl[j] > 20
        hy = s.hypotheses(j)
        k = s.best_inliers_and_iterations(j)[1] - 1   # the hypothesis it converged at
        assert T12[j].tobytes() == hy["T12"][k].tobytes() and hy["count"][k] == n_inl[j]
        # the decisions of this run: every hypothesis up to the convergence
        pre = ref.prepare(job)
        in_band = 0
        for h in range(k + 1):
            e1, e2 = ref.reprojection_errors(job, pre, hy["T12"][h], hy["T21"][h])
            in_band += int((((e1 >= pre["e1"] * (1 - DELTA)) & (e1 <= pre["e1"] * (1 + DELTA))) |
                            ((e2 >= pre["e2"] * (1 - DELTA)) & (e2 <= pre["e2"] * (1 + DELTA)))).sum())
        rs = ref.RefSolver(job)
        rs.SetRansacParameters(0.99, 20, 300)
        rs.find(draws[j])
        print(f"[sim3 f] job {j}: device converged at hypothesis {k} with {n_inl[j]} inliers, reference at "
              f"{rs.state['iterations'] - 1} with {rs.state['n_inliers']}; {in_band} decisions in the band")
        if in_band == 0:
            agree += 1
            assert rs.state["flags"] == ref.CONVERGE and rs.state["iterations"] - 1 == k
        # the recovered transform moves the inlier points to within their thresholds
        e1, e2 = ref.reprojection_errors(job, pre, T12[j], hy["T21"][k])
        m = hy["mask"][k]
        assert (e1[m] < pre["e1"][m] * (1 + DELTA)).all() and (e2[m] < pre["e2"][m] * (1 + DELTA)).all()
        vbj = s.job_inliers(j)
        assert vbj.sum() == n_inl[j] and np.array_equal(np.nonzero(vbj)[0], job["index1"][m])
        R, sc = s.GetEstimatedRotation(j).astype(np.float64), float(s.GetEstimatedScale(j))
        ang = np.arccos(np.clip((np.trace(R.T @ job["R12"]) - 1) / 2, -1, 1))
        assert ang < 0.1 and abs(sc - job["s12"]) < 0.1 * job["s12"]   # a sanity check, not an accuracy bar
    assert agree >= 1


def test_chain_find_then_search_by_sim3(torch_cuda):
    """Truth correspondences of synth_sim3.make_sim3_batch -> Sim3Solver.find -> to_sim3f -> ORBmatcher.SearchBySim3:
    more than 100 matches per pair, as tests/test_sim3_gpu.py sees with the planted Sim3."""
    from openmavis_amd import synth_sim3
    from openmavis_amd.synth_kfmatch import _R_of
    from test_sim3_gpu import _run_gpu
    b = synth_sim3.make_sim3_batch(n_pairs=2, seed=1)
    s2 = ss.level_sigma2(b["nlevels"])
    cam = np.array([synth_sim3.FX, synth_sim3.FY, synth_sim3.CX, synth_sim3.CY, 0, 0, 0, 0], np.float32)
    jobs = []
    for jb in b["jobs"]:
        k1, k2 = jb["kf1"], jb["kf2"]
        kp1 = b["kp1"][jb["start1"]:jb["start1"] + jb["count1"]]
        mp1 = b["mp1"][jb["start1"]:jb["start1"] + jb["count1"]]
        kp2 = b["kp2"][jb["start2"]:jb["start2"] + jb["count2"]]
        mp2 = b["mp2"][jb["start2"]:jb["start2"] + jb["count2"]]
        # block-0 keypoints of the two keyframes that show the same world point (the truth a BoW search approximates)
        w2 = {int(b["wid"][k2, k]): (int(k), int(r)) for k, r in zip(kp2, mp2) if k < b["kp_cap"] and b["wid"][k2, k] >= 0}
        rows = [(int(k), int(r)) + w2[int(b["wid"][k1, k])] for k, r in zip(kp1, mp1)
                if k < b["kp_cap"] and int(b["wid"][k1, k]) in w2]
        a = np.array(rows, np.int64)
        poses = [np.concatenate([_R_of(np.asarray(T[:4], np.float64)).ravel(), np.asarray(T[4:], np.float64)]).astype(np.float32)
                 for T in (jb["T1w"], jb["T2w"])]
        jobs.append(dict(Xw1=b["mps"]["pos"][a[:, 1]], Xw2=b["mps"]["pos"][a[:, 3]],
                         sigma2_1=s2[b["kps"]["octave"][k1, 0, a[:, 0]]], sigma2_2=s2[b["kps"]["octave"][k2, 0, a[:, 2]]],
                         index1=a[:, 0].astype(np.int32), mN1=int(b["n_kp"][k1].sum()), pose1=poses[0], pose2=poses[1],
                         cam1=cam, cam2=cam, model1=PIN, model2=PIN, fix_scale=False))
        assert len(a) > 100
    s = sim3solver.Sim3Solver(jobs, max_hyp=300)
    s.SetRansacParameters(0.99, 20, 300)
    s.find(s.draw(np.random.default_rng(3), int(s.max_its.max())))
    assert (s.flags.cpu().numpy()[:len(jobs)] == ref.CONVERGE).all()
    for j, jb in enumerate(b["jobs"]):
        jb["S12"], jb["S21"] = sim3solver.to_sim3f(s.GetEstimatedRotation(j), s.GetEstimatedTranslation(j),
                                                   s.GetEstimatedScale(j))
    match12, n_found = _run_gpu(b)
    print(f"[sim3 chain] SearchBySim3 with the solver's Sim3: {n_found.tolist()} matches")
    assert n_found.min() > 100


def test_cpp_adapter_consumer(torch_cuda):
    """tests/cpp/sim3_solver_consumer.cpp (omv_adapt::Sim3Solver, LoopClosing's call shape) as a child process."""
    if not os.path.exists(omv_build.SIM3_CONSUMER_BIN):
        pytest.fail(f"{omv_build.SIM3_CONSUMER_BIN} not built (python -m openmavis_amd.build)")
    r = subprocess.run([omv_build.SIM3_CONSUMER_BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


# ---- g. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    import torch
    jobs = ss.make_jobs([10, 12], seed=61, models=(PIN, PIN))
    s = sim3solver.Sim3Solver(jobs, max_hyp=20)
    assert s._set(0.99, 6, 300) == _lib.OMV_OK
    for key, bad in (("model1", 2), ("model2", -1)):
        keep, jobs[1][key] = jobs[1][key], bad
        assert s._set(0.99, 6, 300) == _lib.OMV_ERR_ARG, key
        jobs[1][key] = keep
    keep = jobs[0]["index1"].copy()
    for bad in (jobs[0]["mN1"], -1):
        jobs[0]["index1"][3] = bad
        assert s._set(0.99, 6, 300) == _lib.OMV_ERR_ARG
    jobs[0]["index1"][:] = keep
    jobs[1]["mN1"], keep = -1, jobs[1]["mN1"]
    s.mN1[1] = -1
    assert s._set(0.99, 6, 300) == _lib.OMV_ERR_ARG   # a negative size
    jobs[1]["mN1"] = s.mN1[1] = keep
    assert s._set(0.99, 6, 300) == _lib.OMV_OK
    # capacity: more hypotheses than the handle's, more jobs, more correspondences
    lib = _lib.load()
    z = torch.zeros(21 * 2 * 3, dtype=torch.int32, device="cuda")
    st = lib.omv_sim3_solver_iterate(s._h, 21, _lib.ptr(z), _lib.ptr(s.T12), _lib.ptr(s.n_inliers), _lib.ptr(s.inliers),
                                     _lib.ptr(s.flags), s._stream())
    assert st == _lib.OMV_ERR_CAPACITY
    small = sim3solver.Sim3Solver(jobs[:1], max_hyp=20)
    small.jobs, small.n_jobs = jobs, 2   # two jobs on a handle made for one
    small.corr_start, small.mN1 = s.corr_start, s.mN1
    assert small._set(0.99, 6, 300) == _lib.OMV_ERR_CAPACITY
    small.jobs, small.n_jobs = [jobs[1]], 1   # 12 correspondences on a handle made for 10
    small.corr_start, small.mN1 = np.array([0, 12], np.int32), s.mN1[1:]
    assert small._set(0.99, 6, 300) == _lib.OMV_ERR_CAPACITY
    torch.cuda.synchronize()
