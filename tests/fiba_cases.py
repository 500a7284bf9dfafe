"""The FullInertialBA cases tests/test_fiba_gpu.py runs on the device and tests/test_fiba_ref_cpu.py checks on the
reference alone (no marginal LM decision in any of them), and how two solutions of a case are compared.

Shapes: the smallest that reach each path of the solver (one build group or several, all blocks in LDS or the hybrid
storage, the one-landmark build path past 32 keyframes), not the workload's.

Free gauge.  With no fixed keyframe the problem has four free directions (translation, yaw about gravity) that only
lambda = 1e-5 holds, against entries of 1e15 in the reduced system: two correct solvers drift apart along them by far more
than 1e-5 (1e-4 m between two elimination orders of the reference itself).  Such a case is compared in gauge-invariant
quantities (fiba_ref.gauge_invariant).  It also uses Pinhole cameras: KannalaBrandt8::project goes through float, which
makes every edge's chi2 a step function at 1e-5; a drift along the gauge then re-draws all those steps (measured: 3e-3
of chi2 over 1,700 edges), and every late LM decision, whose gain is smaller than that, becomes a coin toss between two
correct solvers.  Pinhole::project is double throughout, so the chi2 is as invariant as the problem.
The KannalaBrandt8 free-gauge case (`opt_shared_kb8`, the first initialisation's own configuration) is therefore compared
on the optimum alone -- err_end and the gauge-invariant state, no counts -- at the larger of tests/test_lba_gpu.py's bar
and ten times the reference's own spread: `spread_of` measures the reference against itself (the reduced system
eliminated in the reverse order; every input state array one ulp up).  DESIGN's accuracy table records spread and bar."""
import numpy as np

import fiba_ref
from openmavis_amd import synth_fiba

ITERATIONS = 15   # of the optimize cases (the wide case: 6)

CASES = {
    # evaluate / debug_solve (all blocks in LDS)
    "eval_shared": dict(n_kf=6, n_pts=150, seed=21, shared_bias=True),
    "eval_per_kf": dict(n_kf=6, n_pts=150, seed=21, shared_bias=False),
    # every landmark seen by every keyframe: 231 blocks, the hybrid storage
    "dense20": dict(n_kf=20, n_pts=60, seed=22, shared_bias=True, wide_landmarks=60, wide_kfs=20),
    # optimize
    "opt_shared": dict(n_kf=12, n_pts=300, seed=12, shared_bias=True, prior_g=1e2, prior_a=1e5, pinhole=True),
    # the first initialisation's own configuration (KannalaBrandt8, no fixed keyframe): compared on the optimum only
    "opt_shared_kb8": dict(n_kf=12, n_pts=300, seed=3, shared_bias=True, prior_g=1e2, prior_a=1e5),
    # more inertial edges than the errors' lead block has threads (256): the rest go to a kernel of their own
    "many_edges": dict(n_kf=260, n_pts=400, seed=14, shared_bias=True, fix_last=True),
    "opt_per_kf_fix": dict(n_kf=12, n_pts=300, seed=11, shared_bias=False, fix_last=True),
    "no_imu_first": dict(n_kf=10, n_pts=250, seed=5, shared_bias=True, fix_last=True, no_imu_first=True),
    "broken_chain": dict(n_kf=10, n_pts=250, seed=6, shared_bias=True, fix_last=True, break_chain=True),
    "pinhole_stereo": dict(n_kf=10, n_pts=250, seed=8, shared_bias=True, fix_last=True, pinhole=True, stereo_frac=0.5),
    "fixed_only_pts": dict(n_kf=10, n_pts=250, seed=1, shared_bias=True, fix_last=True, fixed_only_pts=5),
    "wide": dict(n_kf=40, n_pts=200, seed=10, shared_bias=True, fix_last=True, wide_landmarks=20, wide_kfs=34),
}
OPTIMIZE = ("opt_shared", "opt_per_kf_fix", "no_imu_first", "broken_chain", "pinhole_stereo", "fixed_only_pts", "wide")


def iterations_of(name):
    return 6 if name == "wide" else ITERATIONS


def problem(name):
    return synth_fiba.make_fiba_problem(**CASES[name])


def free_gauge(prob):
    return int(prob["n_opt"]) == int(prob["n_kf"])


def reference(name, oracle, order=None, ulp=False):
    """(problem, graph, result, final state) of the reference on a case.  order="reverse": the reduced system eliminated
    in the reverse order; ulp: every state array of the input moved one ulp up."""
    prob = problem(name)
    if ulp:
        for k in ("Rwb", "twb", "vel", "pts"):
            prob[k] = np.nextafter(np.asarray(prob[k], np.float64), np.inf)
        K, C = prob["n_kf"], prob["n_cams"]
        G0 = fiba_ref.Graph(prob)
        Rwb = np.asarray(prob["Rwb"]).reshape(K, 3, 3)
        cp = [fiba_ref.cam_poses(G0, Rwb[k], np.asarray(prob["twb"])[k]) for k in range(K)]
        prob["Rcw"], prob["tcw"] = np.stack([c[0] for c in cp]), np.stack([c[1] for c in cp])
    G = fiba_ref.Graph(prob)
    o = np.arange(int(G.present.sum()))[::-1] if order == "reverse" else None
    res, st = fiba_ref.optimize(G, fiba_ref.start_of(prob), oracle, iterations=iterations_of(name), order=o)
    return prob, G, res, st


def views(prob, st):
    """The quantities two solutions are compared in: plain coordinates with a fixed keyframe, gauge-invariant without."""
    st = {k: np.asarray(v, np.float64) for k, v in st.items()}
    st["Rwb"] = st["Rwb"].reshape(-1, 3, 3)
    if free_gauge(prob):
        g = fiba_ref.gauge_invariant(st)
        g.pop("pts")
        return g
    return {k: st[k] for k in ("Rwb", "twb", "vel", "bg", "ba")}


def spread_of(name, oracle, base_state, base_err_end, points_metric):
    """Per compared quantity, the larger difference of the reference from itself (reverse elimination order, inputs one ulp
    up); the same for the points, as points_metric(state) measures them against base_state; and for err_end."""
    prob = problem(name)
    v0 = views(prob, base_state)
    out, pts, end = {k: 0.0 for k in v0}, 0.0, 0.0
    for kw in (dict(order="reverse"), dict(ulp=True)):
        _, _, res, st = reference(name, oracle, **kw)
        end = max(end, abs(res["err_end"] - base_err_end))
        v = views(prob, st)
        for k in v0:
            out[k] = max(out[k], float(np.abs(v[k] - v0[k]).max()))
        pts = max(pts, float(points_metric(st)))
    return out, pts, end
