"""Time LocalBundleAdjustment optimize(10) on workload shapes, beside the inertial handle on the same graph without
inertial edges (the yardstick: the Schur complement and the solve are the same code):

    python tools/vba_time.py [--runs 20] [--warmup 3] [--out profiles/vba_bench.json]

  window  a LocalMapping window: 30 optimisable + 40 fixed keyframes, 4 cameras, 8,000 points
  early   an early map: 5 + 2 keyframes, 800 points
Wall time is a host clock round one optimize() (it ends in a stream synchronise), after a device-side reset; per-stage
milliseconds come from separate runs with the stage events on (direct launches instead of the captured steps).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmavis_amd import synth_vba  # noqa: E402
from openmavis_amd.optimizer import LocalBundleAdjustment, LocalInertialBA  # noqa: E402

SHAPES = {"window": dict(n_kf=70, n_opt=30, n_pts=8000, seed=31, views=6, n_fixed_only=50, n_edgeless=10),
          "early": dict(n_kf=7, n_opt=5, n_pts=800, seed=32, views=4, n_fixed_only=0, n_edgeless=0)}


def as_inertial_problem(p):
    """The same graph for LocalInertialBA: the body is camera 0, no inertial edge, 6-dof keyframe blocks."""
    K, C = p["n_kf"], p["n_cams"]
    R0w = np.stack([synth_vba.q_to_R(q) for q in p["q_cw"]])
    R_c0 = np.stack([synth_vba.q_to_R(q) for q in p["q_c0"]])
    Rwb = np.transpose(R0w, (0, 2, 1))
    twb = -np.einsum("kij,kj->ki", Rwb, p["t_cw"])
    Rbc = np.transpose(R_c0, (0, 2, 1))
    z3 = np.zeros((K, 3))
    return dict(n_cams=C, cam=p["cam"], cam_model=p["cam_model"], Rcb=R_c0, tcb=p["t_c0"], Rbc=Rbc,
                tbc=-np.einsum("cij,cj->ci", Rbc, p["t_c0"]), n_kf=K, n_opt=p["n_opt"], kf_imu=np.zeros(K, np.uint8),
                Rwb=Rwb, twb=twb, Rcw=np.einsum("cij,kjl->kcil", R_c0, R0w),
                tcw=np.einsum("cij,kj->kci", R_c0, p["t_cw"]) + p["t_c0"][None], vel=z3, bg=z3, ba=z3, pts=p["pts"],
                pt_track_depth=np.full(len(p["pts"]), 20.0, np.float32), mono_pt=p["mono_pt"], mono_kf=p["mono_kf"],
                mono_cam=p["mono_cam"], mono_obs=p["mono_obs"], mono_inv_sigma2=p["mono_inv_sigma2"],
                imu_kf1=np.zeros(0, np.int32), imu_kf2=np.zeros(0, np.int32), preint=np.zeros((0, 292), np.float32),
                imu_robust=np.zeros(0, np.uint8), imu_info_scale=np.zeros(0, np.float32))


def time_handle(ba, run, runs, warmup):
    wall, res = [], None
    for i in range(warmup + runs):
        ba.reset()
        t = time.perf_counter()
        res = run()
        if i >= warmup:
            wall.append((time.perf_counter() - t) * 1e3)
    ba.enable_timing(True)
    stages = []
    for _ in range(3):
        ba.reset()
        run()
        stages.append(ba.stage_ms())
    ba.enable_timing(False)
    st = {k: round(float(np.median([s[k] for s in stages])), 4) for k in ("build", "schur", "solve", "update")}
    wall = np.array(wall)
    return dict(wall_ms_median=round(float(np.median(wall)), 4), wall_ms_min=round(float(wall.min()), 4),
                wall_ms_max=round(float(wall.max()), 4), trials=int(res["trials"]), iterations=int(res["iterations"]),
                ms_per_trial=round(float(np.median(wall)) / max(int(res["trials"]), 1), 4), stage_ms=st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}
    for name, shape in SHAPES.items():
        p = synth_vba.make_vba_problem(**shape)
        E = len(p["mono_pt"])
        vba = LocalBundleAdjustment(p["n_kf"], p["n_cams"], len(p["pts"]), E).set_problem(p)
        lba = LocalInertialBA(p["n_kf"], p["n_cams"], len(p["pts"]), E, 1).set_problem(as_inertial_problem(p))
        out[name] = dict(
            n_kf=p["n_kf"], n_opt=p["n_opt"], n_pts=len(p["pts"]), n_edges=E,
            visual=time_handle(vba, lambda: vba.optimize(10, lambda_init=100.0, chi2=False)[0], a.runs, a.warmup),
            inertial_handle_no_imu=time_handle(
                lba, lambda: lba.optimize(opt_it=10, lambda_init=100.0, large=True, chi2=False)[0], a.runs, a.warmup))
        print(json.dumps({name: out[name]}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
