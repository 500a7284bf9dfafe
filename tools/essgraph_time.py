"""Time one pose-graph optimize() (20 iterations of up to 10 trials) on map-sized graphs:

    python tools/essgraph_time.py [--runs 10] [--warmup 2] [--out profiles/essgraph_bench.json]

  sim3_300   OptimizeEssentialGraph on 300 keyframes (covisibility 2, 3, 7 and 11 apart, one older loop edge)
  4dof_300   OptimizeEssentialGraph4DoF on the same trajectory
  sim3_40    a 40-keyframe map (every block in the solver's LDS)
Device time is between two events round the launches of one optimize() (omv_essgraph_last_ms), after a device-side reset;
wall time is a host clock round the call, which ends in its one stream synchronise.  set_problem (host plan + upload) is
timed apart.  The reference runs this step in g2o on the CPU; it has no timed counterpart here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmavis_amd.optimizer import EssentialGraph  # noqa: E402
from openmavis_amd.synth_essgraph import make_essgraph_problem  # noqa: E402

SHAPES = {"sim3_300": dict(kind="sim3", n_kf=300, seed=8, covis=(2, 3, 7), far=11, drift=0.3),
          "4dof_300": dict(kind="4dof", n_kf=300, seed=8, covis=(2, 3, 7), far=11, drift=0.3),
          "sim3_40": dict(kind="sim3", n_kf=40, seed=6, far=0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}
    for name, kw in SHAPES.items():
        p = make_essgraph_problem(**kw)
        g = EssentialGraph(kw["kind"], len(p["vertices"]), len(p["edge_i"]))
        t = time.perf_counter()
        g.set_problem(p)
        set_ms = (time.perf_counter() - t) * 1e3
        dev, wall, r = [], [], None
        for i in range(a.warmup + a.runs):
            g.reset()
            t = time.perf_counter()
            r = g.optimize(20, 10)
            if i >= a.warmup:
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(g.last_ms())
        d = g.debug_solve(1.0)
        out[name] = dict(vertices=len(p["vertices"]), edges=len(p["edge_i"]), blocks=len(d["x"]) // 16, stored_blocks=d["n_slots"],
                         blocks_in_lds=d["n_lds"], levels=d["n_lev"], storage_mode=d["mode"], iterations=r["iterations"],
                         trials=r["trials"], err=r["err"], err_end=r["err_end"], set_problem_ms=round(set_ms, 3),
                         device_ms_median=round(float(np.median(dev)), 3), device_ms_min=round(float(np.min(dev)), 3),
                         wall_ms_median=round(float(np.median(wall)), 3), runs=a.runs)
        print(name, json.dumps(out[name]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
