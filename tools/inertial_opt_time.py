"""Time one omv_inertial_optimization call on cuda:0: J in {1, 64} jobs of K in {10, 50, 200} keyframes, FULL mode, stereo,
priors (1e2, 1e5) -- the first of LocalMapping::InitializeIMU's three calls -- from synth_inertial's planted problems.
The API takes host arrays and synchronises, so the clock is a host clock round the whole call (packing into the pinned
block, upload, the kernel, read-back); warmed, repeated, the median and the spread reported.  The kernel's own split
comes from the debug hook's tick counters (the device's constant 100 MHz clock, job 0): buildSystem, the linear solves
(the velocity chain's cyclic reduction + the 9 x 9 corner), the trials' error evaluations.
--out profiles/inertial_opt_bench.json keeps the figures."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))


def time_shape(n_jobs, K, reps, warmup):
    import numpy as np
    from openmavis_amd import _lib, inertial_init as ii, synth_inertial as si
    base = si.make_jobs([K] * min(n_jobs, 8), seed=11, modes=(ii.FULL,), monos=(False,), priors=((1e2, 1e5),))
    jobs = [base[j % len(base)] for j in range(n_jobs)]
    opt = ii.InertialOptimizer(n_jobs, n_jobs * K, n_jobs * K)
    ms = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        code, o = opt.run(jobs)
        t1 = time.perf_counter()
        _lib.check(code, "omv_inertial_optimization")
        if r >= warmup:
            ms.append((t1 - t0) * 1e3)
    ms = np.array(ms)
    it, tr = o["iterations"][:n_jobs], o["trials"][:n_jobs]
    d = opt.debug(0)
    ticks = d["ticks"].astype(np.float64) * 1e-2   # 100 MHz -> us
    rec = dict(jobs=n_jobs, keyframes=K, median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
               reps=reps, iterations_per_job=float(it.mean()), trials_per_job=float(tr.mean()),
               us_per_trial=float(np.median(ms) * 1e3 / tr.max()),
               job0=dict(iterations=d["iterations"], trials=d["trials"], build_us=float(ticks[0]), solve_us=float(ticks[1]),
                         trial_errors_us=float(ticks[2]), solve_us_per_trial=float(ticks[1] / max(d["trials"], 1))))
    print(f"inertial_optimization FULL: {n_jobs} jobs x {K} keyframes: median {rec['median_ms']:.3f} ms (min "
          f"{rec['min_ms']:.3f}, max {rec['max_ms']:.3f}, {reps} calls); {rec['iterations_per_job']:.1f} iterations, "
          f"{rec['trials_per_job']:.1f} trials per job, {rec['us_per_trial']:.1f} us per trial of the longest job; job 0 in "
          f"the kernel: build {ticks[0]:.0f} us, solve {ticks[1]:.0f} us, trial errors {ticks[2]:.0f} us")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "inertial_opt_time needs a GPU"
    recs = [time_shape(j, k, a.reps, a.warmup) for j in (1, 64) for k in (10, 50, 200)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/inertial_opt_time.py", device=torch.cuda.get_device_name(0), mode="FULL, stereo",
                           priors=[1e2, 1e5], clock="host clock round the call; job0: device 100 MHz ticks", shapes=recs),
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
