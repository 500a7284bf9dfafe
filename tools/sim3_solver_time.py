"""Time Sim3Solver.find on cuda:0 with device events, on the loop-closing shapes: 8 jobs x 100 correspondences x 300
hypotheses, and 1 job x 30 correspondences x 300 hypotheses.  find evaluates every hypothesis of the chunk in one
launch whether or not one of them converges, so the time does not depend on where the convergence falls; minInliers = 6
keeps mRansacMaxIts at 300 for both shapes.  The draws are on the device before the clock starts.  Warmed, repeated;
reports the median and the spread (min .. max) per shape."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_shape(n_jobs, n_corr, reps, warmup, model):
    import numpy as np
    import torch
    from openmavis_amd import synth_sim3solver
    from openmavis_amd.sim3solver import Sim3Solver
    jobs = synth_sim3solver.make_jobs([n_corr] * n_jobs, seed=1, models=(model, model))
    s = Sim3Solver(jobs, max_hyp=300)
    s.SetRansacParameters(0.99, 6, 300)
    n_it = int(s.max_its.max())
    draws = torch.from_numpy(s.draw(np.random.default_rng(2), n_it)).cuda()
    ms = []
    for r in range(warmup + reps):
        s.SetRansacParameters(0.99, 6, 300)   # resets the carried state (synchronises)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.find(draws)
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    conv = int(((s.flags[:n_jobs] & 2) != 0).sum())
    ms = np.array(ms)
    print(f"sim3_solver find: {n_jobs} jobs x {n_corr} correspondences x {n_it} hypotheses, "
          f"{'Pinhole' if model else 'KB8'}, {conv} converged: median {np.median(ms) * 1e3:.1f} us "
          f"(min {ms.min() * 1e3:.1f}, max {ms.max() * 1e3:.1f}, {reps} runs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for model in (0, 1):   # KB8, Pinhole
        time_shape(8, 100, a.reps, a.warmup, model)
        time_shape(1, 30, a.reps, a.warmup, model)


if __name__ == "__main__":
    main()
