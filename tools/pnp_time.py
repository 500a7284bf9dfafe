"""Time MLPnPsolver.iterate on cuda:0 with device events, on the relocalization shape: J in {1, 16, 256} jobs of N = 200
correspondences (40 % outliers) with Tracking's parameters (0.99, 10, 300, 6, 0.5, 5.991), the first iterate(5) of a
job, which runs the whole RANSAC through the OR of its loop condition: mRansacMaxIts = 35 hypotheses per job in one
launch whether or not one of them returns, then the selection with its Refine calls.  The draws are on the device
before the clock starts; SetRansacParameters (which resets the carried state and synchronises) is outside the window.
Warmed, repeated; reports the median and the spread of the whole call (both kernels) per shape.
--out profiles/pnp_bench.json keeps the figures."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_shape(n_jobs, n_corr, reps, warmup, inner):
    import numpy as np
    import torch
    from openmavis_amd import synth_pnp
    from openmavis_amd.pnpsolver import MLPnPsolver
    base = synth_pnp.make_jobs([n_corr] * min(n_jobs, 16), seed=1, models=[j % 2 for j in range(min(n_jobs, 16))],
                               scenes="centred", noise_px=0.5, outlier_share=0.4, depth=(2.0, 6.0))
    jobs = [base[j % len(base)] for j in range(n_jobs)]
    s = MLPnPsolver(jobs, max_hyp=300)
    params = (0.99, 10, 300, 6, 0.5, 5.991)
    s.SetRansacParameters(*params)
    n_draws = int(s.max_its.max())
    draws = torch.from_numpy(s.draw(np.random.default_rng(2), n_draws)).cuda()
    ms = []
    for r in range(warmup + reps):
        tot = 0.0
        for _ in range(inner):   # a window of `inner` calls, each on a fresh state
            s.SetRansacParameters(*params)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.iterate(5, draws)
            e1.record()
            e1.synchronize()
            tot += e0.elapsed_time(e1)
        if r >= warmup:
            ms.append(tot / inner)
    found = int(((s.flags[:n_jobs] & 2) != 0).sum())
    refines = sum(len(s.hypotheses(j)["refine"]["hyp"]) for j in range(min(n_jobs, 16)))
    ms = np.array(ms)
    rec = dict(jobs=n_jobs, correspondences=n_corr, hypotheses_per_job=n_draws, found=found,
               refine_calls_first_16_jobs=refines, median_us=float(np.median(ms) * 1e3), min_us=float(ms.min() * 1e3),
               max_us=float(ms.max() * 1e3), reps=reps, calls_per_rep=inner,
               us_per_job=float(np.median(ms) * 1e3 / n_jobs))
    print(f"pnp iterate(5): {n_jobs} jobs x {n_corr} correspondences x {n_draws} hypotheses, {found} found: median "
          f"{rec['median_us']:.1f} us (min {rec['min_us']:.1f}, max {rec['max_us']:.1f}, {reps} x {inner} calls), "
          f"{rec['us_per_job']:.1f} us per job")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "pnp_time needs a GPU"
    recs = [time_shape(j, 200, a.reps, a.warmup, a.inner) for j in (1, 16, 256)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/pnp_time.py", device=torch.cuda.get_device_name(0), parameters="Tracking",
                           shapes=recs), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
