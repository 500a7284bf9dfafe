"""Time one OptimizeSim3 call on cuda:0 on the loop-closing shapes: 8 jobs x 100 pairs and 1 job x 100 pairs (20 %
gross outliers, the start value a disturbed planted similarity).  The call takes host arrays and returns host results,
so the timed window is a host clock around it: the uploads, the one kernel launch, the read-back and the stream
synchronise it ends in (what a caller waits for).  The packing of the job dicts into flat arrays happens before the
clock starts.  Warmed, repeated; reports the median and the spread (min .. max) per shape, and the LM work done."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_shape(n_jobs, n_pairs, reps, warmup, model):
    import numpy as np
    import torch
    from openmavis_amd import _lib, synth_optsim3
    from openmavis_amd.optimizer import Sim3Optimizer
    assert torch.cuda.is_available(), "needs a GPU"
    jobs = synth_optsim3.make_jobs([n_pairs] * n_jobs, seed=1, models=(model, model))
    opt = Sim3Optimizer(n_jobs, n_jobs * n_pairs)
    lib = _lib.load()
    start = np.arange(n_jobs + 1, dtype=np.int32) * n_pairs

    def cat(key, dt, width):
        return np.ascontiguousarray(np.concatenate([np.asarray(j[key], dt).reshape(-1, width) for j in jobs]))

    arrays = [cat(k, dt, w) for k, dt, w in Sim3Optimizer._ENTRY + Sim3Optimizer._JOB]
    S0 = [cat("q", np.float64, 4), cat("t", np.float64, 3), cat("s", np.float64, 1)]
    n_in, status = np.zeros(n_jobs, np.int32), np.zeros(n_jobs * n_pairs, np.uint8)
    ptrs = [_lib.ptr(a) for a in arrays]
    ms = []
    for r in range(warmup + reps):
        S = [a.copy() for a in S0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        code = lib.omv_optimize_sim3(opt._h, n_jobs, _lib.ptr(start), *ptrs, *[_lib.ptr(a) for a in S], _lib.ptr(n_in),
                                     _lib.ptr(status), opt._stream())
        t1 = time.perf_counter()
        _lib.check(code, "omv_optimize_sim3")
        if r >= warmup:
            ms.append((t1 - t0) * 1e3)
    opt.n = np.full(n_jobs, n_pairs, np.int32)
    dbg = [opt.debug(j) for j in range(n_jobs)]
    its = sum(int(d["iterations"].sum()) for d in dbg)
    trials = sum(int(d["trials"].sum()) for d in dbg)
    ms = np.array(ms)
    print(f"optimize_sim3: {n_jobs} jobs x {n_pairs} pairs, {'Pinhole' if model else 'KB8'}, nIn {n_in.tolist()}, "
          f"{its} LM iterations and {trials} trials over the jobs: median {np.median(ms) * 1e3:.1f} us "
          f"(min {ms.min() * 1e3:.1f}, max {ms.max() * 1e3:.1f}, {reps} runs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for model in (0, 1):   # KB8, Pinhole
        time_shape(8, 100, a.reps, a.warmup, model)
        time_shape(1, 100, a.reps, a.warmup, model)


if __name__ == "__main__":
    main()
