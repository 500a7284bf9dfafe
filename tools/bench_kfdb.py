"""Time the device KeyFrameDatabase on cuda:0 at a loop-closing size: 4,096 keyframes of about 1,200 words each in a
100,000-word synthetic vocabulary (seeded, made here; nothing is read from outside the repository).

  detect_n_best   1 and 16 queries per call (revisits of database keyframes: 70 % of a keyframe's words plus new ones),
                  ten neighbours per keyframe, a fresh query id per query so every call lists and scores.  The call is
                  asynchronous, so a window of `--calls` back-to-back calls is timed with device events and divided;
                  `--reps` windows give the median and the spread.  (query, slot) pairs/s = queries x occupied slots
                  over the time of one call.
  add             16 keyframes into free slots (erased again outside the clock).  add synchronises, so the window is a
                  host clock around the call.

Prints one JSON line per measurement and, with --out, writes them to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_bows(rng, n, n_words, length):
    import numpy as np
    bw = np.full((n, length), -1, np.int32)
    bv = np.zeros((n, length), np.float64)
    bn = np.zeros(n, np.int32)
    for i in range(n):
        w = np.unique(rng.integers(0, n_words, length + length // 16))
        w = np.sort(rng.permutation(w)[:length])
        v = rng.uniform(0.5, 5.0, len(w))
        bw[i, :len(w)], bv[i, :len(w)], bn[i] = w, v / v.sum(), len(w)
    return bw, bv, bn


def revisits(rng, bw, bn, n_q, n_words):
    import numpy as np
    length = bw.shape[1]
    qw = np.full((n_q, length), -1, np.int32)
    qv = np.zeros((n_q, length), np.float64)
    qn = np.zeros(n_q, np.int32)
    for j in range(n_q):
        src = int(rng.integers(0, len(bw)))
        keep = bw[src, :bn[src]][rng.random(bn[src]) < 0.7]
        w = np.unique(np.concatenate([keep, rng.integers(0, n_words, length - len(keep))]))[:length]
        v = rng.uniform(0.5, 5.0, len(w))
        qw[j, :len(w)], qv[j, :len(w)], qn[j] = w, v / v.sum(), len(w)
    return qw, qv, qn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=4096)
    ap.add_argument("--words", type=int, default=1200)
    ap.add_argument("--vocabulary", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from openmavis_amd.kfdb import KeyFrameDatabase
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.Generator(np.random.PCG64(1))
    K, L, V = a.keyframes, a.words, a.vocabulary
    bw, bv, bn = make_bows(rng, K + 16, V, L)
    t = [torch.from_numpy(x).cuda() for x in (bw, bv, bn)]
    db = KeyFrameDatabase(0, max_kf=K + 16, max_bow=L, max_queries=16)
    slots = np.arange(K, dtype=np.int32)
    db.add(slots, (slots >= K * 3 // 4).astype(np.int32), t[0][:K], t[1][:K], t[2][:K])   # a quarter in a second map
    db.set_neighbours(slots, [np.clip(np.r_[s - 5:s, s + 1:s + 6], 0, K - 1) for s in slots])
    results = []
    next_id = 1
    for n_q in (1, 16):
        q = [torch.from_numpy(x).cuda() for x in revisits(rng, bw[:K], bn[:K], n_q, V)]
        conn = [rng.choice(K, 15, replace=False).astype(np.int32) for _ in range(n_q)]
        maps = np.zeros(n_q, np.int32)
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                ids = np.arange(next_id, next_id + n_q)
                next_id += n_q
                out = db.DetectNBestCandidates(ids, maps, conn, *q, 3)
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1) / a.calls)
        d = db.debug(n_q - 1)
        ms = np.array(ms)
        med = float(np.median(ms))
        results.append(dict(what="detect_n_best", queries=n_q, keyframes=K, words=L, vocabulary=V,
                            listed_last_query=int(len(d["list_slot"])), scored_last_query=int(len(d["scored_slot"])),
                            n_loop=out[1].tolist(), n_merge=out[3].tolist(), calls_per_window=a.calls, windows=a.reps,
                            ms_per_call_median=med, ms_per_call_min=float(ms.min()), ms_per_call_max=float(ms.max()),
                            pairs_per_s=n_q * K / (med * 1e-3)))
        print(json.dumps(results[-1]), flush=True)
    extra = np.arange(K, K + 16, dtype=np.int32)
    ms = []
    for r in range(a.warmup + 30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db.add(extra, np.zeros(16, np.int32), t[0][K:], t[1][K:], t[2][K:])
        t1 = time.perf_counter()
        db.erase(extra)
        if r >= a.warmup:
            ms.append((t1 - t0) * 1e3)
    ms = np.array(ms)
    results.append(dict(what="add", keyframes=16, words=L, runs=len(ms), ms_per_call_median=float(np.median(ms)),
                        ms_per_call_min=float(ms.min()), ms_per_call_max=float(ms.max())))
    print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
