"""What tests/sim3_ref.py and tests/mlpnp_ref.py share: the sampling of iterate (Sim3Solver.cc:230-243, MLPnPsolver.cpp:79-98)
as the literal list and as the replay the device evaluates (csrc/omv_ransac.h), SetRansacParameters' tail (ransac_plan.h)."""
import math

import numpy as np


def ransac_its(prob, eps, all_inliers, max_its):
    """mRansacMaxIts from the float epsilon in the reference's types: double pow / log / ceil, int min / max.  A NaN or
    out-of-range double -> int conversion (undefined in C++, INT_MIN on x86) counts as INT_MIN."""
    if all_inliers:
        n_it = 1
    else:
        eps = float(np.float32(eps))
        with np.errstate(all="ignore"):
            e3 = math.pow(eps, 3.0) if np.isfinite(eps) else eps
            v = np.ceil(np.log(np.float64(1 - prob)) / np.log(np.float64(1) - np.float64(e3)))
        n_it = int(v) if np.isfinite(v) and -2 ** 31 <= v < 2 ** 31 else -2 ** 31
    return max(1, min(n_it, max_its))


def sample_literal(n, r, k):
    """The k picks by the literal shrinking list with swap-with-back removal; draws are clamped into their range."""
    avail, out = list(range(n)), []
    for i in range(k):
        ri = min(max(int(r[i]), 0), len(avail) - 1)
        out.append(avail[ri])
        avail[ri] = avail[-1]
        avail.pop()
    return out


def sample_replay(n, r, k):
    """The same picks without the list (what the device evaluates): position p holds the value the latest earlier pick
    that removed from p moved there, else p."""
    pos, val, out = [], [], []
    for i in range(k):
        size = n - i
        ri = min(max(int(r[i]), 0), size - 1)
        at_r, at_back = ri, size - 1
        for pj, vj in zip(pos, val):
            if pj == ri:
                at_r = vj
            if pj == size - 1:
                at_back = vj
        out.append(at_r)
        pos.append(ri)
        val.append(at_back)
    return out
