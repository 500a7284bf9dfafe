"""MLPnPsolver (src/MLPnPsolver.cpp) on the device, batched: one object holds J independent solvers ("jobs", one per
relocalization candidate keyframe of Tracking::Relocalization, src/Tracking.cc:3543-3730; many frames may share an
object) on one omv_pnp handle (openmavis_amd/csrc/pnp.hip).  The call shape is the reference's: constructor,
SetRansacParameters, iterate.  There is no CPU fallback.

A job is a dict: P2D [N][2] float32 (F.mvKeysUn[i].pt of the correspondences the constructor keeps, in its order),
sigma2 [N] (F.mvLevelSigma2[kp.octave]), Xw [N][3] float32 (pMP->GetWorldPos()), index [N] (mvKeyPointIndices), mN
(vpMapPointMatches.size()), cam [8], model (_lib.CAM_KB8 / CAM_PINHOLE).  select_correspondences() restates the
constructor's graph part on flattened flags.

iterate's loop condition is an OR (:75): a call runs max(nIterations, mRansacMaxIts - mnIterations) hypotheses unless it
returns earlier, so the draws of a call are [J][H][6] with H >= max(nIterations, max(mRansacMaxIts)) on the first call.

Differences from the reference, all deliberate: the decompositions are Jacobi eigen-decompositions in double (the same
pose, not the same bits); Refine's CheckInliers sees the pose Refine computed, and its outcome is evaluated once per
distinct best and kept; the random draws of a call are made up front, so after a return the caller's rand() stream has
advanced further than the reference's."""
import ctypes

import numpy as np

from . import _lib
from .ransac import BatchedRansac

NO_MORE, FOUND = 1, 2
GN_MAXIT, GN_EPSP, GN_BREAK, GN_NAN = 0, 1, 2, 3
MIN_SET = 6


def select_correspondences(has_mp, is_bad, n_keys):
    """The constructor's graph part (:21-27): entry i of vpMapPointMatches is kept if pMP && !pMP->isBad() &&
    i < F.mvKeysUn.size().  has_mp / is_bad [mN] flags; returns mvKeyPointIndices (int32, increasing)."""
    has_mp, is_bad = np.asarray(has_mp, bool), np.asarray(is_bad, bool)
    keep = has_mp & ~is_bad & (np.arange(len(has_mp)) < int(n_keys))
    return np.nonzero(keep)[0].astype(np.int32)


class MLPnPsolver(BatchedRansac):
    K, _CREATE, _DESTROY = MIN_SET, "omv_pnp_create", "omv_pnp_destroy"

    def __init__(self, jobs, max_hyp=300, device="cuda:0", stream=None):
        super().__init__(jobs, "index", "mN", max_hyp, device, stream)
        self.mN, self.T = self._mn, self._T
        self.SetRansacParameters()   # the constructor's last line (:52): the header's defaults

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=6, epsilon=0.4, th2=5.991):
        """Uploads the jobs and resets the carried state; mRansacMaxIts / mRansacMinInliers per job are left in
        self.max_its / self.min_inliers.  Tracking passes (0.99, 10, 300, 6, 0.5, 5.991)."""
        _lib.check(self._set(probability, minInliers, maxIterations, minSet, epsilon, th2), "omv_pnp_set")
        return self

    def _set(self, probability=0.99, minInliers=8, maxIterations=300, minSet=6, epsilon=0.4, th2=5.991):
        """omv_pnp_set on self.jobs; returns the status."""
        J, cat = self.n_jobs, self._cat
        arrs = [self.corr_start, cat("P2D", np.float32, 2), cat("sigma2", np.float32, 1), cat("Xw", np.float32, 3),
                cat("index", np.int32, 1), self.mN, cat("cam", np.float32, 8),
                np.array([j["model"] for j in self.jobs], np.int32)]
        max_its, min_inl = np.zeros(max(J, 1), np.int32), np.zeros(max(J, 1), np.int32)
        status = self._lib.omv_pnp_set(self._h, J, *[_lib.ptr(a) for a in arrs], float(probability), int(minInliers),
                                       int(maxIterations), int(minSet), float(epsilon), float(th2), _lib.ptr(max_its),
                                       _lib.ptr(min_inl), self._stream())
        if status == _lib.OMV_OK:
            self.max_its, self.min_inliers = max_its[:J], min_inl[:J]
        return status

    def iterate(self, nIterations, draws):
        """iterate(nIterations, bNoMore, vbInliers, nInliers, Tout) for every job.  draws: [n_jobs][H][6] int32, host
        array or device tensor; a job runs min(H, max(nIterations, mRansacMaxIts - mnIterations)) hypotheses unless it
        returns earlier.  Returns device tensors (found [J], Tcw [J][4][4], bNoMore [J], vbInliers (flat uint8; job j at
        inl_start[j]), nInliers [J]); nothing is synchronised."""
        draws = self._device_draws(draws)
        J = self.n_jobs
        H = draws.numel() // (J * MIN_SET) if J else 0
        assert draws.numel() == J * H * MIN_SET, "draws: [n_jobs][H][6]"
        _lib.check(self._lib.omv_pnp_iterate(self._h, int(nIterations), int(H), _lib.ptr(draws), _lib.ptr(self.T),
                                             _lib.ptr(self.n_inliers), _lib.ptr(self.inliers), _lib.ptr(self.flags),
                                             self._stream()), "omv_pnp_iterate")
        return ((self.flags[:J] & FOUND) != 0, self.T[:J].view(J, 4, 4), (self.flags[:J] & NO_MORE) != 0, self.inliers,
                self.n_inliers[:J])

    def hypotheses(self, j=0):
        """What job j did in the last iterate call (the library's test hook): dict of host arrays over its H hypotheses
        idx [H][6], planar, its, reason, count [H], R0, R [H][3][3], t0, t [H][3] (float64), mask [H][N] bool, words;
        `refine`: the same keys (hyp, n_in in place of idx) over its Refine calls; `state`: mnIterations, mnBestInliers,
        refined_valid, refined_count, refined_ok, out_kind; `prepared` [N][12]: bearing, nullspace r, s, Xw."""
        H, N = self.max_hyp, int(self.n[j])
        W = (N + 63) // 64
        n_hyp, n_ref = ctypes.c_int32(), ctypes.c_int32()
        hi, hp = np.zeros((H, 10), np.int32), np.zeros((H, 24), np.float64)
        ri, rp = np.zeros((H, 8), np.int32), np.zeros((H, 24), np.float64)
        hw, rw = np.zeros((H, max(W, 1)), np.uint64), np.zeros((H, max(W, 1)), np.uint64)
        state, prep = np.zeros(6, np.int32), np.zeros((max(N, 1), 12), np.float64)
        _lib.check(self._lib.omv_pnp_debug(self._h, int(j), ctypes.byref(n_hyp), _lib.ptr(hi), _lib.ptr(hp), _lib.ptr(hw),
                                           ctypes.byref(n_ref), _lib.ptr(ri), _lib.ptr(rp), _lib.ptr(rw), _lib.ptr(state),
                                           _lib.ptr(prep), self._stream()), "omv_pnp_debug")

        def poses(p, n):
            p = p[:n]
            return dict(R0=p[:, :9].reshape(n, 3, 3), t0=p[:, 9:12], R=p[:, 12:21].reshape(n, 3, 3), t=p[:, 21:24])

        nh, nr = n_hyp.value, n_ref.value
        o = dict(idx=hi[:nh, :6], planar=hi[:nh, 6].astype(bool), its=hi[:nh, 7], reason=hi[:nh, 8], count=hi[:nh, 9],
                 **poses(hp, nh))
        o["mask"], o["words"] = self._unpack(hw, nh, j)
        r = dict(hyp=ri[:nr, 0], n_in=ri[:nr, 1], planar=ri[:nr, 2].astype(bool), its=ri[:nr, 3], reason=ri[:nr, 4],
                 count=ri[:nr, 5], ok=ri[:nr, 6].astype(bool), **poses(rp, nr))
        r["mask"], r["words"] = self._unpack(rw, nr, j)
        o["refine"] = r
        o["state"] = dict(zip(("iterations", "best", "refined_valid", "refined_count", "refined_ok", "out_kind"),
                              (int(x) for x in state)))
        o["prepared"] = prep[:N]
        return o
