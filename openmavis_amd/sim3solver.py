"""Sim3Solver (src/Sim3Solver.cc) on the device, batched: one object holds J independent solvers ("jobs", one per loop /
merge candidate pair of LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:812-832) on one omv_sim3_solver
handle (openmavis_amd/csrc/sim3.hip).  The call shape is the reference's: constructor, SetRansacParameters, iterate /
find, GetEstimated*.  There is no CPU fallback.

A job is a dict: Xw1, Xw2 [N][3] float32 (pMP1 / pMP2->GetWorldPos() of the correspondences the constructor keeps, in
its order), sigma2_1, sigma2_2 [N] (mvLevelSigma2[kp.octave] per side), index1 [N] (mvnIndices1), mN1
(vpMatched12.size()), pose1, pose2 [12] (Riw row-major, tiw of the chosen cameras), cam1, cam2 [8], model1, model2
(_lib.CAM_KB8 / CAM_PINHOLE), fix_scale.  select_correspondences() restates the constructor's graph part, which picks
the camera pair and the correspondences, on flattened GetIndexInKeyFrame tuples.

Differences from the reference, all deliberate: ComputeSim3's eigenvector step is a Jacobi in double (the same rotation,
not the same bits); the 5-argument iterate returns the carried mBestT12 where the reference returns an uninitialised
matrix; the random draws of a call are made up front, so after a convergence the caller's rand() stream has advanced
further than the reference's; SetRansacParameters also resets mnBestInliers."""
import ctypes

import numpy as np

from . import _lib
from .ransac import RAND_MAX, BatchedRansac, draw   # RAND_MAX and draw stay importable from here

NO_MORE, CONVERGE = 1, 2


def select_correspondences(indices1, indices2, valid=None):
    """The constructor's graph part (:57-117, :125-149).  indices1 / indices2 [mN1][4]: per entry i1 of vpMatched12 the
    tuple pMP1->GetIndexInKeyFrame(pKF1) / pMP2->GetIndexInKeyFrame(pKFm) (-1: not seen by that camera); valid [mN1]:
    vpMatched12[i1] && pMP1 && !pMP1->isBad() && !pMP2->isBad().  Every (c1, c2) with both indices >= 0 gets a vote; the
    winner is camPairsCountVec[0] after std::sort by descending count -- at most 16 entries, so libstdc++ runs a plain
    insertion sort, which is stable: among equal counts the pair first in std::map order (lexicographic) wins.
    Returns (cameraID1, cameraID2, mvnIndices1, indexKF1, indexKF2), or None when no pair has a vote (mState = false)."""
    i1 = np.asarray(indices1, np.int64).reshape(-1, 4)
    i2 = np.asarray(indices2, np.int64).reshape(-1, 4)
    ok = np.ones(len(i1), bool) if valid is None else np.asarray(valid, bool)
    votes = ((i1[ok][:, :, None] >= 0) & (i2[ok][:, None, :] >= 0)).sum(0)   # [c1][c2]
    if votes.sum() == 0:
        return None
    pairs = [(c1, c2) for c1 in range(4) for c2 in range(4) if votes[c1, c2] > 0]   # std::map order
    c1, c2 = sorted(pairs, key=lambda p: -votes[p])[0]   # Python's sort is stable, like the insertion sort
    keep = ok & (i1[:, c1] >= 0) & (i2[:, c2] >= 0)
    idx = np.nonzero(keep)[0].astype(np.int32)
    return int(c1), int(c2), idx, i1[idx, c1].astype(np.int32), i2[idx, c2].astype(np.int32)


def to_sim3f(R, t, s):
    """(S12, S21) as the omv_sim3f dicts ORBmatcher.SearchBySim3 takes (q = unit quaternion (x, y, z, w) * sqrt(scale),
    scale = |q|^2 in float), from GetEstimatedRotation / Translation / Scale: S12 = (R, t, s), S21 its inverse."""
    from .synth import quat_from_R

    def one(R, t, s):
        q = (quat_from_R(np.asarray(R, np.float64)) * np.sqrt(s)).astype(np.float32)
        scale = np.float32(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        return dict(q=q, t=np.asarray(t, np.float32), scale=scale)

    R, t, s = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64), float(s)
    return one(R, t, s), one(R.T, -(R.T @ t) / s, 1.0 / s)


class Sim3Solver(BatchedRansac):
    K, _CREATE, _DESTROY = 3, "omv_sim3_solver_create", "omv_sim3_solver_destroy"

    def __init__(self, jobs, max_hyp=300, device="cuda:0", stream=None):
        super().__init__(jobs, "index1", "mN1", max_hyp, device, stream)
        self.mN1, self.T12 = self._mn, self._T
        self.SetRansacParameters()   # the constructor's last line (:181): 0.99, 6, 300

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """minInliers: one value or one per job.  Uploads the jobs and resets the carried state; mRansacMaxIts per job is
        left in self.max_its."""
        _lib.check(self._set(probability, minInliers, maxIterations), "omv_sim3_solver_set")
        return self

    def _set(self, probability, minInliers, maxIterations):
        """omv_sim3_solver_set on self.jobs; returns the status."""
        J = self.n_jobs
        mi = np.broadcast_to(np.asarray(minInliers, np.int32), (J,)).copy()
        cat = self._cat
        arrs = [self.corr_start, cat("Xw1", np.float32, 3), cat("Xw2", np.float32, 3), cat("sigma2_1", np.float32, 1),
                cat("sigma2_2", np.float32, 1), cat("index1", np.int32, 1), self.mN1, cat("pose1", np.float32, 12),
                cat("pose2", np.float32, 12), cat("cam1", np.float32, 8), cat("cam2", np.float32, 8),
                np.array([j["model1"] for j in self.jobs], np.int32), np.array([j["model2"] for j in self.jobs], np.int32),
                np.array([int(bool(j["fix_scale"])) for j in self.jobs], np.int32)]
        max_its = np.zeros(max(J, 1), np.int32)
        status = self._lib.omv_sim3_solver_set(self._h, J, *[_lib.ptr(a) for a in arrs], float(probability),
                                               _lib.ptr(mi), int(maxIterations), _lib.ptr(max_its), self._stream())
        if status == _lib.OMV_OK:
            self.max_its, self.min_inliers = max_its[:J], mi
        return status

    def iterate(self, nIterations, draws):
        """The 5-argument iterate for every job.  draws: [n_jobs][nIterations][3] int32, host array or device tensor.
        Returns device tensors (T12 [J][4][4], bNoMore [J], vbInliers (flat uint8; job j at inl_start[j]), nInliers [J],
        bConverge [J]); nothing is synchronised."""
        draws = self._device_draws(draws)
        assert draws.numel() == self.n_jobs * nIterations * 3, "draws: [n_jobs][nIterations][3]"
        _lib.check(self._lib.omv_sim3_solver_iterate(self._h, int(nIterations), _lib.ptr(draws), _lib.ptr(self.T12),
                                                     _lib.ptr(self.n_inliers), _lib.ptr(self.inliers),
                                                     _lib.ptr(self.flags), self._stream()), "omv_sim3_solver_iterate")
        J = self.n_jobs
        return (self.T12[:J].view(J, 4, 4), (self.flags[:J] & NO_MORE) != 0, self.inliers, self.n_inliers[:J],
                (self.flags[:J] & CONVERGE) != 0)

    def find(self, draws):
        """find(vbInliers12, nInliers) = the 4-argument iterate(mRansacMaxIts): identity unless the job converged.
        draws: [n_jobs][max(mRansacMaxIts)][3].  Returns (T12 [J][4][4], vbInliers, nInliers), device tensors."""
        n_it = int(self.max_its.max()) if self.n_jobs else 0
        T12, _, vb, n, conv = self.iterate(n_it, draws)
        eye = self._torch.eye(4, dtype=T12.dtype, device=T12.device).expand_as(T12)
        return self._torch.where(conv[:, None, None], T12, eye), vb, n

    def _best(self, j):
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        s, nb, it = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.omv_sim3_solver_best(self._h, int(j), _lib.ptr(R), _lib.ptr(t), ctypes.byref(s),
                                                  ctypes.byref(nb), ctypes.byref(it), self._stream()),
                   "omv_sim3_solver_best")
        return R.reshape(3, 3), t, np.float32(s.value), int(nb.value), int(it.value)

    def GetEstimatedRotation(self, j=0):
        return self._best(j)[0]

    def GetEstimatedTranslation(self, j=0):
        return self._best(j)[1]

    def GetEstimatedScale(self, j=0):
        return self._best(j)[2]

    def best_inliers_and_iterations(self, j=0):
        """(mnBestInliers, mnIterations) of job j."""
        return self._best(j)[3:]

    def hypotheses(self, j=0):
        """The hypotheses job j evaluated in the last iterate call (the library's test hook): dict of host arrays idx
        [H][3], R [H][3][3], t [H][3], s [H], T12, T21 [H][4][4], count [H], mask [H][N] bool."""
        H, W = self.max_hyp, (int(self.n[j]) + 63) // 64
        n_hyp = ctypes.c_int32()
        o = dict(idx=np.zeros((H, 3), np.int32), R=np.zeros((H, 3, 3), np.float32), t=np.zeros((H, 3), np.float32),
                 s=np.zeros(H, np.float32), T12=np.zeros((H, 4, 4), np.float32), T21=np.zeros((H, 4, 4), np.float32),
                 count=np.zeros(H, np.int32))
        words = np.zeros((H, max(W, 1)), np.uint64)
        _lib.check(self._lib.omv_sim3_solver_debug(self._h, int(j), ctypes.byref(n_hyp), *[
            _lib.ptr(o[k]) for k in ("idx", "R", "t", "s", "T12", "T21", "count")], _lib.ptr(words), self._stream()),
            "omv_sim3_solver_debug")
        o = {k: v[:n_hyp.value] for k, v in o.items()}
        o["mask"], o["words"] = self._unpack(words, n_hyp.value, j)
        return o
