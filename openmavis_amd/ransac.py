"""The batched RANSAC frame Sim3Solver and MLPnPsolver share (csrc/ransac_plan.h, omv_ransac.h): J jobs on one handle, each
a slice of the flat correspondence and vbInliers arrays, the draws of a call made up front, the masks as 64-bit words."""
import ctypes

import numpy as np

from . import _lib

RAND_MAX = 2147483647


def draw(rng_or_rand, n_iterations, n, k=3):
    """Raw draws [n_iterations][k] for a job with n correspondences by DUtils::Random::RandomInt's formula
    (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min with
    d = n - i for the i-th pick (k = 3 for Sim3Solver, 6 for MLPnPsolver).  rng_or_rand: a callable returning rand()
    values in [0, RAND_MAX], or a numpy.random.Generator (then rand() is its integers(0, RAND_MAX + 1))."""
    if callable(rng_or_rand):
        r = np.array([[rng_or_rand() for _ in range(k)] for _ in range(n_iterations)], np.float64).reshape(-1, k)
    else:
        r = rng_or_rand.integers(0, RAND_MAX + 1, (n_iterations, k)).astype(np.float64)
    d = np.maximum(n - np.arange(k), 1).astype(np.float64)
    return ((r / (RAND_MAX + 1.0)) * d).astype(np.int32)


class BatchedRansac:
    """A subclass supplies K (picks per hypothesis) and _CREATE / _DESTROY (the handle's entry points), names self._mn
    (mN per job) and self._T (the [J][16] output) as the reference does, and ends its constructor in SetRansacParameters."""

    def __init__(self, jobs, index_key, mn_key, max_hyp, device, stream):
        import torch
        self._torch, self._lib, self.device, self.stream = torch, _lib.load(), device, stream
        self.jobs = list(jobs)
        J = self.n_jobs = len(self.jobs)
        self.n = np.array([len(j[index_key]) for j in self.jobs], np.int32)
        self._mn = np.array([int(j[mn_key]) for j in self.jobs], np.int32)
        self.corr_start = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int32)
        self.inl_start = np.concatenate([[0], np.cumsum(self._mn)]).astype(np.int64)
        self.max_hyp = int(max_hyp)
        self._h = ctypes.c_void_p()
        _lib.check(getattr(self._lib, self._CREATE)(max(J, 1), int(self.corr_start[-1]), self.max_hyp,
                                                    ctypes.byref(self._h)), self._CREATE)
        self._T = torch.zeros((max(J, 1), 16), dtype=torch.float32, device=device)
        self.n_inliers = torch.zeros(max(J, 1), dtype=torch.int32, device=device)
        self.flags = torch.zeros(max(J, 1), dtype=torch.int32, device=device)
        self.inliers = torch.zeros(max(int(self.inl_start[-1]), 1), dtype=torch.uint8, device=device)

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = None

    def _stream(self):
        s = self.stream if self.stream is not None else self._torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def _cat(self, key, dt, width):
        """The jobs' arrays `key` as one contiguous [sum][width] array."""
        if not self.n_jobs:
            return np.zeros((0, width), dt)
        return np.ascontiguousarray(np.concatenate([np.asarray(j[key], dt).reshape(-1, width) for j in self.jobs]))

    def draw(self, rng_or_rand, count):
        """Raw draws [n_jobs][count][K] (int32, host), job after job."""
        return np.stack([draw(rng_or_rand, count, int(n), self.K) for n in self.n]) if self.n_jobs else \
            np.zeros((0, count, self.K), np.int32)

    def _device_draws(self, draws):
        torch = self._torch
        if not torch.is_tensor(draws):
            draws = torch.from_numpy(np.ascontiguousarray(draws, np.int32))
        return draws.to(self.device, torch.int32).contiguous()

    def job_inliers(self, j):
        """vbInliers of job j (host bool [mN])."""
        return self.inliers[int(self.inl_start[j]):int(self.inl_start[j + 1])].cpu().numpy().astype(bool)

    def _unpack(self, words, rows, j):
        """The first `rows` rows of a debug hook's mask words of job j -> (mask [rows][N] bool, words [rows][W])."""
        N, W = int(self.n[j]), (int(self.n[j]) + 63) // 64
        words = words[:rows, :W]
        bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
        return bits.reshape(rows, 64 * W)[:, :N].astype(bool), words
