// The device part of the batched RANSAC frame Sim3Solver (sim3.hip) and MLPnPsolver (pnp.hip) share, and the host
// helpers of it that call the HIP runtime; the layout and the host arithmetic are in ransac_plan.h.  A solver supplies its
// minimal solver, its inlier predicate and its selection rule.
#pragma once
#include <hip/hip_runtime.h>

#include "omv_device.h"
#include "ransac_plan.h"

namespace omv_ransac {

// The i-th pick for i < K from raw draws r_i in [0, n-1-i] (clamped) on the shrinking copy of mvAllIndices = 0 .. n-1
// with swap-with-back removal (Sim3Solver.cc:230-243, MLPnPsolver.cpp:87-98).  The list is not materialised: position p
// of the current list holds the value the latest earlier pick that removed from position p moved there, else p.
template <int K>
__device__ __forceinline__ void replay_sampling(int n, const int32_t *draws, int *idx) {
    int pos[K], val[K];   // pick j removed position pos[j] and wrote the then-back value val[j] there
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int size = n - i, r = min(max(draws[i], 0), size - 1);
        int at_r = r, at_back = size - 1;
#pragma unroll
        for (int j = 0; j < i; j++) {
            if (pos[j] == r) at_r = val[j];
            if (pos[j] == size - 1) at_back = val[j];
        }
        idx[i] = at_r;
        pos[i] = r, val[i] = at_back;
    }
}

// CheckInliers' loop by one wavefront: the lanes stride over the job's n correspondences, inlier(i) judges one, and
// __ballot builds the mask as 64-bit words (word i / 64, bit i % 64) at `mask`.  Returns the count, in every lane.
template <class Pred>
__device__ __forceinline__ int wave_inlier_mask(int n, int lane, unsigned long long *mask, Pred inlier) {
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const unsigned long long m = __ballot(i < n && inlier(i));
        if (lane == 0) mask[base >> 6] = m;
        count += __popcll(m);
    }
    return count;
}

// vbInliers of a job by its (only) wavefront: zeros, then a one at index[.] of every correspondence set in `mask` (the
// job's words; null: none).
__device__ __forceinline__ void wave_scatter_inliers(const JobLayout &jl, int lane, const unsigned long long *mask,
                                                     const int32_t *index, uint8_t *inliers_out) {
    uint8_t *vb = inliers_out + jl.inl_start;
    for (int i = lane; i < jl.mn; i += 64) vb[i] = 0;
    omv::wave_mem_sync();   // the zeros land before the scatter
    if (mask)
        for (int i = lane; i < jl.n; i += 64)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) vb[index[jl.corr_start + i]] = 1;
}

// the argument and device check both `create`s begin with
inline omv_status check_create(const void *out, int max_jobs, int max_corr_total, int max_hyp) {
    if (!out || max_jobs <= 0 || max_corr_total < 0 || max_hyp <= 0) return OMV_ERR_ARG;
    int ndev = 0;
    return hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 ? OMV_ERR_NO_DEVICE : OMV_OK;
}

// the debug hooks' read-back of a job's mask words of `rows` hypothesis rows into dst [rows][ceil(n / 64)] (null: none)
inline hipError_t read_mask_rows(uint64_t *dst, const unsigned long long *d_mask, const JobLayout &jl, int words_total,
                                 int rows, hipStream_t st) {
    const size_t nw = (size_t)(jl.n + 63) / 64;
    if (!dst || !nw || rows <= 0) return hipSuccess;
    return hipMemcpy2DAsync(dst, nw * 8, d_mask + jl.word_start, (size_t)words_total * 8, nw * 8, rows,
                            hipMemcpyDeviceToHost, st);
}

}  // namespace omv_ransac
