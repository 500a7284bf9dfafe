// The host part of the batched RANSAC frame of Sim3Solver (sim3.hip) and MLPnPsolver (pnp.hip): how J jobs slice the flat
// arrays, the argument checks of `set` in their order, SetRansacParameters' arithmetic.  Nothing here needs the HIP runtime:
// hipcc compiles this text into the product, the host compiler into tests/cpp/ransac_plan_host.cpp.  Device: omv_ransac.h.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/omv.h"

namespace omv_ransac {

// The head of both JobParams: job j has correspondences [corr_start, corr_start + n) of the flat arrays, vbInliers
// [inl_start, inl_start + mn) and mask words [word_start, word_start + ceil(n / 64)) of a hypothesis' row.
struct JobLayout { int corr_start, n, mn, inl_start, word_start; };

// mask words a handle holds per hypothesis row (every job rounds up to whole words)
inline int words_cap(int max_corr, int max_jobs) { return max_corr / 64 + max_jobs; }

// The checks of a `set` call in the order the ABI keeps (the caller's own null pointers came first), then the layout: the
// JobLayout of jobs [n_jobs] (a solver's JobParams), corr_job [n_corr] (the job of a correspondence), words_total.
// job_ok(j): the caller's per-job test (the camera models); data_present: no per-correspondence array (`index`) is null.
template <class Job, class JobOk>
omv_status plan_layout(int n_jobs, const int32_t *corr_start, const int32_t *mN, const int32_t *index, bool data_present,
                       int max_jobs, int max_corr, int words_cap, JobOk job_ok, std::vector<Job> *jobs,
                       std::vector<int32_t> *corr_job, int *words_total) {
    if (n_jobs < 0 || (n_jobs > 0 && (!corr_start || !mN))) return OMV_ERR_ARG;
    if (n_jobs > max_jobs) return OMV_ERR_CAPACITY;
    const int n_corr = n_jobs ? corr_start[n_jobs] : 0;
    if (n_jobs && corr_start[0] != 0) return OMV_ERR_ARG;
    for (int j = 0; j < n_jobs; j++)
        if (corr_start[j + 1] < corr_start[j] || mN[j] < 0 || !job_ok(j)) return OMV_ERR_ARG;
    if (n_corr > max_corr) return OMV_ERR_CAPACITY;
    if (n_corr > 0 && !data_present) return OMV_ERR_ARG;
    jobs->assign(n_jobs, Job()), corr_job->resize(n_corr);
    int inl = 0, words = 0;
    for (int j = 0; j < n_jobs; j++) {
        JobLayout &l = (*jobs)[j];
        l = JobLayout{corr_start[j], corr_start[j + 1] - corr_start[j], mN[j], inl, words};
        for (int i = corr_start[j]; i < corr_start[j + 1]; i++) {
            if (index[i] < 0 || index[i] >= mN[j]) return OMV_ERR_ARG;
            (*corr_job)[i] = j;
        }
        inl += l.mn, words += (l.n + 63) / 64;
    }
    if (words > words_cap) return OMV_ERR_CAPACITY;
    *words_total = words;
    return OMV_OK;
}

// The tail of both SetRansacParameters (Sim3Solver.cc:194-204, MLPnPsolver.cpp:200-213) in the reference's types.  A NaN
// or out-of-range number -> int conversion (undefined; x86 yields INT_MIN) gives INT_MIN, so mRansacMaxIts becomes 1.
inline int ransac_its(double prob, float epsilon, bool all_inliers, int max_its) {
    int n_iterations = 1;
    if (!all_inliers) {
        const double v = ceil(log(1 - prob) / log(1 - pow((double)epsilon, 3.0)));
        n_iterations = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MIN;
    }
    return std::max(1, std::min(n_iterations, max_its));
}

// MLPnPsolver::SetRansacParameters (:177-213): its nMinInliers and epsilon, then the tail
inline void mlpnp_parameters(int N, double prob, int min_inliers, int max_its, int min_set, float epsilon,
                             int *max_its_out, int *min_inliers_out) {
    const float prod = (float)N * epsilon;   // int nMinInliers = N * mRansacEpsilon
    int n_min = (prod >= -2147483648.f && prod < 2147483648.f) ? (int)prod : INT_MIN;
    if (n_min < min_inliers) n_min = min_inliers;
    if (n_min < min_set) n_min = min_set;
    if (epsilon < (float)n_min / N) epsilon = (float)n_min / N;
    *max_its_out = ransac_its(prob, epsilon, n_min == N, max_its);
    *min_inliers_out = n_min;
}

}  // namespace omv_ransac
