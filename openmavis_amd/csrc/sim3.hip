// MI355X-native Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): the Horn RANSAC LoopClosing runs per loop /
// merge candidate (src/LoopClosing.cc:812-832), batched over J independent solvers ("jobs") that share one handle.
//
//   sim3_prepare_kernel     the constructor's per-correspondence part (:125-179): X3Dc = Riw Xw + tiw (float, 3-term
//                           sums left to right, no contraction), the image points through omv::cam_project_f, and the
//                           thresholds.  mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:73-74): 9.210 * sigma2
//                           (double) truncated to an unsigned integer, converted to float where it is compared.
//   sim3_hypothesis_kernel  ComputeSim3 + CheckInliers (:360-479): one wavefront per (job, hypothesis), four per block.
//                           The sampling is replayed from the caller's raw draws (the swap-with-back removal of
//                           :230-243 is O(1) integer logic); Horn's steps 1-3 and 5-8 in float as the reference forms
//                           them; step 4 (the eigenvector of the largest eigenvalue of the symmetric 4 x 4 N) by a
//                           cyclic Jacobi in double with a fixed sweep bound, then quaternion -> R in double, rounded
//                           to float.  Every lane computes the solve (wave-uniform); the lanes then stride over the
//                           job's correspondences, and __ballot builds the inlier mask as 64-bit words.
//   sim3_select_kernel      the sequential rule of iterate (:298-345) over the chunk's counts, one wavefront per job:
//                           a prefix maximum per 64 hypotheses finds the ones that become best (count >= mnBestInliers,
//                           ties replace) and the first of those with count > mRansacMinInliers; the carried state
//                           (mnIterations, mnBestInliers, the best T12 / R / t / s / mask) lives on the device.
//
// Not bit-exact with the reference: Eigen::EigenSolver<Matrix4f> + atan2 + SO3f::exp are replaced by the Jacobi (the
// same rotation mathematically); tests/test_sim3solver_gpu.py bounds the difference by the problem's conditioning.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/omv.h"
#include "omv_camera.h"
#include "omv_device.h"
#include "omv_host.h"
#include "omv_ransac.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kFlagNoMore = 1, kFlagConverge = 2;

struct JobParams : omv_ransac::JobLayout {   // mn: mN1
    int min_inliers, max_its, fix_scale, model1, model2;
    float pose1[12], pose2[12];   // Riw row-major, tiw
    float cam1[8], cam2[8];
};
static_assert(sizeof(JobParams) == 50 * 4, "the layout is the head, nothing is padded");

struct JobState {
    int iterations, best_inliers, flags, last_chunk, n_inliers;
    float T12[16], R[9], t[3], s;   // mBestT12, mBestRotation, mBestTranslation, mBestScale
};

// Riw X + tiw as Eigen evaluates the fixed-size product: each row a 3-term sum left to right, then the translation
__device__ __forceinline__ void rt_apply(const float *R, const float *t, const float *X, float *Y) {
#pragma unroll
    for (int i = 0; i < 3; i++) Y[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i];
}

// 3x4 top of a row-major 4x4: Rcw X + tcw (Sim3Solver::Project)
__device__ __forceinline__ void t44_apply(const float *T, const float *X, float *Y) {
#pragma unroll
    for (int i = 0; i < 3; i++) Y[i] = ((T[4 * i] * X[0] + T[4 * i + 1] * X[1]) + T[4 * i + 2] * X[2]) + T[4 * i + 3];
}

__global__ void __launch_bounds__(256) sim3_prepare_kernel(const JobParams *jobs, int n_corr, const int32_t *corr_job,
                                                           const float *Xw1, const float *Xw2, const float *sigma2_1,
                                                           const float *sigma2_2, float *X1, float *X2, float *P1, float *P2,
                                                           float *e1, float *e2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_corr) return;
    const JobParams &jp = jobs[corr_job[i]];
    float a[3], b[3], Y1[3], Y2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = Xw1[3 * i + k], b[k] = Xw2[3 * i + k];
    rt_apply(jp.pose1, jp.pose1 + 9, a, Y1);
    rt_apply(jp.pose2, jp.pose2 + 9, b, Y2);
    float u, v;
    omv::cam_project_f(jp.model1, jp.cam1, Y1, u, v);
    P1[2 * i] = u, P1[2 * i + 1] = v;
    omv::cam_project_f(jp.model2, jp.cam2, Y2, u, v);
    P2[2 * i] = u, P2[2 * i + 1] = v;
#pragma unroll
    for (int k = 0; k < 3; k++) X1[3 * i + k] = Y1[k], X2[3 * i + k] = Y2[k];
    // mvnMaxError.push_back(9.210 * sigmaSquare): double -> size_t (truncation), compared as float
    e1[i] = (float)(unsigned long long)(9.210 * (double)sigma2_1[i]);
    e2[i] = (float)(unsigned long long)(9.210 * (double)sigma2_2[i]);
}

// One Jacobi rotation of the symmetric a (full storage) in the (P, Q) plane, accumulated into the eigenvector columns v.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
    for (int k = 0; k < 4; k++) {   // A <- A J
        const double akp = a[k][P], akq = a[k][Q];
        a[k][P] = c * akp - s * akq;
        a[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {   // A <- J^T A
        const double apk = a[P][k], aqk = a[Q][k];
        a[P][k] = c * apk - s * aqk;
        a[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// The unit eigenvector (w, x, y, z) of the largest eigenvalue of the symmetric 4 x 4 `a` (destroyed): cyclic Jacobi,
// at most kSweeps sweeps, ended early once the off-diagonal mass is below 1e-34 of the matrix's.  Any comparison with a
// NaN ends the loop, so the routine terminates for every input (a NaN matrix returns the first unit vector).
constexpr int kSweeps = 16;
__device__ __forceinline__ void jacobi4_top_eigenvector(double (&a)[4][4], double *q) {
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] +
                           a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (!(off > 1e-34 * (dia + 2.0 * off))) break;
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<0, 3>(a, v);
        jacobi_rotate<1, 2>(a, v);
        jacobi_rotate<1, 3>(a, v);
        jacobi_rotate<2, 3>(a, v);
    }
    double best = a[0][0];   // eval.maxCoeff(&maxIndex): the first maximum
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = v[k][0];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const bool g = a[i][i] > best;
        best = g ? a[i][i] : best;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = g ? v[k][i] : q[k];
    }
}

__global__ void __launch_bounds__(64 * kWavesPerBlock)
    sim3_hypothesis_kernel(const JobParams *jobs, const JobState *state, int n_jobs, int n_it, const int32_t *draws,
                           const float *X1, const float *X2, const float *P1, const float *P2, const float *e1,
                           const float *e2, int words_total, int32_t *h_idx, float *h_T12, float *h_T21, float *h_R,
                           float *h_t, float *h_s, int32_t *h_count, unsigned long long *h_mask) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= n_jobs * n_it) return;
    const int job = g / n_it, hyp = g - job * n_it;
    const JobParams &jp = jobs[job];
    const JobState &js = state[job];
    if (js.flags != 0 || hyp >= min(n_it, jp.max_its - js.iterations)) return;
    const int n = jp.n, c0 = jp.corr_start;
    int idx[3];
    omv_ransac::replay_sampling<3>(n, draws + 3 * (size_t)g, idx);

    // ---- ComputeSim3 (wave-uniform) ----
    float p1[3][3], p2[3][3];   // [row][col]: column i = the i-th picked point (P3Dc1i, P3Dc2i)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) p1[r][i] = X1[3 * (size_t)(c0 + idx[i]) + r], p2[r][i] = X2[3 * (size_t)(c0 + idx[i]) + r];
    float O1[3], O2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {   // ComputeCentroid: the row sum / P.cols(), then the relative coordinates
        O1[r] = ((p1[r][0] + p1[r][1]) + p1[r][2]) / 3.f;
        O2[r] = ((p2[r][0] + p2[r][1]) + p2[r][2]) / 3.f;
#pragma unroll
        for (int i = 0; i < 3; i++) p1[r][i] = p1[r][i] - O1[r], p2[r][i] = p2[r][i] - O2[r];
    }
    float M[3][3];   // M = Pr2 Pr1^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (p2[i][0] * p1[j][0] + p2[i][1] * p1[j][1]) + p2[i][2] * p1[j][2];
    double a[4][4];   // the ten entries in float as the reference forms them, then Matrix4f N
    a[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    a[0][1] = M[1][2] - M[2][1];
    a[0][2] = M[2][0] - M[0][2];
    a[0][3] = M[0][1] - M[1][0];
    a[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    a[1][2] = M[0][1] + M[1][0];
    a[1][3] = M[2][0] + M[0][2];
    a[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    a[2][3] = M[1][2] + M[2][1];
    a[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
        for (int j = 0; j < i; j++) a[i][j] = a[j][i];
    double q[4];
    jacobi4_top_eigenvector(a, q);
    float R[3][3];
    {
        const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
        R[0][0] = (float)(1.0 - 2.0 * (y * y + z * z)), R[0][1] = (float)(2.0 * (x * y - w * z));
        R[0][2] = (float)(2.0 * (x * z + w * y)), R[1][0] = (float)(2.0 * (x * y + w * z));
        R[1][1] = (float)(1.0 - 2.0 * (x * x + z * z)), R[1][2] = (float)(2.0 * (y * z - w * x));
        R[2][0] = (float)(2.0 * (x * z - w * y)), R[2][1] = (float)(2.0 * (y * z + w * x));
        R[2][2] = (float)(1.0 - 2.0 * (x * x + y * y));
    }
    float s = 1.0f;
    if (!jp.fix_scale) {   // P3 = R Pr2; nom = sum(Pr1 .* P3), den = sum(P3 .* P3): float sums, the quotient in double
        float nom = 0.f, den = 0.f;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p3 = (R[i][0] * p2[0][j] + R[i][1] * p2[1][j]) + R[i][2] * p2[2][j];
                nom = nom + p1[i][j] * p3;
                den = den + p3 * p3;
            }
        s = (float)((double)nom / (double)den);
    }
    float T12[16], T21[16], t12[3];
    const float sinv = (float)(1.0 / (double)s);
#pragma unroll
    for (int i = 0; i < 3; i++) {   // t12 = O1 - (s R) O2
        t12[i] = O1[i] - (((s * R[i][0]) * O2[0] + (s * R[i][1]) * O2[1]) + (s * R[i][2]) * O2[2]);
#pragma unroll
        for (int j = 0; j < 3; j++) T12[4 * i + j] = s * R[i][j], T21[4 * i + j] = sinv * R[j][i];
        T12[4 * i + 3] = t12[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)   // tinv = -sRinv t12
        T21[4 * i + 3] = ((-T21[4 * i]) * t12[0] + (-T21[4 * i + 1]) * t12[1]) + (-T21[4 * i + 2]) * t12[2];
    T12[12] = T12[13] = T12[14] = 0.f, T12[15] = 1.f;
    T21[12] = T21[13] = T21[14] = 0.f, T21[15] = 1.f;

    // ---- CheckInliers: the lanes stride over the correspondences ----
    unsigned long long *mask = h_mask + (size_t)hyp * words_total + jp.word_start;
    const int count = omv_ransac::wave_inlier_mask(n, lane, mask, [&](int i) {
        const size_t c = (size_t)(c0 + i);
        float xa[3] = {X1[3 * c], X1[3 * c + 1], X1[3 * c + 2]}, xb[3] = {X2[3 * c], X2[3 * c + 1], X2[3 * c + 2]};
        float Y[3], u, v;
        t44_apply(T12, xb, Y);   // vP2im1 = project(T12 X3Dc2) with camera 1
        omv::cam_project_f(jp.model1, jp.cam1, Y, u, v);
        const float d1x = P1[2 * c] - u, d1y = P1[2 * c + 1] - v;
        t44_apply(T21, xa, Y);   // vP1im2 = project(T21 X3Dc1) with camera 2
        omv::cam_project_f(jp.model2, jp.cam2, Y, u, v);
        const float d2x = u - P2[2 * c], d2y = v - P2[2 * c + 1];
        const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
        return err1 < e1[c] && err2 < e2[c];   // false for a NaN, as in the reference
    });
    const size_t o = (size_t)g;
    // the per-hypothesis record: written by lane 0 (a few dozen words)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) h_T12[16 * o + k] = T12[k], h_T21[16 * o + k] = T21[k];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) h_R[9 * o + 3 * i + j] = R[i][j];
            h_t[3 * o + i] = t12[i];
            h_idx[3 * o + i] = idx[i];
        }
        h_s[o] = s;
        h_count[o] = count;
    }
}

// One wavefront per job: the sequential part of iterate over the chunk, then the call's outputs from the carried state.
__global__ void __launch_bounds__(64)
    sim3_select_kernel(const JobParams *jobs, JobState *state, int n_it, int words_total, const int32_t *h_count,
                       const float *h_T12, const float *h_R, const float *h_t, const float *h_s,
                       const unsigned long long *h_mask, unsigned long long *best_mask, const int32_t *index1,
                       float *T12_out, int32_t *n_inliers_out, uint8_t *inliers_out, int32_t *flags_out) {
    const int job = blockIdx.x, lane = threadIdx.x;
    const JobParams &jp = jobs[job];
    JobState &js = state[job];
    const int n_words = (jp.n + 63) >> 6;
    int flags = js.flags;
    if (flags == 0) {
        const int it0 = js.iterations, chunk = min(n_it, jp.max_its - it0);
        int best = js.best_inliers, chosen = -1, done = 0, converged = 0;
        for (int base = 0; base < chunk && !converged; base += 64) {
            const int h = base + lane;
            const int c = h < chunk ? h_count[(size_t)job * n_it + h] : -1;
            int pm = c;   // inclusive prefix maximum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(pm, d);
                if (lane >= d) pm = max(pm, o);
            }
            int before = __shfl_up(pm, 1);   // the running best when this hypothesis is judged
            before = lane == 0 ? best : max(best, before);
            const bool becomes = h < chunk && c >= before;
            const unsigned long long mb = __ballot(becomes), mc = __ballot(becomes && c > jp.min_inliers);
            if (mc) {
                const int f = __ffsll(mc) - 1;
                chosen = base + f, converged = 1, done = base + f + 1;
            } else {
                if (mb) chosen = base + 63 - __clzll(mb);
                done = min(chunk, base + 64);
            }
            if (mb) best = __shfl(c, chosen - base);
        }
        flags = converged ? kFlagConverge : 0;
        if (!converged && it0 + done >= jp.max_its) flags |= kFlagNoMore;
        if (chosen >= 0) {   // mBestT12 / mBestRotation / mBestTranslation / mBestScale / mvbBestInliers
            const size_t o = (size_t)job * n_it + chosen;
            if (lane < 16) js.T12[lane] = h_T12[16 * o + lane];
            if (lane < 9) js.R[lane] = h_R[9 * o + lane];
            if (lane < 3) js.t[lane] = h_t[3 * o + lane];
            if (lane == 0) js.s = h_s[o];
            for (int w = lane; w < n_words; w += 64)
                best_mask[jp.word_start + w] = h_mask[(size_t)chosen * words_total + jp.word_start + w];
        }
        if (lane == 0) {
            js.iterations = it0 + done, js.best_inliers = best, js.flags = flags, js.last_chunk = chunk;
            js.n_inliers = converged ? best : 0;
        }
        __syncthreads();   // the state written above is read below by other lanes
    } else if (lane == 0) {
        js.last_chunk = 0;
    }
    // the outputs are a function of the carried state, so a finished job repeats them on every later call
    const bool conv = (flags & kFlagConverge) != 0;
    if (lane < 16) T12_out[16 * job + lane] = js.T12[lane];
    if (lane == 0) n_inliers_out[job] = conv ? js.n_inliers : 0, flags_out[job] = flags;
    omv_ransac::wave_scatter_inliers(jp, lane, conv ? best_mask + jp.word_start : nullptr, index1, inliers_out);
}

}  // namespace

struct omv_sim3_solver {
    int max_jobs = 0, max_corr = 0, max_hyp = 0, words_cap = 0;
    int n_jobs = 0, n_corr = 0, words_total = 0, last_n_it = 0;
    std::vector<JobParams> jobs;
    JobParams *d_jobs = nullptr;
    JobState *d_state = nullptr;
    int32_t *d_corr_job = nullptr, *d_index1 = nullptr;
    float *d_in = nullptr;    // Xw1 [3], Xw2 [3], sigma2_1, sigma2_2 per correspondence (8 floats, planar)
    float *d_pre = nullptr;   // X3Dc1 [3], X3Dc2 [3], P1 [2], P2 [2], maxErr1, maxErr2 (12 floats, planar)
    int32_t *d_hidx = nullptr, *d_hcount = nullptr;
    float *d_hf = nullptr;    // per (job, hypothesis): T12 [16], T21 [16], R [9], t [3], s (45 floats, planar)
    unsigned long long *d_hmask = nullptr, *d_best_mask = nullptr;
    omv::DeviceArena mem;   // owns the d_* buffers
};

extern "C" {

omv_status omv_sim3_solver_create(int max_jobs, int max_corr_total, int max_hyp, omv_sim3_solver **out) {
    if (const omv_status e = omv_ransac::check_create(out, max_jobs, max_corr_total, max_hyp)) return e;
    auto h = std::make_unique<omv_sim3_solver>();
    h->max_jobs = max_jobs, h->max_corr = max_corr_total, h->max_hyp = max_hyp;
    h->words_cap = omv_ransac::words_cap(max_corr_total, max_jobs);
    const size_t nc = (size_t)std::max(1, max_corr_total), nh = (size_t)max_jobs * max_hyp;
    omv::DeviceArena &mem = h->mem;
    if (!mem.alloc(&h->d_jobs, max_jobs) || !mem.alloc(&h->d_state, max_jobs) || !mem.alloc(&h->d_corr_job, nc) ||
        !mem.alloc(&h->d_index1, nc) || !mem.alloc(&h->d_in, nc * 8) || !mem.alloc(&h->d_pre, nc * 12) ||
        !mem.alloc(&h->d_hidx, nh * 3) || !mem.alloc(&h->d_hcount, nh) || !mem.alloc(&h->d_hf, nh * 45) ||
        !mem.alloc(&h->d_hmask, (size_t)max_hyp * h->words_cap) || !mem.alloc(&h->d_best_mask, h->words_cap))
        return OMV_ERR_HIP;
    *out = h.release();
    return OMV_OK;
}

omv_status omv_sim3_solver_destroy(omv_sim3_solver *h) {
    if (!h) return OMV_ERR_ARG;
    delete h;
    return OMV_OK;
}

omv_status omv_sim3_solver_set(omv_sim3_solver *h, int n_jobs, const int32_t *corr_start, const float *Xw1,
                               const float *Xw2, const float *sigma2_1, const float *sigma2_2, const int32_t *index1,
                               const int32_t *mN1, const float *pose1, const float *pose2, const float *cam1,
                               const float *cam2, const int32_t *model1, const int32_t *model2, const int32_t *fix_scale,
                               double prob, const int32_t *min_inliers, int max_its, int32_t *ransac_max_its_out,
                               void *stream) {
    if (!h || (n_jobs > 0 && (!pose1 || !pose2 || !cam1 || !cam2 || !model1 || !model2 || !fix_scale || !min_inliers)))
        return OMV_ERR_ARG;
    std::vector<JobParams> jobs;
    std::vector<int32_t> corr_job;
    int words = 0;
    const auto models_ok = [&](int j) {
        return (model1[j] == OMV_CAM_KB8 || model1[j] == OMV_CAM_PINHOLE) &&
               (model2[j] == OMV_CAM_KB8 || model2[j] == OMV_CAM_PINHOLE);
    };
    if (const omv_status e = omv_ransac::plan_layout(n_jobs, corr_start, mN1, index1,
                                                     Xw1 && Xw2 && sigma2_1 && sigma2_2 && index1, h->max_jobs,
                                                     h->max_corr, h->words_cap, models_ok, &jobs, &corr_job, &words))
        return e;
    const int n_corr = (int)corr_job.size();
    std::vector<JobState> state(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        JobParams &p = jobs[j];
        p.min_inliers = min_inliers[j], p.fix_scale = fix_scale[j] != 0, p.model1 = model1[j], p.model2 = model2[j];
        p.max_its = p.n > 0 ? omv_ransac::ransac_its(prob, (float)p.min_inliers / p.n, p.min_inliers == p.n, max_its) : 1;
        if (ransac_max_its_out) ransac_max_its_out[j] = p.max_its;
        for (int k = 0; k < 12; k++) p.pose1[k] = pose1[12 * j + k], p.pose2[k] = pose2[12 * j + k];
        for (int k = 0; k < 8; k++) p.cam1[k] = cam1[8 * j + k], p.cam2[k] = cam2[8 * j + k];
        JobState &s = state[j];
        s = JobState();
        s.T12[0] = s.T12[5] = s.T12[10] = s.T12[15] = 1.f;
        s.R[0] = s.R[4] = s.R[8] = 1.f, s.s = 1.f;
        // iterate's entry test N < mRansacMinInliers; fewer than three correspondences cannot be sampled (the reference
        // is undefined there) and are treated the same way: bNoMore, identity, no work
        if (p.n < p.min_inliers || p.n < 3) s.flags = kFlagNoMore;
    }
    hipStream_t st = (hipStream_t)stream;
    h->jobs = jobs, h->n_jobs = n_jobs, h->n_corr = n_corr, h->words_total = words, h->last_n_it = 0;
    if (n_jobs == 0) return OMV_OK;
    HIP_OK(hipMemcpyAsync(h->d_jobs, jobs.data(), n_jobs * sizeof(JobParams), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->d_state, state.data(), n_jobs * sizeof(JobState), hipMemcpyHostToDevice, st));
    if (n_corr > 0) {
        const size_t nc = (size_t)h->max_corr, fb = (size_t)n_corr * sizeof(float);
        HIP_OK(hipMemcpyAsync(h->d_corr_job, corr_job.data(), n_corr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_index1, index1, n_corr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in, Xw1, 3 * fb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in + 3 * nc, Xw2, 3 * fb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in + 6 * nc, sigma2_1, fb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in + 7 * nc, sigma2_2, fb, hipMemcpyHostToDevice, st));
        float *pre = h->d_pre;
        sim3_prepare_kernel<<<(n_corr + 255) / 256, 256, 0, st>>>(
            h->d_jobs, n_corr, h->d_corr_job, h->d_in, h->d_in + 3 * nc, h->d_in + 6 * nc, h->d_in + 7 * nc, pre,
            pre + 3 * nc, pre + 6 * nc, pre + 8 * nc, pre + 10 * nc, pre + 11 * nc);
        HIP_OK(hipGetLastError());
    }
    // the host arrays above go out of scope: the copies must have left them
    HIP_OK(hipStreamSynchronize(st));
    return OMV_OK;
}

omv_status omv_sim3_solver_iterate(omv_sim3_solver *h, int n_iterations, const int32_t *draws, float *T12_out,
                                   int32_t *n_inliers_out, uint8_t *inliers_out, int32_t *flags_out, void *stream) {
    if (!h || n_iterations < 0 || !T12_out || !n_inliers_out || !inliers_out || !flags_out ||
        (n_iterations > 0 && !draws))
        return OMV_ERR_ARG;
    if (n_iterations > h->max_hyp) return OMV_ERR_CAPACITY;
    if (h->n_jobs == 0) return OMV_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t nh = (size_t)h->max_jobs * h->max_hyp, nc = (size_t)h->max_corr;
    float *hf = h->d_hf, *pre = h->d_pre;
    const int n_waves = h->n_jobs * n_iterations;
    if (n_waves > 0) {
        sim3_hypothesis_kernel<<<(n_waves + kWavesPerBlock - 1) / kWavesPerBlock, 64 * kWavesPerBlock, 0, st>>>(
            h->d_jobs, h->d_state, h->n_jobs, n_iterations, draws, pre, pre + 3 * nc, pre + 6 * nc, pre + 8 * nc,
            pre + 10 * nc, pre + 11 * nc, h->words_total, h->d_hidx, hf, hf + 16 * nh, hf + 32 * nh, hf + 41 * nh,
            hf + 44 * nh, h->d_hcount, h->d_hmask);
        HIP_OK(hipGetLastError());
    }
    sim3_select_kernel<<<h->n_jobs, 64, 0, st>>>(h->d_jobs, h->d_state, n_iterations, h->words_total, h->d_hcount, hf,
                                                 hf + 32 * nh, hf + 41 * nh, hf + 44 * nh, h->d_hmask, h->d_best_mask,
                                                 h->d_index1, T12_out, n_inliers_out, inliers_out, flags_out);
    HIP_OK(hipGetLastError());
    h->last_n_it = n_iterations;
    return OMV_OK;
}

omv_status omv_sim3_solver_best(omv_sim3_solver *h, int job, float *R, float *t, float *scale, int32_t *n_best,
                                int32_t *iterations, void *stream) {
    if (!h || job < 0 || job >= h->n_jobs) return OMV_ERR_ARG;
    JobState s;
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(&s, h->d_state + job, sizeof(JobState), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (R) std::copy(s.R, s.R + 9, R);
    if (t) std::copy(s.t, s.t + 3, t);
    if (scale) *scale = s.s;
    if (n_best) *n_best = s.best_inliers;
    if (iterations) *iterations = s.iterations;
    return OMV_OK;
}

omv_status omv_sim3_solver_debug(omv_sim3_solver *h, int job, int32_t *n_hyp, int32_t *idx, float *R, float *t,
                                 float *scale, float *T12, float *T21, int32_t *count, uint64_t *mask_words,
                                 void *stream) {
    if (!h || job < 0 || job >= h->n_jobs || !n_hyp) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    JobState s;
    HIP_OK(hipMemcpyAsync(&s, h->d_state + job, sizeof(JobState), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const int H = std::min(s.last_chunk, h->last_n_it);
    *n_hyp = H;
    if (H <= 0) return OMV_OK;
    const size_t nh = (size_t)h->max_jobs * h->max_hyp, o = (size_t)job * h->last_n_it;
    const float *hf = h->d_hf;
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    if (idx) HIP_OK(hipMemcpyAsync(idx, h->d_hidx + 3 * o, (size_t)H * 3 * sizeof(int32_t), k, st));
    if (T12) HIP_OK(hipMemcpyAsync(T12, hf + 16 * o, (size_t)H * 16 * sizeof(float), k, st));
    if (T21) HIP_OK(hipMemcpyAsync(T21, hf + 16 * nh + 16 * o, (size_t)H * 16 * sizeof(float), k, st));
    if (R) HIP_OK(hipMemcpyAsync(R, hf + 32 * nh + 9 * o, (size_t)H * 9 * sizeof(float), k, st));
    if (t) HIP_OK(hipMemcpyAsync(t, hf + 41 * nh + 3 * o, (size_t)H * 3 * sizeof(float), k, st));
    if (scale) HIP_OK(hipMemcpyAsync(scale, hf + 44 * nh + o, (size_t)H * sizeof(float), k, st));
    if (count) HIP_OK(hipMemcpyAsync(count, h->d_hcount + o, (size_t)H * sizeof(int32_t), k, st));
    HIP_OK(omv_ransac::read_mask_rows(mask_words, h->d_hmask, h->jobs[job], h->words_total, H, st));
    HIP_OK(hipStreamSynchronize(st));
    return OMV_OK;
}

}  // extern "C"
