// MI355X-native MLPnPsolver (src/MLPnPsolver.cpp, include/MLPnPsolver.h): the PnP RANSAC Tracking::Relocalization runs
// per candidate keyframe (src/Tracking.cc:3543-3730), batched over J independent solvers ("jobs") that share one handle.
//
//   pnp_prepare_kernel     the constructor's per-correspondence part (:28-45): the bearing cam_unproject_f(P2D) / z in
//                          float (z = 1, not unit length), widened to double; its two nullspace vectors (:325-328) as
//                          columns 1 and 2 of the Householder reflector Eigen's makeHouseholder builds for it; Xw widened;
//                          mvMaxError = sigma2 * th2 in float (:217).
//   pnp_hypothesis_kernel  computePose + CheckInliers (:306-617, :220-247): one wavefront per (job, hypothesis), four per
//                          block.  The sampling (:79-98) is replayed from the caller's raw draws.  The 12 x 12 (9 x 9)
//                          A^T A, the 3 x 3 and 6 x 6 systems live in the wave's LDS slot; one lane per matrix entry sums
//                          over the correspondences in their order, the Jacobi rotations (g2o_types.h sym_eig_wave) and
//                          Eigen::LDLT (ldlt_pivot_solve_wave<6>) run over the wave.  The lanes then stride over the job's
//                          correspondences and __ballot builds the inlier mask as 64-bit words.
//   pnp_select_kernel      the sequential rule of iterate (:56-175), one wavefront per job, with Refine (:249-303) for
//                          every hypothesis that becomes the best: computePose over the best mask's correspondences (the
//                          same device function as the hypotheses', the sums plain per-entry loops), CheckInliers, and
//                          the outcome kept with the carried state.
//
// iterate's loop condition is an OR (:75): a call runs max(nIterations, mRansacMaxIts - mnIterations) hypotheses unless
// it returns earlier, so Tracking's iterate(5) runs the whole RANSAC on its first call and five more on every later one.
//
// All of computePose is double, as in the reference.  Not bit-exact with it: the JacobiSVDs are cyclic Jacobi
// eigen-decompositions (of A^T A, and of M^T M for the nearest rotation), the eigenvectors of the planarity matrix get a
// fixed sign (largest component positive), the sums run in correspondence order per entry, and mlpnpJacs (:764-1393) is
// the same derivative written through the chain rule.  tests/test_mlpnp_gpu.py bounds the difference by the problem's
// conditioning.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/omv.h"
#include "g2o_types.h"
#include "omv_camera.h"
#include "omv_device.h"
#include "omv_host.h"
#include "omv_ransac.h"

namespace {

using omv_g2o::ldlt_pivot_solve_wave;
using omv_g2o::sym_eig_wave;

constexpr int kWavesPerBlock = 4;
constexpr int kMinSet = 6;
constexpr int kPre = 12;       // doubles per prepared correspondence: f [3], r [3], s [3], Xw [3]
constexpr int kRow = 14;       // doubles per Gauss-Newton row pair: Jac row r [6], Jac row s [6], residual r, s
constexpr int kHypD = 24;      // doubles per pose record: R0 [9], t0 [3], R [9], t [3]
constexpr int kHypI = 10;      // ints per hypothesis record: idx [6], planar, GN iterations, exit reason, count
constexpr int kRefI = 8;       // ints per Refine record: hypothesis, n points, planar, iterations, reason, count, ok, -
// per-wave LDS slot (doubles): A^T A | V | 3x3 | V3 | J^T J | g | dx | ldlt scratch | Jacobian rows of six points
constexpr int kOffA = 0, kOffV = 144, kOffM = 288, kOffVM = 297, kOffH = 306, kOffG = 342, kOffDx = 348, kOffT = 354,
              kOffRows = 366, kSlot = kOffRows + kMinSet * kRow;
constexpr int kSlotI = 16;     // ints: ldlt transpositions [8], the sampled list [6]

struct JobParams : omv_ransac::JobLayout {
    int min_inliers, max_its, model;
    float cam[8];
};
static_assert(sizeof(JobParams) == 16 * 4, "the layout is the head, nothing is padded");

struct JobState {
    int iterations, best_inliers, flags, last_chunk, n_inliers, n_refine;
    int refined_valid, refined_count, refined_ok, out_kind;   // out_kind: 0 identity, 1 the refined outcome, 2 the best
    float Tbest[16], Tref[16];
};

struct Pose {
    double R0[9], t0[3], R[9], t[3];
    int planar, its, reason;
};

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// Eigen's makeHouseholder (Householder.h) for the vector (c0, tail): H = I - tau [1; v][1; v]^T maps it to beta e0
__device__ __forceinline__ void householder3(const double *f, double *H) {
    const double c0 = f[0], tail_sq = f[1] * f[1] + f[2] * f[2];
    double tau, v[3] = {1.0, 0.0, 0.0};
    if (tail_sq <= DBL_MIN) {
        tau = 0.0;
    } else {
        double beta = sqrt(c0 * c0 + tail_sq);
        if (c0 >= 0.0) beta = -beta;
        v[1] = f[1] / (c0 - beta), v[2] = f[2] / (c0 - beta);
        tau = (beta - c0) / beta;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) H[3 * i + j] = (i == j ? 1.0 : 0.0) - tau * v[i] * v[j];
}

__global__ void __launch_bounds__(256)
    pnp_prepare_kernel(const JobParams *jobs, int n_corr, const int32_t *corr_job, const float *P2D, const float *sigma2,
                       const float *Xw, float th2, double *pre, float *max_err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_corr) return;
    const JobParams &jp = jobs[corr_job[i]];
    float ray[3];
    omv::cam_unproject_f(jp.model, jp.cam, P2D[2 * i], P2D[2 * i + 1], ray);
    const float z = ray[2];
    const double f[3] = {(double)(ray[0] / z), (double)(ray[1] / z), (double)(ray[2] / z)};   // cv_br /= cv_br.z
    double H[9];
    householder3(f, H);
    double *o = pre + (size_t)kPre * i;
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = f[k], o[3 + k] = H[3 * k + 1], o[6 + k] = H[3 * k + 2], o[9 + k] = (double)Xw[3 * i + k];
    max_err[i] = sigma2[i] * th2;
}

// rank of the 3 x 3 m (destroyed) as Eigen::FullPivHouseholderQR with its default threshold reports it
// (FullPivHouseholderQR.h computeInPlace / rank): full pivoting, the column-major first maximum, the early end when the
// corner is below 3 eps of the first pivot candidate, and |R_ii| > max|R_kk| * 3 eps.
__device__ inline int fullpiv_rank3(double (&m)[3][3]) {
    const double prec = 3.0 * DBL_EPSILON;
    double maxpivot = 0.0, biggest = 0.0;
    int nonzero = 3;
    for (int k = 0; k < 3; k++) {
        int row = k, col = k;
        double big = fabs(m[k][k]);
        for (int c = k; c < 3; c++)
            for (int r = k; r < 3; r++)
                if (fabs(m[r][c]) > big) big = fabs(m[r][c]), row = r, col = c;
        if (k == 0) biggest = big;
        if (big <= biggest * prec) {
            nonzero = k;
            break;
        }
        for (int c = k; c < 3; c++) {
            const double u = m[k][c];
            m[k][c] = m[row][c], m[row][c] = u;
        }
        for (int r = 0; r < 3; r++) {
            const double u = m[r][k];
            m[r][k] = m[r][col], m[r][col] = u;
        }
        const double c0 = m[k][k];
        double tail_sq = 0.0, ess[3] = {0.0, 0.0, 0.0}, tau, beta;
        for (int r = k + 1; r < 3; r++) tail_sq += m[r][k] * m[r][k];
        if (tail_sq <= DBL_MIN) {
            tau = 0.0, beta = c0;
        } else {
            beta = sqrt(c0 * c0 + tail_sq);
            if (c0 >= 0.0) beta = -beta;
            for (int r = k + 1; r < 3; r++) ess[r] = m[r][k] / (c0 - beta);
            tau = (beta - c0) / beta;
        }
        m[k][k] = beta;
        if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
        for (int c = k + 1; c < 3; c++) {
            double s = m[k][c];
            for (int r = k + 1; r < 3; r++) s += ess[r] * m[r][c];
            m[k][c] -= tau * s;
            for (int r = k + 1; r < 3; r++) m[r][c] -= tau * ess[r] * s;
        }
    }
    int rank = 0;
    for (int i = 0; i < nonzero; i++) rank += fabs(m[i][i]) > maxpivot * prec;
    return rank;
}

__device__ __forceinline__ double det3(const double *R) {
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// rodrigues2rot (:619-632)
__device__ inline void rodrigues2rot(const double *w, double *R) {
    const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (n > DBL_EPSILON) {
        const double a = sin(n) / n, b = (1.0 - cos(n)) / (n * n);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                R[3 * i + j] = (R[3 * i + j] + a * K[3 * i + j]) + b * kk;
            }
    }
}

// rot2rodrigues (:634-648), the acos of the unclamped trace / 2 included: a NaN fails the test and leaves omega zero
__device__ inline void rot2rodrigues(const double *R, double *w) {
    w[0] = w[1] = w[2] = 0.0;
    const double trace = ((R[0] + R[4]) + R[8]) - 1.0;
    const double wn = acos(trace / 2.0);
    if (wn > DBL_EPSILON) {
        const double sc = wn / (2.0 * sin(wn));
        w[0] = (R[7] - R[5]) * sc, w[1] = (R[2] - R[6]) * sc, w[2] = (R[3] - R[1]) * sc;
    }
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

// The residual pair and Jacobian rows of one correspondence at x = (w, t) (mlpnp_residuals_and_jacs :718-762 with
// mlpnpJacs :764-1393 as d(N^T normalize(R(w) p + t)) / d(w, t) through the chain rule).  R is rodrigues2rot(w); the
// derivative of R(w) p uses the unguarded Rodrigues coefficients, so that w == 0 divides by zero as the reference does.
__device__ inline void residual_and_jac(const double *x, const double *R, const double *q, double *row) {
    const double *r = q + 3, *s = q + 6, *p = q + 9;
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + x[3 + i];
    const double nc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double u[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
    row[12] = (r[0] * u[0] + r[1] * u[1]) + r[2] * u[2];
    row[13] = (s[0] * u[0] + s[1] * u[1]) + s[2] * u[2];
    // d u / d c = (I - u u^T) / |c|; the rows N^T d u / d c
    double gr[3], gs[3];
#pragma unroll
    for (int i = 0; i < 3; i++) gr[i] = (r[i] - row[12] * u[i]) / nc, gs[i] = (s[i] - row[13] * u[i]) / nc;
    const double *w = x;
    const double n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], n = sqrt(n2);
    const double sn = sin(n), cn = cos(n);
    const double a = sn / n, b = (1.0 - cn) / n2;
    const double da = (n * cn - sn) / (n2 * n), db = (n * sn - 2.0 * (1.0 - cn)) / (n2 * n2);   // a' / n, b' / n
    double Kp[3], KKp[3];
    cross3(w, p, Kp);
    cross3(w, Kp, KKp);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double ep[3], eKp[3], wep[3], d[3];
        cross3(e, p, ep);
        cross3(e, Kp, eKp);
        cross3(w, ep, wep);
#pragma unroll
        for (int i = 0; i < 3; i++)
            d[i] = ((da * w[k]) * Kp[i] + a * ep[i]) + ((db * w[k]) * KKp[i] + b * (eKp[i] + wep[i]));
        row[k] = (gr[0] * d[0] + gr[1] * d[1]) + gr[2] * d[2];
        row[6 + k] = (gs[0] * d[0] + gs[1] * d[1]) + gs[2] * d[2];
        row[3 + k] = gr[k], row[9 + k] = gs[k];
    }
}

// Entry `a` of the design-matrix row of nullspace vector v (3) and point p (:393-465)
__device__ __forceinline__ double design_entry(bool planar, const double *v, const double *p, int a) {
    if (planar) return a < 6 ? v[a >> 1] * p[1 + (a & 1)] : v[a - 6];
    return a < 9 ? v[a / 3] * p[a % 3] : v[a - 9];
}

// U V^T of the SVD of the 3 x 3 T (row-major) as T (T^T T)^(-1/2), the eigen-decomposition by the wave's Jacobi
__device__ inline void nearest_rotation_wave(const double *T, double *sm, int lane, double *R) {
    double *B = sm + kOffM, *V = sm + kOffVM;
    if (lane < 9) {
        const int i = lane / 3, j = lane % 3;
        B[lane] = (T[i] * T[j] + T[3 + i] * T[3 + j]) + T[6 + i] * T[6 + j];
    }
    omv::wave_lds_sync();
    sym_eig_wave<3>(B, V, lane);
    omv::wave_lds_sync();
    double S[9];   // V diag(1 / sqrt(lambda)) V^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (V[3 * i + k] / sqrt(B[4 * k])) * V[3 * j + k];
            S[3 * i + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (T[3 * i] * S[j] + T[3 * i + 1] * S[3 + j]) + T[3 * i + 2] * S[6 + j];
    omv::wave_lds_sync();
}

// sum over the first six correspondences of 1 - normalize(R p + t) . f (:534-543, :584-589)
__device__ inline double direction_error(const double *pre, const int *list, const double *R, const double *t) {
    double e = 0.0;
    for (int k = 0; k < 6; k++) {
        const double *q = pre + (size_t)kPre * list[k], *p = q + 9;
        double v[3];
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + t[i];
        const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        e += 1.0 - (((v[0] / nv) * q[0] + (v[1] / nv) * q[1]) + (v[2] / nv) * q[2]);
    }
    return e;
}

// computePose (:306-617) over the n >= 6 correspondences list[0 .. n-1] (indices into pre) by one wavefront; sm / smi:
// the wave's LDS slot; rows: n * kRow doubles (LDS or global).  Every lane calls it and gets the same result.
__device__ inline void compute_pose_wave(const double *pre, const int *list, int n, double *sm, int *smi, double *rows,
                                         int lane, Pose &o) {
    double *A = sm + kOffA, *V = sm + kOffV, *M = sm + kOffM, *VM = sm + kOffVM;
    // ---- 1. planarity: rank of sum p p^T (:336-344) ----
    if (lane < 9) {
        const int i = lane / 3, j = lane % 3;
        double s = 0.0;
        for (int k = 0; k < n; k++) {
            const double *p = pre + (size_t)kPre * list[k] + 9;
            s += p[i] * p[j];
        }
        M[lane] = s;
    }
    omv::wave_lds_sync();
    double m[3][3];
#pragma unroll
    for (int i = 0; i < 9; i++) m[i / 3][i % 3] = M[i];
    const bool planar = fullpiv_rank3(m) == 2;
    double E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};   // eigenRot
    omv::wave_lds_sync();
    if (planar) {   // eigenvectors by increasing eigenvalue, as rows (:349-351); sign: the largest component positive
        sym_eig_wave<3>(M, VM, lane);
        omv::wave_lds_sync();
        int ord[3] = {0, 1, 2};   // a stable sort of the three eigenvalues
        if (M[4 * ord[1]] < M[4 * ord[0]]) ord[0] = 1, ord[1] = 0;
        if (M[4 * ord[2]] < M[4 * ord[1]]) {
            const int u = ord[1];
            ord[1] = ord[2], ord[2] = u;
        }
        if (M[4 * ord[1]] < M[4 * ord[0]]) {
            const int u = ord[0];
            ord[0] = ord[1], ord[1] = u;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double v0 = VM[ord[i]], v1 = VM[3 + ord[i]], v2 = VM[6 + ord[i]];
            double big = v0;
            if (fabs(v1) > fabs(big)) big = v1;
            if (fabs(v2) > fabs(big)) big = v2;
            const double sg = big < 0.0 ? -1.0 : 1.0;
            E[3 * i] = sg * v0, E[3 * i + 1] = sg * v1, E[3 * i + 2] = sg * v2;
        }
        omv::wave_lds_sync();
    }
    // ---- 3./4. A^T A (:382-475): one entry per lane, summed in row order ----
    const int cols = planar ? 9 : 12;
    for (int e = lane; e < cols * cols; e += 64) {
        const int a = e / cols, b = e - a * cols;
        double s = 0.0;
        for (int k = 0; k < n; k++) {
            const double *q = pre + (size_t)kPre * list[k];
            double p[3] = {q[9], q[10], q[11]};
            if (planar) {
                const double x = p[0], y = p[1], z = p[2];
#pragma unroll
                for (int i = 0; i < 3; i++) p[i] = (E[3 * i] * x + E[3 * i + 1] * y) + E[3 * i + 2] * z;
            }
            s += design_entry(planar, q + 3, p, a) * design_entry(planar, q + 3, p, b);
            s += design_entry(planar, q + 6, p, a) * design_entry(planar, q + 6, p, b);
        }
        A[e] = s;
    }
    omv::wave_lds_sync();
    // the right singular vector of the smallest singular value (:477-478): the eigenvector of the smallest eigenvalue
    double x[12];
    if (planar) sym_eig_wave<9>(A, V, lane);
    else sym_eig_wave<12>(A, V, lane);
    omv::wave_lds_sync();
    {
        int im = 0;
        for (int i = 1; i < cols; i++)
            if (A[i * cols + i] < A[im * cols + im]) im = i;
#pragma unroll
        for (int i = 0; i < 12; i++) x[i] = i < cols ? V[i * cols + im] : 0.0;
    }
    omv::wave_lds_sync();
    double Rout[9], tout[3];
    if (planar) {   // :486-548
        double c1[3] = {x[0], x[2], x[4]}, c2[3] = {x[1], x[3], x[5]}, c0[3];
        cross3(c1, c2, c0);
        // tmp (columns c0 c1 c2) transposed: rows c0 c1 c2
        const double T[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};
        const double n1 = sqrt((T[1] * T[1] + T[4] * T[4]) + T[7] * T[7]), n2 = sqrt((T[2] * T[2] + T[5] * T[5]) + T[8] * T[8]);
        const double scale = 1.0 / sqrt(fabs(n1 * n2));
        double R1[9], Q[9];
        nearest_rotation_wave(T, sm, lane, R1);
        if (det3(R1) < 0.0)
#pragma unroll
            for (int i = 0; i < 9; i++) R1[i] *= -1.0;
        // Rout1 = eigenRot^T Rout1, transposed, negated
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Q[3 * j + i] = -((E[i] * R1[j] + E[3 + i] * R1[3 + j]) + E[6 + i] * R1[6 + j]);
        if (det3(Q) < 0.0) Q[2] *= -1.0, Q[5] *= -1.0, Q[8] *= -1.0;
        const double t[3] = {scale * x[6], scale * x[7], scale * x[8]}, tn[3] = {-t[0], -t[1], -t[2]};
        double Q2[9];
#pragma unroll
        for (int i = 0; i < 3; i++) Q2[3 * i] = -Q[3 * i], Q2[3 * i + 1] = -Q[3 * i + 1], Q2[3 * i + 2] = Q[3 * i + 2];
        const double e0 = direction_error(pre, list, Q, t), e1 = direction_error(pre, list, Q, tn);
        const double e2 = direction_error(pre, list, Q2, t), e3 = direction_error(pre, list, Q2, tn);
        int best = 0;   // std::min_element: the first minimum
        double eb = e0;
        if (e1 < eb) eb = e1, best = 1;
        if (e2 < eb) eb = e2, best = 2;
        if (e3 < eb) eb = e3, best = 3;
#pragma unroll
        for (int i = 0; i < 9; i++) Rout[i] = best < 2 ? Q[i] : Q2[i];
#pragma unroll
        for (int i = 0; i < 3; i++) tout[i] = (best & 1) ? tn[i] : t[i];
    } else {   // :549-596
        const double T[9] = {x[0], x[3], x[6], x[1], x[4], x[7], x[2], x[5], x[8]};
        const double n0 = sqrt((T[0] * T[0] + T[3] * T[3]) + T[6] * T[6]), n1 = sqrt((T[1] * T[1] + T[4] * T[4]) + T[7] * T[7]),
                     n2 = sqrt((T[2] * T[2] + T[5] * T[5]) + T[8] * T[8]);
        const double scale = 1.0 / pow(fabs((n0 * n1) * n2), 1.0 / 3.0);
        double R1[9];
        nearest_rotation_wave(T, sm, lane, R1);
        if (det3(R1) < 0.0)
#pragma unroll
            for (int i = 0; i < 9; i++) R1[i] *= -1.0;
        // Ts[s] = [Rout, +-tout]^-1 with tout = Rout (scale x[9..11]): rotation Rout^T, translation -+ scale x[9..11]
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Rout[3 * i + j] = R1[3 * j + i];
        const double tp[3] = {-(scale * x[9]), -(scale * x[10]), -(scale * x[11])}, tm[3] = {scale * x[9], scale * x[10], scale * x[11]};
        const double e0 = direction_error(pre, list, Rout, tp), e1 = direction_error(pre, list, Rout, tm);
#pragma unroll
        for (int i = 0; i < 3; i++) tout[i] = e0 < e1 ? tp[i] : tm[i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) o.R0[i] = Rout[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o.t0[i] = tout[i];
    o.planar = planar;
    // ---- 5. Gauss-Newton (mlpnp_gn :650-716) ----
    double xs[6];
    rot2rodrigues(Rout, xs);
    xs[3] = tout[0], xs[4] = tout[1], xs[5] = tout[2];
    double *H = sm + kOffH, *g = sm + kOffG, *dxs = sm + kOffDx, *tl = sm + kOffT;
    int it = 0, reason = 0;   // 0: five iterations, 1: max|Jac dx| < epsP, 2: the 5 / 1 break, 3: no finite step
    while (it < 5) {
        double R[9];
        rodrigues2rot(xs, R);
        for (int k = lane; k < n; k += 64) residual_and_jac(xs, R, pre + (size_t)kPre * list[k], rows + (size_t)kRow * k);
        omv::wave_mem_sync();
        if (lane < 42) {   // A = Jac^T Jac (36 entries), g = Jac^T r (6)
            const int a = lane < 36 ? lane / 6 : lane - 36, b = lane < 36 ? lane % 6 : 12;
            double s = 0.0;
            for (int k = 0; k < n; k++) {
                const double *rw = rows + (size_t)kRow * k;
                s += rw[a] * (b == 12 ? rw[12] : rw[b]);
                s += rw[6 + a] * (b == 12 ? rw[13] : rw[6 + b]);
            }
            if (lane < 36) H[lane] = s;
            else g[lane - 36] = s;
        }
        omv::wave_lds_sync();
        bool finite = true;
        for (int i = 0; i < 36; i++) finite = finite && fabs(H[i]) <= DBL_MAX;
        for (int i = 0; i < 6; i++) finite = finite && fabs(g[i]) <= DBL_MAX;
        omv::wave_lds_sync();
        const bool solved = finite && ldlt_pivot_solve_wave<6>(H, g, dxs, tl, smi, lane);
        omv::wave_lds_sync();
        double dx[6], mx = 0.0, mn = DBL_MAX;
        bool dx_finite = solved;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            dx[i] = solved ? dxs[i] : 0.0;
            dx_finite = dx_finite && fabs(dx[i]) <= DBL_MAX;
            mx = fmax(mx, fabs(dx[i])), mn = fmin(mn, fabs(dx[i]));
        }
        if (!dx_finite) {   // the reference goes on with NaN (a non-finite system) to a non-finite pose
            if (!finite)
#pragma unroll
                for (int i = 0; i < 6; i++) xs[i] = __builtin_nan("");
            reason = 3;
            break;
        }
        if (mx > 5.0 || mn > 1.0) {
            reason = 2;
            break;
        }
        double dl = 0.0;
        for (int k = lane; k < n; k += 64) {
            const double *rw = rows + (size_t)kRow * k;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) s0 += rw[i] * dx[i], s1 += rw[6 + i] * dx[i];
            dl = fmax(dl, fmax(fabs(s0), fabs(s1)));
        }
        dl = wave_max_f64(dl);
        omv::wave_mem_sync();   // the rows are rewritten by the next iteration
#pragma unroll
        for (int i = 0; i < 6; i++) xs[i] = xs[i] - dx[i];
        if (dl < 1e-5) {
            reason = 1;
            break;
        }
        ++it;
    }
    rodrigues2rot(xs, o.R);
    // a non-finite w gives the identity through rodrigues2rot's guard; the translation carries the NaN
    o.t[0] = xs[3], o.t[1] = xs[4], o.t[2] = xs[5];
    o.its = it, o.reason = reason;
}

// CheckInliers (:220-247) of the pose (R, t) over the job's n correspondences by one wavefront; returns the count
__device__ inline int check_inliers_wave(const JobParams &jp, const double *R, const double *t, const double *pre,
                                         const float *P2D, const float *max_err, unsigned long long *mask, int lane) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; i++) finite = finite && fabs(R[i]) <= DBL_MAX;
#pragma unroll
    for (int i = 0; i < 3; i++) finite = finite && fabs(t[i]) <= DBL_MAX;
    return omv_ransac::wave_inlier_mask(jp.n, lane, mask, [&](int i) {
        if (!finite) return false;
        const size_t c = (size_t)(jp.corr_start + i);
        const double *p = pre + kPre * c + 9;
        float X[3], u, v;
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = (float)(((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + t[r]);
        omv::cam_project_f(jp.model, jp.cam, X, u, v);
        const float dx = P2D[2 * c] - u, dy = P2D[2 * c + 1] - v;
        const float e2 = dx * dx + dy * dy;
        return e2 < max_err[c];
    });
}

__device__ __forceinline__ void store_pose(double *hd, const Pose &po) {
#pragma unroll
    for (int k = 0; k < 9; k++) hd[k] = po.R0[k], hd[12 + k] = po.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) hd[9 + k] = po.t0[k], hd[21 + k] = po.t[k];
}

// the chunk of a call (:75): max(nIterations, mRansacMaxIts - mnIterations), within the draws the caller supplied
__device__ __forceinline__ int call_chunk(const JobParams &jp, const JobState &js, int n_it, int n_draws) {
    if (jp.n < jp.min_inliers) return 0;
    return min(n_draws, max(n_it, jp.max_its - js.iterations));
}

__global__ void __launch_bounds__(64 * kWavesPerBlock)
    pnp_hypothesis_kernel(const JobParams *jobs, const JobState *state, int n_jobs, int n_it, int n_draws,
                          const int32_t *draws, const double *pre, const float *P2D, const float *max_err,
                          int words_total, int32_t *h_int, double *h_dbl, unsigned long long *h_mask) {
    __shared__ double sm_all[kWavesPerBlock][kSlot];
    __shared__ int smi_all[kWavesPerBlock][kSlotI];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int gidx = blockIdx.x * kWavesPerBlock + wv;
    if (gidx >= n_jobs * n_draws) return;
    const int job = gidx / n_draws, hyp = gidx - job * n_draws;
    const JobParams &jp = jobs[job];
    if (hyp >= call_chunk(jp, state[job], n_it, n_draws)) return;
    double *sm = sm_all[wv];
    int *smi = smi_all[wv];
    int idx[kMinSet];
    omv_ransac::replay_sampling<kMinSet>(jp.n, draws + (size_t)kMinSet * gidx, idx);
    if (lane < kMinSet) {
        int v = idx[0];
#pragma unroll
        for (int i = 1; i < kMinSet; i++) v = lane == i ? idx[i] : v;
        smi[8 + lane] = jp.corr_start + v;
    }
    omv::wave_lds_sync();
    Pose po;
    compute_pose_wave(pre, smi + 8, kMinSet, sm, smi, sm + kOffRows, lane, po);
    const int count = check_inliers_wave(jp, po.R, po.t, pre, P2D, max_err,
                                         h_mask + (size_t)hyp * words_total + jp.word_start, lane);
    if (lane == 0) {
        int32_t *hi = h_int + (size_t)kHypI * gidx;
#pragma unroll
        for (int k = 0; k < kMinSet; k++) hi[k] = idx[k];
        hi[6] = po.planar, hi[7] = po.its, hi[8] = po.reason, hi[9] = count;
        store_pose(h_dbl + (size_t)kHypD * gidx, po);
    }
}

// One wavefront per job: iterate's sequential rule over the call's hypotheses with Refine for every new best, then the
// call's outputs.
__global__ void __launch_bounds__(64)
    pnp_select_kernel(const JobParams *jobs, JobState *state, int n_it, int n_draws, int words_total, const double *pre,
                      const float *P2D, const float *max_err, const int32_t *h_int, const double *h_dbl,
                      const unsigned long long *h_mask, unsigned long long *best_mask, unsigned long long *ref_mask,
                      int32_t *list, double *rows, int32_t *r_int, double *r_dbl, unsigned long long *r_mask,
                      const int32_t *index, float *T_out, int32_t *n_inliers_out, uint8_t *inliers_out,
                      int32_t *flags_out) {
    __shared__ double sm[kSlot];
    __shared__ int smi[kSlotI];
    const int job = blockIdx.x, lane = threadIdx.x;
    const JobParams &jp = jobs[job];
    JobState &js = state[job];
    const int n_words = (jp.n + 63) >> 6;
    const int chunk = call_chunk(jp, js, n_it, n_draws);
    int best = js.best_inliers, valid = js.refined_valid, ok = js.refined_ok, rcount = js.refined_count;
    int done = chunk, found = 0, n_ref = 0;
    unsigned long long *bm = best_mask + jp.word_start, *rm = ref_mask + jp.word_start;
    int32_t *lst = list + jp.corr_start;
    for (int base = 0; base < chunk && !found; base += 64) {
        const int h = base + lane;
        const int c = h < chunk ? h_int[(size_t)kHypI * ((size_t)job * n_draws + h) + 9] : -1;
        unsigned long long q = __ballot(c >= jp.min_inliers);   // the hypotheses that pass :129
        while (q && !found) {
            const int f = __ffsll(q) - 1;
            q &= q - 1;
            const int cf = __shfl(c, f), hyp = base + f;
            if (cf > best) {   // :131-145, then Refine (:147) on the new mvbBestInliers
                best = cf;
                const size_t o = (size_t)job * n_draws + hyp;
                const double *hd = h_dbl + kHypD * o;
                if (lane < 16) {
                    const int r = lane >> 2, cc = lane & 3;
                    js.Tbest[lane] = r == 3 ? (cc == 3 ? 1.f : 0.f) : (cc == 3 ? (float)hd[21 + r] : (float)hd[12 + 3 * r + cc]);
                }
                int n_in = 0;
                for (int w = 0; w < n_words; w++) {
                    const unsigned long long m = h_mask[(size_t)hyp * words_total + jp.word_start + w];
                    if (lane == 0) bm[w] = m;
                    if ((m >> lane) & 1ull) lst[n_in + __popcll(m & ((1ull << lane) - 1ull))] = jp.corr_start + 64 * w + lane;
                    n_in += __popcll(m);
                }
                omv::wave_mem_sync();
                Pose po;
                compute_pose_wave(pre, lst, n_in, sm, smi, rows + (size_t)kRow * jp.corr_start, lane, po);
                unsigned long long *rec_mask = r_mask + (size_t)n_ref * words_total + jp.word_start;
                rcount = check_inliers_wave(jp, po.R, po.t, pre, P2D, max_err, rec_mask, lane);
                omv::wave_mem_sync();
                for (int w = lane; w < n_words; w += 64) rm[w] = rec_mask[w];
                ok = rcount > jp.min_inliers, valid = 1;   // :287
                if (lane < 16) {
                    const int r = lane >> 2, cc = lane & 3;
                    js.Tref[lane] = r == 3 ? (cc == 3 ? 1.f : 0.f) : (cc == 3 ? (float)po.t[r] : (float)po.R[3 * r + cc]);
                }
                if (lane == 0) {
                    int32_t *ri = r_int + (size_t)kRefI * ((size_t)job * n_draws + n_ref);
                    ri[0] = hyp, ri[1] = n_in, ri[2] = po.planar, ri[3] = po.its, ri[4] = po.reason, ri[5] = rcount;
                    ri[6] = ok, ri[7] = 0;
                    store_pose(r_dbl + (size_t)kHypD * ((size_t)job * n_draws + n_ref), po);
                }
                ++n_ref;
            }
            if (valid && ok) found = 1, done = hyp + 1;   // :147-156 with the kept outcome of Refine
        }
    }
    const int iterations = js.iterations + done;
    int flags = 0, kind = 0, n_inl = 0;
    if (found) {
        flags = OMV_PNP_FOUND, kind = 1, n_inl = rcount;
    } else if (jp.n < jp.min_inliers) {
        flags = OMV_PNP_NO_MORE;   // :67-70
    } else if (iterations >= jp.max_its) {   // :160-172
        flags = OMV_PNP_NO_MORE;
        if (best >= jp.min_inliers) flags |= OMV_PNP_FOUND, kind = 2, n_inl = best;
    }
    __syncthreads();   // Tbest / Tref written above are read below by other lanes
    if (lane < 16)
        T_out[16 * job + lane] = kind == 1 ? js.Tref[lane] : (kind == 2 ? js.Tbest[lane] : ((lane & 3) == (lane >> 2) ? 1.f : 0.f));
    if (lane == 0) {
        js.iterations = iterations, js.best_inliers = best, js.flags = flags, js.last_chunk = done, js.n_inliers = n_inl;
        js.n_refine = n_ref, js.refined_valid = valid, js.refined_count = rcount, js.refined_ok = ok, js.out_kind = kind;
        n_inliers_out[job] = n_inl, flags_out[job] = flags;
    }
    omv_ransac::wave_scatter_inliers(jp, lane, kind == 1 ? rm : (kind == 2 ? bm : nullptr), index, inliers_out);
}

}  // namespace

struct omv_pnp {
    int max_jobs = 0, max_corr = 0, max_hyp = 0, words_cap = 0;
    int n_jobs = 0, n_corr = 0, words_total = 0, last_n_draws = 0;
    std::vector<JobParams> jobs;
    JobParams *d_jobs = nullptr;
    JobState *d_state = nullptr;
    int32_t *d_corr_job = nullptr, *d_index = nullptr, *d_list = nullptr;
    float *d_in = nullptr;       // P2D [2], sigma2, Xw [3] per correspondence (6 floats, planar), then mvMaxError
    double *d_pre = nullptr;     // kPre doubles per correspondence
    double *d_rows = nullptr;    // Refine's Gauss-Newton rows, kRow doubles per correspondence
    int32_t *d_hint = nullptr, *d_rint = nullptr;
    double *d_hdbl = nullptr, *d_rdbl = nullptr;
    unsigned long long *d_hmask = nullptr, *d_rmask = nullptr, *d_best_mask = nullptr, *d_ref_mask = nullptr;
    omv::DeviceArena mem;   // owns the d_* buffers
};

extern "C" {

omv_status omv_pnp_create(int max_jobs, int max_corr_total, int max_hyp, omv_pnp **out) {
    if (const omv_status e = omv_ransac::check_create(out, max_jobs, max_corr_total, max_hyp)) return e;
    auto h = std::make_unique<omv_pnp>();
    h->max_jobs = max_jobs, h->max_corr = max_corr_total, h->max_hyp = max_hyp;
    h->words_cap = omv_ransac::words_cap(max_corr_total, max_jobs);
    const size_t nc = (size_t)std::max(1, max_corr_total), nh = (size_t)max_jobs * max_hyp;
    const size_t nm = (size_t)max_hyp * h->words_cap;
    omv::DeviceArena &mem = h->mem;
    if (!mem.alloc(&h->d_jobs, max_jobs) || !mem.alloc(&h->d_state, max_jobs) || !mem.alloc(&h->d_corr_job, nc) ||
        !mem.alloc(&h->d_index, nc) || !mem.alloc(&h->d_list, nc) || !mem.alloc(&h->d_in, nc * 7) ||
        !mem.alloc(&h->d_pre, nc * kPre) || !mem.alloc(&h->d_rows, nc * kRow) || !mem.alloc(&h->d_hint, nh * kHypI) ||
        !mem.alloc(&h->d_rint, nh * kRefI) || !mem.alloc(&h->d_hdbl, nh * kHypD) || !mem.alloc(&h->d_rdbl, nh * kHypD) ||
        !mem.alloc(&h->d_hmask, nm) || !mem.alloc(&h->d_rmask, nm) || !mem.alloc(&h->d_best_mask, h->words_cap) ||
        !mem.alloc(&h->d_ref_mask, h->words_cap))
        return OMV_ERR_HIP;
    *out = h.release();
    return OMV_OK;
}

omv_status omv_pnp_destroy(omv_pnp *h) {
    if (!h) return OMV_ERR_ARG;
    delete h;
    return OMV_OK;
}

omv_status omv_pnp_set(omv_pnp *h, int n_jobs, const int32_t *corr_start, const float *P2D, const float *sigma2,
                       const float *Xw, const int32_t *index, const int32_t *mN, const float *cam, const int32_t *model,
                       double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2,
                       int32_t *ransac_max_its_out, int32_t *ransac_min_inliers_out, void *stream) {
    if (!h || min_set != kMinSet || (n_jobs > 0 && (!cam || !model))) return OMV_ERR_ARG;
    std::vector<JobParams> jobs;
    std::vector<int32_t> corr_job;
    int words = 0;
    const auto model_ok = [&](int j) { return model[j] == OMV_CAM_KB8 || model[j] == OMV_CAM_PINHOLE; };
    if (const omv_status e = omv_ransac::plan_layout(n_jobs, corr_start, mN, index, P2D && sigma2 && Xw && index,
                                                     h->max_jobs, h->max_corr, h->words_cap, model_ok, &jobs,
                                                     &corr_job, &words))
        return e;
    const int n_corr = (int)corr_job.size();
    std::vector<JobState> state(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        JobParams &p = jobs[j];
        p.model = model[j];
        omv_ransac::mlpnp_parameters(p.n, prob, min_inliers, max_its, min_set, epsilon, &p.max_its, &p.min_inliers);
        if (ransac_max_its_out) ransac_max_its_out[j] = p.max_its;
        if (ransac_min_inliers_out) ransac_min_inliers_out[j] = p.min_inliers;
        for (int k = 0; k < 8; k++) p.cam[k] = cam[8 * j + k];
        JobState &s = state[j];
        s = JobState();
        s.Tbest[0] = s.Tbest[5] = s.Tbest[10] = s.Tbest[15] = 1.f;
        s.Tref[0] = s.Tref[5] = s.Tref[10] = s.Tref[15] = 1.f;
    }
    hipStream_t st = (hipStream_t)stream;
    h->jobs = jobs, h->n_jobs = n_jobs, h->n_corr = n_corr, h->words_total = words, h->last_n_draws = 0;
    if (n_jobs == 0) return OMV_OK;
    HIP_OK(hipMemcpyAsync(h->d_jobs, jobs.data(), n_jobs * sizeof(JobParams), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->d_state, state.data(), n_jobs * sizeof(JobState), hipMemcpyHostToDevice, st));
    if (n_corr > 0) {
        const size_t nc = (size_t)h->max_corr, fb = (size_t)n_corr * sizeof(float);
        HIP_OK(hipMemcpyAsync(h->d_corr_job, corr_job.data(), n_corr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_index, index, n_corr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in, P2D, 2 * fb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in + 2 * nc, sigma2, fb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_in + 3 * nc, Xw, 3 * fb, hipMemcpyHostToDevice, st));
        pnp_prepare_kernel<<<(n_corr + 255) / 256, 256, 0, st>>>(h->d_jobs, n_corr, h->d_corr_job, h->d_in,
                                                                 h->d_in + 2 * nc, h->d_in + 3 * nc, th2, h->d_pre,
                                                                 h->d_in + 6 * nc);
        HIP_OK(hipGetLastError());
    }
    // the host arrays above go out of scope: the copies must have left them
    HIP_OK(hipStreamSynchronize(st));
    return OMV_OK;
}

omv_status omv_pnp_iterate(omv_pnp *h, int n_iterations, int n_draws, const int32_t *draws, float *T_out,
                           int32_t *n_inliers_out, uint8_t *inliers_out, int32_t *flags_out, void *stream) {
    if (!h || n_iterations < 0 || n_draws < 0 || !T_out || !n_inliers_out || !inliers_out || !flags_out ||
        (n_draws > 0 && !draws))
        return OMV_ERR_ARG;
    if (n_draws > h->max_hyp) return OMV_ERR_CAPACITY;
    if (h->n_jobs == 0) return OMV_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t nc = (size_t)h->max_corr;
    const int n_waves = h->n_jobs * n_draws;
    if (n_waves > 0) {
        pnp_hypothesis_kernel<<<(n_waves + kWavesPerBlock - 1) / kWavesPerBlock, 64 * kWavesPerBlock, 0, st>>>(
            h->d_jobs, h->d_state, h->n_jobs, n_iterations, n_draws, draws, h->d_pre, h->d_in, h->d_in + 6 * nc,
            h->words_total, h->d_hint, h->d_hdbl, h->d_hmask);
        HIP_OK(hipGetLastError());
    }
    pnp_select_kernel<<<h->n_jobs, 64, 0, st>>>(h->d_jobs, h->d_state, n_iterations, n_draws, h->words_total, h->d_pre,
                                                h->d_in, h->d_in + 6 * nc, h->d_hint, h->d_hdbl, h->d_hmask,
                                                h->d_best_mask, h->d_ref_mask, h->d_list, h->d_rows, h->d_rint, h->d_rdbl,
                                                h->d_rmask, h->d_index, T_out, n_inliers_out, inliers_out, flags_out);
    HIP_OK(hipGetLastError());
    h->last_n_draws = n_draws;
    return OMV_OK;
}

omv_status omv_pnp_debug(omv_pnp *h, int job, int32_t *n_hyp, int32_t *hyp_int, double *hyp_pose, uint64_t *mask_words,
                         int32_t *n_refine, int32_t *ref_int, double *ref_pose, uint64_t *ref_mask_words,
                         int32_t *state_out, double *prepared, void *stream) {
    if (!h || job < 0 || job >= h->n_jobs || !n_hyp || !n_refine) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    JobState s;
    HIP_OK(hipMemcpyAsync(&s, h->d_state + job, sizeof(JobState), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const int H = std::min(s.last_chunk, h->last_n_draws), NR = std::min(s.n_refine, H);
    *n_hyp = H, *n_refine = NR;
    if (state_out) state_out[0] = s.iterations, state_out[1] = s.best_inliers, state_out[2] = s.refined_valid,
                   state_out[3] = s.refined_count, state_out[4] = s.refined_ok, state_out[5] = s.out_kind;
    const size_t o = (size_t)job * h->last_n_draws;
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    const JobParams &p = h->jobs[job];
    if (prepared && p.n)
        HIP_OK(hipMemcpyAsync(prepared, h->d_pre + (size_t)kPre * p.corr_start, (size_t)p.n * kPre * sizeof(double), k, st));
    if (H > 0) {
        if (hyp_int) HIP_OK(hipMemcpyAsync(hyp_int, h->d_hint + kHypI * o, (size_t)H * kHypI * sizeof(int32_t), k, st));
        if (hyp_pose) HIP_OK(hipMemcpyAsync(hyp_pose, h->d_hdbl + kHypD * o, (size_t)H * kHypD * sizeof(double), k, st));
        HIP_OK(omv_ransac::read_mask_rows(mask_words, h->d_hmask, p, h->words_total, H, st));
    }
    if (NR > 0) {
        if (ref_int) HIP_OK(hipMemcpyAsync(ref_int, h->d_rint + kRefI * o, (size_t)NR * kRefI * sizeof(int32_t), k, st));
        if (ref_pose) HIP_OK(hipMemcpyAsync(ref_pose, h->d_rdbl + kHypD * o, (size_t)NR * kHypD * sizeof(double), k, st));
        HIP_OK(omv_ransac::read_mask_rows(ref_mask_words, h->d_rmask, p, h->words_total, NR, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    return OMV_OK;
}

}  // extern "C"
