// MI355X-native Optimizer::InertialOptimization (src/Optimizer.cc:3469-3925): the IMU initialisation LocalMapping runs
// three times per map (InitializeIMU, src/LocalMapping.cc:1255-1517), ScaleRefinement (:1548) and LoopClosing
// (src/LoopClosing.cc:2037) call, batched over J independent maps ("jobs"), one workgroup of 256 threads per job.
//
// The three overloads are modes of one kernel:
//   FULL  velocities, bg, ba, the gravity direction (VertexGDir, 2 DoF) and -- mono only -- the scale free; Levenberg,
//         optimize(200), setUserLambdaInit(1e3) only if priorG != 0; EdgePriorAcc / EdgePriorGyro
//   BIAS  velocities, bg, ba free, Rwg = I and scale = 1; Levenberg, optimize(200), lambda init 1e3; the same priors
//   GS    gravity direction and scale free; Gauss-Newton, optimize(10); Huber (delta 1) on every edge; no priors
// One edge type, EdgeInertialGS (g2o_types.h gs_error / gs_jacobian), one bias for the whole graph (every bias vertex
// is built from vpKFs.front()).
//
// The normal equations of FULL / BIAS have 3K + 9 unknowns in a fixed structure: the velocity part is block-tridiagonal
// in the host planner's position order (inertial_plan.h: the keyframes along their mPrevKF paths), the border to the nine
// shared unknowns (bg ba gdir scale; a fixed one has zero rows and columns) is dense, and the corner is 9 x 9.
//   build   per edge, one thread: residual and Jacobian J [9][16] (column 15 = the residual) to the workspace; per edge,
//           16 threads: Omega J and the upper triangle of J^T Omega J [16][16] (Huber: rho' Omega); then a GATHER per
//           position: its diagonal block is the V2 block of the edge that enters it plus the V1 block of the edge that
//           leaves it, in that order, likewise its border rows; the corner is one fixed-order sum over the edges.
//   solve   block cyclic reduction over the positions, in LDS, with the border and the gradient as ten right-hand sides:
//           at stride s the positions s, 3s, 5s .. are eliminated (their 3 x 3 blocks inverted), the positions 0, 2s,
//           4s .. gather the two updates, and every eliminated position adds B^T D^-1 B to the corner's Schur complement
//           (per thread in position order, then one fixed reduction); the 9 x 9 complement by ldlt_pick_solve<9>; back-
//           substitution down the strides.  ceil(log2 K) + 1 steps of three barriers each.  A non-positive or
//           non-finite pivot anywhere is g2o's ok2 == false (tempChi = DBL_MAX, the trial rejected).
// No atomics anywhere: two calls agree bit for bit.  The assembled system (45 doubles per position) stays in global
// memory / L2 between the trials of one iteration; each trial copies it into LDS with lambda on the diagonal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <vector>

#include "../../include/omv.h"
#include "g2o_types.h"
#include "inertial_plan.h"
#include "omv_device.h"
#include "omv_host.h"

namespace {

using namespace omv_g2o;

constexpr int kInT = 256;                   // threads per job
constexpr int kInNode = 6 + 9 + 9 + 30 + 3;   // LDS doubles per position: D (sym), C, L, B [3][10], x
constexpr int kInInfoLds = 4 * 264;         // inertial_info9_wave's scratch, one slice per wave
static_assert((size_t)OMV_INERTIAL_MAX_KF * kInNode * 8 + 8 * 1024 <= 160 * 1024, "dynamic + static LDS of a workgroup");

struct InJob {
    int k0, K, e0, E, mode, mono;
    float priorG, priorA;
    double bg0[3], ba0[3], Rwg[9], scale;
};
struct InDebug {
    double corner[81], bc[9], xc[9], chi2, lambda_init;
    int32_t iterations, trials, max_trials;
    float err[2];
    int32_t pad;
    long long ticks[3];   // wall_clock64 ticks spent in buildSystem, the linear solves, the trials' error evaluations
};
struct InArgs {
    const InJob *jobs;
    const double *Rwb, *twb, *vel_in;
    const float *old_bg;
    const int32_t *kf1, *kf2;
    const float *pre;
    const int32_t *order, *edge_in, *edge_out;   // per position (k0 + p)
    double *info, *Jw, *EH;                      // per edge: [81], [9][16], [16][16]
    double *D0, *C0, *B0;                        // per position: [6], [9], [3][10]
    double *velC, *velT;                         // per keyframe [3]: the estimate and the trial
    double *dD, *dC, *dB, *dE0, *dX;             // the first system (debug)
    InDebug *dbg;
    double *Rwg_out, *scale_out, *bg_out, *ba_out, *vel_out;
    float *velf_out;
    uint8_t *reint;
    int32_t *iters, *trials;
};

// symmetric 3 x 3 as (00 01 02 11 12 22)
__device__ __forceinline__ void sym3_mul(const double *d, const double *x, double *y) {
    y[0] = d[0] * x[0] + d[1] * x[1] + d[2] * x[2];
    y[1] = d[1] * x[0] + d[3] * x[1] + d[4] * x[2];
    y[2] = d[2] * x[0] + d[4] * x[1] + d[5] * x[2];
}
__device__ __forceinline__ void sym3_full(const double *d, double *m) {
    m[0] = d[0], m[1] = d[1], m[2] = d[2], m[3] = d[1], m[4] = d[3], m[5] = d[4], m[6] = d[2], m[7] = d[4], m[8] = d[5];
}
// In-place inverse by cofactors; false unless the three pivots of its LDL^T (a00, c22 / a00, det / c22) are positive and
// the determinant is finite.
__device__ __forceinline__ bool sym3_invert(double *d) {
    const double c00 = d[3] * d[5] - d[4] * d[4], c01 = d[2] * d[4] - d[1] * d[5], c02 = d[1] * d[4] - d[2] * d[3];
    const double c11 = d[0] * d[5] - d[2] * d[2], c12 = d[1] * d[2] - d[0] * d[4], c22 = d[0] * d[3] - d[1] * d[1];
    const double det = d[0] * c00 + d[1] * c01 + d[2] * c02;
    const bool ok = d[0] > 0.0 && c22 > 0.0 && det > 0.0 && det < DBL_MAX;
    const double id = 1.0 / det;
    d[0] = c00 * id, d[1] = c01 * id, d[2] = c02 * id, d[3] = c11 * id, d[4] = c12 * id, d[5] = c22 * id;
    return ok;
}
__device__ double block_reduce_max(double v, double *sh) {
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double t = 0;
    for (int q = 0; q < nw; ++q) t = fmax(t, sh[q]);
    return t;
}

struct InEst {   // the shared (non-velocity) part of an estimate, in LDS: [0] the estimate, [1] the trial
    double bg[3], ba[3], Rwg[9], s;
};
__device__ __forceinline__ void in_gs_state(const InEst &x, GsState &S) {
    for (int q = 0; q < 3; ++q) S.b1[q] = (float)x.ba[q], S.b1[3 + q] = (float)x.bg[q];
    for (int q = 0; q < 9; ++q) S.Rwg[q] = x.Rwg[q];
    gs_gravity(x.Rwg, S.g);
    S.s = x.s;
}

__global__ void __launch_bounds__(kInT) inertial_opt_kernel(InArgs A) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ double Hs[81], gs[9], xs[9], Ad[81], rhs[9], Lm[81], red[8], red2[256], red3[360], scal[4];
    __shared__ int pick[16], flag[2];
    __shared__ InEst sE[2];
    __shared__ GsState sS[2];
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = tid & 15, grp = tid >> 4;
    const InJob &jp = A.jobs[job];
    const int K = jp.K, E = jp.E, mode = jp.mode;
    const size_t k0 = (size_t)jp.k0, e0 = (size_t)jp.e0;
    const bool gsmode = mode == OMV_INERTIAL_GS, chain = !gsmode;
    const bool fv = !gsmode, fb = !gsmode, fg = mode != OMV_INERTIAL_BIAS && E > 0;
    const bool fs = E > 0 && (gsmode || (mode == OMV_INERTIAL_FULL && jp.mono != 0));
    const double priorG = (double)jp.priorG, priorA = (double)jp.priorA;
    double *sD = dyn, *sC = sD + 6 * K, *sL = sC + 9 * K, *sB = sL + 9 * K, *sX = sB + 30 * K;
    auto is_free = [&](int r) { return r < 6 ? fb : (r < 8 ? fg : fs); };

    if (tid == 0) {
        InEst &est = sE[0];
        for (int q = 0; q < 3; ++q) est.bg[q] = jp.bg0[q], est.ba[q] = jp.ba0[q];
        for (int q = 0; q < 9; ++q) est.Rwg[q] = mode == OMV_INERTIAL_BIAS ? ((q % 4 == 0) ? 1.0 : 0.0) : jp.Rwg[q];
        est.s = mode == OMV_INERTIAL_BIAS ? 1.0 : jp.scale;
        in_gs_state(est, sS[0]);
    }

    // ---- once per call: the edges' information (EdgeInertialGS's ctor), the velocities, x = 0 ----
    for (int e = wave; e < E; e += kInT / 64)
        inertial_info9_wave<true>(A.pre + (e0 + e) * kPF + PreView::C, A.info + (e0 + e) * 81, dyn + wave * 264, lane);
    for (int i = tid; i < 3 * K; i += kInT) A.velC[3 * k0 + i] = A.vel_in[3 * k0 + i];
    __syncthreads();
    for (int i = tid; i < 3 * K; i += kInT) sX[i] = 0.0;
    if (tid < 9) xs[tid] = 0.0;
    __syncthreads();

    auto edge_err = [&](int e, const double *vel, const GsState &S, double *err, double *eR, double *dvw, double *dpw) {
        const size_t a = k0 + A.kf1[e0 + e], b = k0 + A.kf2[e0 + e];
        gs_error(A.pre + (e0 + e) * kPF, A.Rwb + 9 * a, A.twb + 3 * a, vel + 3 * a, A.Rwb + 9 * b, A.twb + 3 * b, vel + 3 * b,
                 S, err, eR, dvw, dpw);
    };
    // computeActiveErrors + activeRobustChi2 at the trial (velT, sE[1])
    auto chi2_trial = [&]() -> double {
        const double *vel = A.velT;
        const InEst &x = sE[1];
        const GsState &S = sS[1];
        double c = 0.0;
        for (int e = tid; e < E; e += kInT) {
            double er[9];
            edge_err(e, vel, S, er, nullptr, nullptr, nullptr);
            const double *Om = A.info + (e0 + e) * 81;
            double chi = 0.0;
            for (int r = 0; r < 9; ++r) {
                double t = 0.0;
                for (int q = 0; q < 9; ++q) t += Om[r * 9 + q] * er[q];
                chi += er[r] * t;
            }
            if (gsmode) {
                double r0, r1;
                huber(chi, 1.0, 1.0, r0, r1);
                chi = r0;
            }
            c += chi;
        }
        double tot = block_reduce_sum(c, red);
        if (!gsmode) {   // EdgePriorAcc / EdgePriorGyro: error = bprior (0) - estimate, information prior * I
            double pa = 0.0, pg = 0.0;
            for (int q = 0; q < 3; ++q) pa += x.ba[q] * (priorA * x.ba[q]), pg += x.bg[q] * (priorG * x.bg[q]);
            tot += pa + pg;
        }
        return tot;
    };

    // computeActiveErrors + buildSystem at the estimate: D0 / C0 / B0 (global), Hs / gs (LDS); returns the robust chi2
    auto build = [&](bool first) -> double {
        const GsState &S = sS[0];
        const InEst &est = sE[0];
        for (int e = tid; e < E; e += kInT) {
            double er[9], eR[9], dvw[3], dpw[3];
            edge_err(e, A.velC, S, er, eR, dvw, dpw);
            double *J = A.Jw + (e0 + e) * 144;
            gs_jacobian(A.pre + (e0 + e) * kPF, A.Rwb + 9 * (k0 + A.kf1[e0 + e]), S, er, eR, dvw, dpw, fv, fb, fg, fs, J, 16);
            for (int r = 0; r < 9; ++r) J[r * 16 + 15] = er[r];
            if (first)
                for (int r = 0; r < 9; ++r) A.dE0[(e0 + e) * 9 + r] = er[r];
        }
        __syncthreads();
        // Omega J and J^T (rho' Omega) J per edge, 16 threads each: thread `sub` owns column sub
        for (int base = 0; base < E; base += 16) {
            const int e = base + grp;
            const bool on = e < E;
            double w[9], chi = 0.0;
            if (on) {
                const double *J = A.Jw + (e0 + e) * 144, *Om = A.info + (e0 + e) * 81;
                double jc[9];
                for (int k = 0; k < 9; ++k) jc[k] = J[k * 16 + sub];
                for (int k = 0; k < 9; ++k) {
                    double t = 0.0;
                    for (int l = 0; l < 9; ++l) t += Om[k * 9 + l] * jc[l];
                    w[k] = t;
                }
                if (sub == 15)
                    for (int k = 0; k < 9; ++k) chi += jc[k] * w[k];
            }
            chi = __shfl(chi, (lane & 48) | 15, 64);
            double r0 = chi, r1 = 1.0;
            if (gsmode) huber(chi, 1.0, 1.0, r0, r1);
            if (on) {
                const double *J = A.Jw + (e0 + e) * 144;
                double *H = A.EH + (e0 + e) * 256;
                for (int r = 0; r <= sub; ++r) {
                    double t = 0.0;
                    for (int k = 0; k < 9; ++k) t += J[k * 16 + r] * w[k];
                    H[r * 16 + sub] = r == 15 ? r0 : r1 * t;
                }
            }
        }
        __syncthreads();
        // the gather per position: entering edge (as V2, columns 3-5) then leaving edge (as V1, columns 0-2)
        if (chain)
            for (int base = 0; base < K; base += 16) {
                const int p = base + grp;
                if (p >= K) continue;
                const int ein = A.edge_in[k0 + p], eout = A.edge_out[k0 + p];
                const double *Hi = ein >= 0 ? A.EH + (e0 + ein) * 256 : nullptr;
                const double *Ho = eout >= 0 ? A.EH + (e0 + eout) * 256 : nullptr;
                if (sub < 10) {
                    for (int i = 0; i < 3; ++i) {
                        const double v = (Hi ? Hi[(3 + i) * 16 + 6 + sub] : 0.0) + (Ho ? Ho[i * 16 + 6 + sub] : 0.0);
                        A.B0[(k0 + p) * 30 + i * 10 + sub] = sub == 9 ? -v : v;   // column 9: b = -J^T Omega e
                    }
                } else if (sub == 10) {
                    int q = 0;
                    for (int i = 0; i < 3; ++i)
                        for (int j = i; j < 3; ++j, ++q)
                            A.D0[(k0 + p) * 6 + q] = (Hi ? Hi[(3 + i) * 16 + 3 + j] : 0.0) + (Ho ? Ho[i * 16 + j] : 0.0);
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) A.C0[(k0 + p) * 9 + 3 * i + j] = Ho ? Ho[i * 16 + 3 + j] : 0.0;
                }
            }
        // the corner, the shared gradient and chi2: entry q of the 55 upper entries of columns 6..15, four partial sums
        {
            const int q = lane;
            int r = 0, c = q;
            for (int len = 10; r < 10 && c >= len; ++r, --len) c -= len;
            c += r;   // (r, c), r <= c, of the 10 x 10
            double acc = 0.0;
            if (q < 55)
                for (int e = wave; e < E; e += 4) acc += A.EH[(e0 + e) * 256 + (6 + r) * 16 + 6 + c];
            red2[wave * 64 + q] = acc;
            __syncthreads();
            if (tid < 55) {
                const double tot = ((red2[q] + red2[64 + q]) + red2[128 + q]) + red2[192 + q];
                if (c < 9) Hs[r * 9 + c] = tot, Hs[c * 9 + r] = tot;
                else if (r < 9) gs[r] = -tot;
                else scal[0] = tot;
            }
            __syncthreads();
            if (tid == 0 && !gsmode) {
                double pa = 0.0, pg = 0.0;
                for (int k = 0; k < 3; ++k) {
                    Hs[k * 10] += priorG, Hs[(3 + k) * 10] += priorA;
                    gs[k] += priorG * (0.0 - est.bg[k]), gs[3 + k] += priorA * (0.0 - est.ba[k]);
                    pa += est.ba[k] * (priorA * est.ba[k]), pg += est.bg[k] * (priorG * est.bg[k]);
                }
                scal[0] += pa + pg;
            }
            __syncthreads();
        }
        if (first) {
            if (chain) {
                for (int i = tid; i < 6 * K; i += kInT) A.dD[6 * k0 + i] = A.D0[6 * k0 + i];
                for (int i = tid; i < 9 * K; i += kInT) A.dC[9 * k0 + i] = A.C0[9 * k0 + i];
                for (int i = tid; i < 30 * K; i += kInT) A.dB[30 * k0 + i] = A.B0[30 * k0 + i];
            }
            if (tid < 81) A.dbg[job].corner[tid] = Hs[tid];
            if (tid < 9) A.dbg[job].bc[tid] = gs[tid];
            if (tid == 0) A.dbg[job].chi2 = scal[0];
        }
        return scal[0];
    };

    // (H + lambda I) x = b: velocities to sX (position order), the nine shared unknowns to xs; false = ok2 false (then
    // both keep what they held, as the solver's vector does)
    auto solve = [&](double lambda) -> bool {
        if (tid == 0) flag[0] = 0;
        if (chain) {
            for (int i = tid; i < 6 * K; i += kInT) {
                const int q = i % 6;
                sD[i] = A.D0[6 * k0 + i] + ((q == 0 || q == 3 || q == 5) ? lambda : 0.0);
            }
            for (int i = tid; i < 9 * K; i += kInT) sC[i] = A.C0[9 * k0 + i];
            for (int i = tid; i < 30 * K; i += kInT) sB[i] = A.B0[30 * k0 + i];
        }
        double acc[9];
        for (int r = 0; r < 9; ++r) acc[r] = 0.0;
        __syncthreads();
        if (chain) {
            for (int s = 1;; s *= 2) {
                const bool last = s >= K;   // only position 0 is left
                const int n_odd = last ? 1 : ((K - 1) / s + 1) / 2;
                for (int i = tid; i < n_odd; i += kInT) {
                    const int u = last ? 0 : s * (2 * i + 1);
                    if (!sym3_invert(sD + 6 * u)) flag[0] = 1;
                }
                __syncthreads();
                if (sub < 10)
                    for (int i = grp; i < n_odd; i += 16) {   // the eliminated positions' B^T D^-1 B, in position order
                        const int u = last ? 0 : s * (2 * i + 1);
                        const double *Bu = sB + 30 * u;
                        const double b[3] = {Bu[sub], Bu[10 + sub], Bu[20 + sub]};
                        double y[3];
                        sym3_mul(sD + 6 * u, b, y);
                        for (int r = 0; r < 9; ++r) acc[r] += Bu[r] * y[0] + Bu[10 + r] * y[1] + Bu[20 + r] * y[2];
                    }
                if (last) break;
                const int n_even = (K - 1) / (2 * s) + 1;
                for (int i = grp; i < n_even; i += 16) {
                    const int j = 2 * s * i, up = j + s, lo = j - s;
                    if (sub < 10) {
                        double *Bj = sB + 30 * j;
                        if (up < K) {
                            const double *Bu = sB + 30 * up, *Cj = sC + 9 * j;
                            const double b[3] = {Bu[sub], Bu[10 + sub], Bu[20 + sub]};
                            double y[3];
                            sym3_mul(sD + 6 * up, b, y);
                            for (int r = 0; r < 3; ++r)
                                Bj[10 * r + sub] -= Cj[3 * r] * y[0] + Cj[3 * r + 1] * y[1] + Cj[3 * r + 2] * y[2];
                        }
                        if (lo >= 0) {
                            const double *Bl = sB + 30 * lo, *Cl = sC + 9 * lo;
                            const double b[3] = {Bl[sub], Bl[10 + sub], Bl[20 + sub]};
                            double y[3];
                            sym3_mul(sD + 6 * lo, b, y);
                            for (int r = 0; r < 3; ++r) Bj[10 * r + sub] -= Cl[r] * y[0] + Cl[3 + r] * y[1] + Cl[6 + r] * y[2];
                        }
                    } else if (sub == 10) {
                        double Dj[9], nC[9];
                        sym3_full(sD + 6 * j, Dj);
                        for (int q = 0; q < 9; ++q) nC[q] = 0.0;
                        if (up < K) {
                            double Cj[9], Di[9], P[9];
                            for (int q = 0; q < 9; ++q) Cj[q] = sC[9 * j + q];
                            sym3_full(sD + 6 * up, Di);
                            mm3(Cj, Di, P);
                            for (int r = 0; r < 3; ++r)
                                for (int c = r; c < 3; ++c)
                                    Dj[3 * r + c] -= P[3 * r] * Cj[3 * c] + P[3 * r + 1] * Cj[3 * c + 1] + P[3 * r + 2] * Cj[3 * c + 2];
                            if (up + s < K) {
                                mm3(P, sC + 9 * up, nC);
                                for (int q = 0; q < 9; ++q) nC[q] = -nC[q];
                            }
                            for (int q = 0; q < 9; ++q) sL[9 * up + q] = Cj[q];   // (j, up): up's lower coupling
                        }
                        if (lo >= 0) {
                            double Cl[9], Di[9], Q[9];
                            for (int q = 0; q < 9; ++q) Cl[q] = sC[9 * lo + q];
                            sym3_full(sD + 6 * lo, Di);
                            mtm3(Cl, Di, Q);
                            for (int r = 0; r < 3; ++r)
                                for (int c = r; c < 3; ++c)
                                    Dj[3 * r + c] -= Q[3 * r] * Cl[c] + Q[3 * r + 1] * Cl[3 + c] + Q[3 * r + 2] * Cl[6 + c];
                        }
                        sD[6 * j] = Dj[0], sD[6 * j + 1] = Dj[1], sD[6 * j + 2] = Dj[2];
                        sD[6 * j + 3] = Dj[4], sD[6 * j + 4] = Dj[5], sD[6 * j + 5] = Dj[8];
                        for (int q = 0; q < 9; ++q) sL[9 * j + q] = nC[q];   // staged: sC[j] is still being read
                    }
                }
                __syncthreads();
                for (int i = tid; i < 9 * n_even; i += kInT) {
                    const int j = 2 * s * (i / 9), q = i % 9;
                    sC[9 * j + q] = sL[9 * j + q];   // (j, j + 2s)
                }
                __syncthreads();
            }
        }
        for (int r = 0; r < 9; ++r) {
            acc[r] += __shfl_xor(acc[r], 16, 64);
            acc[r] += __shfl_xor(acc[r], 32, 64);
        }
        if (lane < 10)
            for (int r = 0; r < 9; ++r) red3[(wave * 10 + lane) * 9 + r] = acc[r];
        __syncthreads();
        if (tid < 90) {
            const int r = tid / 10, c = tid % 10;
            const double t = ((red3[c * 9 + r] + red3[(10 + c) * 9 + r]) + red3[(20 + c) * 9 + r]) + red3[(30 + c) * 9 + r];
            if (c == 9) rhs[r] = gs[r] - t;
            else if (r == c) Ad[r * 9 + c] = is_free(r) ? (Hs[r * 9 + c] + lambda) - t : 1.0;
            else Ad[r * 9 + c] = Hs[r * 9 + c] - t;
        }
        __syncthreads();
        if (wave == 0) {
            const bool ok = ldlt_pick_solve<9>(Ad, rhs, xs, pick, Lm, lane);
            if (lane == 0) flag[1] = ok ? 1 : 0;
        }
        __syncthreads();
        const bool ok = flag[1] != 0 && flag[0] == 0;
        if (chain && ok) {
            auto back = [&](int u, int lo, int up) {
                const double *Bu = sB + 30 * u;
                double r[3], x[3];
                for (int i = 0; i < 3; ++i) {
                    double t = Bu[10 * i + 9];
                    for (int c = 0; c < 9; ++c) t -= Bu[10 * i + c] * xs[c];
                    r[i] = t;
                }
                if (lo >= 0) {
                    const double *L = sL + 9 * u, *xl = sX + 3 * lo;
                    for (int i = 0; i < 3; ++i) r[i] -= L[i] * xl[0] + L[3 + i] * xl[1] + L[6 + i] * xl[2];
                }
                if (up < K) {
                    const double *C = sC + 9 * u, *xu = sX + 3 * up;
                    for (int i = 0; i < 3; ++i) r[i] -= C[3 * i] * xu[0] + C[3 * i + 1] * xu[1] + C[3 * i + 2] * xu[2];
                }
                sym3_mul(sD + 6 * u, r, x);
                for (int i = 0; i < 3; ++i) sX[3 * u + i] = x[i];
            };
            if (tid == 0) back(0, -1, K);
            __syncthreads();
            int smax = 0;
            if (K > 1)
                for (smax = 1; 2 * smax < K;) smax *= 2;
            for (int s = smax; s >= 1; s >>= 1) {
                const int n_odd = ((K - 1) / s + 1) / 2;
                for (int i = tid; i < n_odd; i += kInT) {
                    const int u = s * (2 * i + 1);
                    back(u, u - s, u + s);
                }
                __syncthreads();
            }
        }
        return ok;
    };

    // update(x): the trial estimate (velocities to velT, the rest to sE[1] / sS[1])
    auto oplus = [&]() {
        if (chain)
            for (int p = tid; p < K; p += kInT) {
                const size_t k = k0 + A.order[k0 + p];
                for (int i = 0; i < 3; ++i) A.velT[3 * k + i] = A.velC[3 * k + i] + sX[3 * p + i];
            }
        if (tid == 0) {
            const InEst &est = sE[0];
            InEst &t = sE[1];
            t = est;
            if (chain)
                for (int q = 0; q < 3; ++q) t.bg[q] = est.bg[q] + xs[q], t.ba[q] = est.ba[q] + xs[3 + q];
            if (fg) {   // Rwg <- Rwg * ExpSO3(u0, u1, 0)
                const double u[3] = {xs[6], xs[7], 0.0};
                double Ex[9];
                exp_so3(u, Ex);
                mm3(est.Rwg, Ex, t.Rwg);
            }
            if (fs) t.s = est.s * exp(xs[8]);
            in_gs_state(t, sS[1]);
        }
        __syncthreads();
    };
    auto accept = [&]() {   // discardTop(): the trial becomes the estimate
        if (tid == 0) sE[0] = sE[1], sS[0] = sS[1];
        if (chain)
            for (int i = tid; i < 3 * K; i += kInT) A.velC[3 * k0 + i] = A.velT[3 * k0 + i];
        __syncthreads();
    };

    // SparseOptimizer::optimize (anything but OK ends it): OptimizationAlgorithmGaussNewton, optimize(10), in GS mode --
    // without an edge there is no vertex and it returns at once -- otherwise OptimizationAlgorithmLevenberg, optimize(200).
    // GS mode takes one more pass that only evaluates (:3920-3921, err_end).
    // The Levenberg step control below is omv_lm.h's rules WRITTEN OUT: every form of this loop that calls the header
    // moved the kernel's AGPR and SGPR-spill counts (profiles/lm_control_ab.log, section 2).  Keep the two in step.
    const int max_it = gsmode ? (E > 0 ? 10 : 0) : 200;
    int n_it = 0, n_trials = 0, most = 0, lm_bad = 0;
    float err0 = 0.f, err1 = 0.f;
    double lambda = 0.0, ni = 2.0;
    bool stop = false;
    long long ticks[3] = {0, 0, 0}, t0;
    for (int it = 0; it <= max_it && max_it > 0; ++it) {
        const bool done = it == max_it || stop;
        if (done && !gsmode) break;
        t0 = wall_clock64();
        double cur = build(it == 0);
        ticks[0] += wall_clock64() - t0;
        if (gsmode && it == 0) err0 = (float)cur;
        if (done) {
            err1 = (float)cur;
            break;
        }
        const double ini = cur;
        if (it == 0 && !gsmode) {   // computeLambdaInit; _ni and _nBad reset
            const bool user = mode == OMV_INERTIAL_BIAS || jp.priorG != 0.f;
            double md = 0.0;
            for (int i = tid; i < 6 * K; i += kInT) {
                const int q = i % 6;
                if (q == 0 || q == 3 || q == 5) md = fmax(fabs(A.D0[6 * k0 + i]), md);
            }
            md = block_reduce_max(md, red);
            for (int r = 0; r < 9; ++r)
                if (is_free(r)) md = fmax(fabs(Hs[r * 10]), md);
            lambda = user ? 1e3 : 1e-5 * md, ni = 2.0, lm_bad = 0;
            if (tid == 0) A.dbg[job].lambda_init = lambda;
        }
        ++n_it;
        int qmax = 0;
        double rho = 0.0;
        bool again = false;
        do {
            t0 = wall_clock64();
            const bool ok = solve(lambda);
            ticks[1] += wall_clock64() - t0;
            if (it == 0 && qmax == 0) {
                if (chain)
                    for (int i = tid; i < 3 * K; i += kInT) A.dX[3 * k0 + i] = sX[i];
                if (tid < 9) A.dbg[job].xc[tid] = xs[tid];
            }
            oplus();
            ++qmax, ++n_trials;
            if (gsmode) {   // Gauss-Newton: the update stays, a failed solve ends optimize()
                accept();
                stop = !ok;
                continue;
            }
            t0 = wall_clock64();
            const double c = chi2_trial();
            ticks[2] += wall_clock64() - t0;
            const double temp = ok ? c : DBL_MAX;
            double sc = 0.0;   // computeScale: x . (lambda x + b)
            for (int i = tid; i < 3 * K; i += kInT)
                sc += sX[i] * (lambda * sX[i] + A.B0[(k0 + i / 3) * 30 + (i % 3) * 10 + 9]);
            sc = block_reduce_sum(sc, red);
            for (int r = 0; r < 9; ++r)
                if (is_free(r)) sc += xs[r] * (lambda * xs[r] + gs[r]);
            sc += 1e-3;
            rho = (cur - temp) / sc;
            if (rho > 0 && isfinite(temp)) {
                const double a3 = 2 * rho - 1;
                double alpha = 1. - a3 * a3 * a3;   // pow(2 rho - 1, 3)
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                cur = temp;
                accept();
            } else {   // pop()
                lambda *= ni;
                ni *= 2;
            }
            again = rho < 0 && qmax < 10;
        } while (again);
        most = max(most, qmax);
        if (!gsmode) {
            if (qmax == 10 || rho == 0) {
                stop = true;
            } else {
                lm_bad = (ini - cur) * 1e3 < ini ? lm_bad + 1 : 0;
                if (lm_bad >= 3) stop = true;
            }
        }
    }

    // ---- the epilogue (:3619-3652, :3783-3812, :3923-3924) ----
    const InEst &est = sE[0];
    if (tid == 0) {
        InDebug &d = A.dbg[job];
        d.iterations = n_it, d.trials = n_trials, d.max_trials = most, d.err[0] = err0, d.err[1] = err1;
        for (int q = 0; q < 3; ++q) d.ticks[q] = ticks[q];
        A.iters[job] = n_it, A.trials[job] = n_trials;
        if (mode != OMV_INERTIAL_BIAS && n_it > 0) {   // BIAS has no Rwg / scale; nothing ran: the input's bits stay
            for (int q = 0; q < 9; ++q) A.Rwg_out[9 * job + q] = est.Rwg[q];
            A.scale_out[job] = est.s;
        }
        for (int q = 0; q < 3; ++q) A.bg_out[3 * job + q] = est.bg[q], A.ba_out[3 * job + q] = est.ba[q];
    }
    const float bgf[3] = {(float)est.bg[0], (float)est.bg[1], (float)est.bg[2]};
    for (int k = tid; k < K; k += kInT) {
        for (int i = 0; i < 3; ++i) {
            const double v = A.velC[3 * (k0 + k) + i];
            A.vel_out[3 * (k0 + k) + i] = v;
            A.velf_out[3 * (k0 + k) + i] = (float)v;   // SetVelocity(Vw.cast<float>())
        }
        uint8_t re = 0;
        if (!gsmode) {   // (pKFi->GetGyroBias() - bg.cast<float>()).norm() > 0.01
            const float *ob = A.old_bg + 3 * (k0 + k);
            const float d0 = ob[0] - bgf[0], d1 = ob[1] - bgf[1], d2 = ob[2] - bgf[2];
            const float n = sqrtf_cr((d0 * d0 + d1 * d1) + d2 * d2);
            re = (double)n > 0.01 ? 1 : 0;
        }
        A.reint[k0 + k] = re;
    }
}

}  // namespace

struct omv_inertial_opt {
    int max_jobs = 0, max_kf = 0, max_edges = 0, n_jobs = 0;
    std::vector<int32_t> kf_start, edge_start, kf1, kf2, order;   // of the last call (the debug hook's index maps)
    // device: the call's inputs (one upload through h_in), the workspace, the outputs (one read-back through h_out)
    char *d_in = nullptr, *h_in = nullptr, *d_out = nullptr, *h_out = nullptr;
    double *d_ws = nullptr, *d_dbgv = nullptr;
    InDebug *d_dbg = nullptr;
    omv::DeviceArena mem;
};

namespace {
// bytes per job / keyframe / edge of the upload and read-back blocks, every array 8-byte aligned
constexpr size_t kInJobIn = sizeof(InJob), kInKfIn = (9 + 3 + 3) * 8 + 3 * 4 + 3 * 4 + 8, kInEdgeIn = 2 * 4 + (size_t)OMV_PREINT_FLOATS * 4 + 8;
constexpr size_t kInJobOut = (9 + 1 + 3 + 3) * 8 + 2 * 4 + 8, kInKfOut = 3 * 8 + 3 * 4 + 1 + 8;
constexpr size_t kInWsKf = 6 + 9 + 30 + 3 + 3, kInWsEdge = 81 + 144 + 256, kInDbgKf = 6 + 9 + 30 + 3, kInDbgEdge = 9;
static_assert(sizeof(InJob) % 8 == 0, "arrays of doubles follow the jobs");
inline size_t up8(size_t n) { return (n + 7) & ~(size_t)7; }
}  // namespace

extern "C" {

omv_status omv_inertial_opt_create(int max_jobs, int max_kf_total, int max_edges_total, omv_inertial_opt **out) {
    if (!out || max_jobs <= 0 || max_kf_total <= 0 || max_edges_total <= 0) return OMV_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OMV_ERR_NO_DEVICE;
    auto h = std::make_unique<omv_inertial_opt>();
    h->max_jobs = max_jobs, h->max_kf = max_kf_total, h->max_edges = max_edges_total;
    const size_t J = max_jobs, Kt = max_kf_total, Et = max_edges_total;
    const size_t in_bytes = J * kInJobIn + Kt * kInKfIn + Et * kInEdgeIn + 256, out_bytes = J * kInJobOut + Kt * kInKfOut + 256;
    omv::DeviceArena &mem = h->mem;
    if (!mem.alloc(&h->d_in, in_bytes) || !mem.alloc_pinned(&h->h_in, in_bytes) || !mem.alloc(&h->d_out, out_bytes) ||
        !mem.alloc_pinned(&h->h_out, out_bytes) || !mem.alloc(&h->d_ws, Kt * kInWsKf + Et * kInWsEdge) ||
        !mem.alloc(&h->d_dbgv, Kt * kInDbgKf + Et * kInDbgEdge) || !mem.alloc(&h->d_dbg, J))
        return OMV_ERR_HIP;
    if (hipFuncSetAttribute((const void *)inertial_opt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((size_t)OMV_INERTIAL_MAX_KF * kInNode * 8)) != hipSuccess) {
        (void)hipGetLastError();
        return OMV_ERR_HIP;
    }
    *out = h.release();
    return OMV_OK;
}

omv_status omv_inertial_opt_destroy(omv_inertial_opt *h) {
    if (!h) return OMV_ERR_ARG;
    delete h;
    return OMV_OK;
}

omv_status omv_inertial_optimization(omv_inertial_opt *h, int n_jobs, const int32_t *kf_start, const int32_t *edge_start,
                                     const double *Rwb, const double *twb, const double *vel_in, const float *old_gyro_bias,
                                     const int32_t *edge_kf1, const int32_t *edge_kf2, const float *preint,
                                     const double *bg0, const double *ba0, const int32_t *mode, const int32_t *mono,
                                     const float *priorG, const float *priorA, double *Rwg, double *scale, double *bg,
                                     double *ba, double *vel, float *vel_f32, uint8_t *reintegrate, int32_t *iterations,
                                     int32_t *trials, void *stream) {
    if (!h || n_jobs < 0 || n_jobs > h->max_jobs) return OMV_ERR_ARG;
    if (n_jobs > 0 && (!kf_start || !edge_start || !bg0 || !ba0 || !mode || !mono || !priorG || !priorA || !Rwg || !scale ||
                       !bg || !ba || !iterations || !trials))
        return OMV_ERR_ARG;
    if (n_jobs > 0 && (kf_start[0] != 0 || edge_start[0] != 0)) return OMV_ERR_ARG;
    int max_k = 0;
    for (int j = 0; j < n_jobs; j++) {
        const int K = kf_start[j + 1] - kf_start[j], E = edge_start[j + 1] - edge_start[j];
        if (K < 0 || E < 0 || K > OMV_INERTIAL_MAX_KF) return OMV_ERR_ARG;
        if (mode[j] != OMV_INERTIAL_FULL && mode[j] != OMV_INERTIAL_BIAS && mode[j] != OMV_INERTIAL_GS) return OMV_ERR_ARG;
        max_k = std::max(max_k, K);
    }
    const int Kt = n_jobs ? kf_start[n_jobs] : 0, Et = n_jobs ? edge_start[n_jobs] : 0;
    if (Kt > h->max_kf || Et > h->max_edges) return OMV_ERR_ARG;
    if (Kt > 0 && (!Rwb || !twb || !vel_in || !old_gyro_bias || !vel || !vel_f32 || !reintegrate)) return OMV_ERR_ARG;
    if (Et > 0 && (!edge_kf1 || !edge_kf2 || !preint)) return OMV_ERR_ARG;
    // the plans: a keyframe with two successors or predecessors, an index out of range, a cycle are argument errors
    std::vector<int32_t> order((size_t)Kt), ein((size_t)Kt), eout((size_t)Kt);
    omv_inertial::Plan plan;
    for (int j = 0; j < n_jobs; j++) {
        const int k0 = kf_start[j], K = kf_start[j + 1] - k0, e0 = edge_start[j], E = edge_start[j + 1] - e0;
        if (!omv_inertial::plan_paths(K, E, E ? edge_kf1 + e0 : nullptr, E ? edge_kf2 + e0 : nullptr, &plan)) return OMV_ERR_ARG;
        std::copy(plan.order.begin(), plan.order.end(), order.begin() + k0);
        std::copy(plan.edge_in.begin(), plan.edge_in.end(), ein.begin() + k0);
        std::copy(plan.edge_out.begin(), plan.edge_out.end(), eout.begin() + k0);
    }
    h->n_jobs = n_jobs;
    h->kf_start.assign(kf_start, kf_start + (n_jobs ? n_jobs + 1 : 0));
    h->edge_start.assign(edge_start, edge_start + (n_jobs ? n_jobs + 1 : 0));
    h->kf1.assign(edge_kf1, edge_kf1 + Et), h->kf2.assign(edge_kf2, edge_kf2 + Et);
    h->order = order;
    if (n_jobs == 0) return OMV_OK;

    // ---- the upload block ----
    const size_t J = n_jobs, K8 = Kt, E8 = Et;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = up8(off + bytes);
        return o;
    };
    const size_t o_jobs = take(J * sizeof(InJob)), o_Rwb = take(K8 * 72), o_twb = take(K8 * 24), o_vel = take(K8 * 24);
    const size_t o_obg = take(K8 * 12), o_ord = take(K8 * 4), o_ein = take(K8 * 4), o_eout = take(K8 * 4);
    const size_t o_kf1 = take(E8 * 4), o_kf2 = take(E8 * 4), o_pre = take(E8 * OMV_PREINT_FLOATS * 4);
    const size_t in_bytes = off;
    InJob *jobs = reinterpret_cast<InJob *>(h->h_in + o_jobs);
    for (int j = 0; j < n_jobs; j++) {
        InJob &p = jobs[j];
        p.k0 = kf_start[j], p.K = kf_start[j + 1] - kf_start[j], p.e0 = edge_start[j], p.E = edge_start[j + 1] - edge_start[j];
        p.mode = mode[j], p.mono = mono[j] != 0, p.priorG = priorG[j], p.priorA = priorA[j];
        for (int q = 0; q < 3; q++) p.bg0[q] = bg0[3 * j + q], p.ba0[q] = ba0[3 * j + q];
        for (int q = 0; q < 9; q++) p.Rwg[q] = Rwg[9 * j + q];
        p.scale = scale[j];
    }
    auto put = [&](size_t o, const void *src, size_t bytes) {
        if (bytes) std::copy((const char *)src, (const char *)src + bytes, h->h_in + o);
    };
    put(o_Rwb, Rwb, K8 * 72), put(o_twb, twb, K8 * 24), put(o_vel, vel_in, K8 * 24), put(o_obg, old_gyro_bias, K8 * 12);
    put(o_ord, order.data(), K8 * 4), put(o_ein, ein.data(), K8 * 4), put(o_eout, eout.data(), K8 * 4);
    put(o_kf1, edge_kf1, E8 * 4), put(o_kf2, edge_kf2, E8 * 4), put(o_pre, preint, E8 * OMV_PREINT_FLOATS * 4);
    // ---- the read-back block ----
    off = 0;
    const size_t r_Rwg = take(J * 72), r_s = take(J * 8), r_bg = take(J * 24), r_ba = take(J * 24), r_vel = take(K8 * 24);
    const size_t r_velf = take(K8 * 12), r_re = take(K8), r_it = take(J * 4), r_tr = take(J * 4);
    const size_t out_bytes = off;

    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(h->d_in, h->h_in, in_bytes, hipMemcpyHostToDevice, st));
    InArgs A;
    A.jobs = reinterpret_cast<const InJob *>(h->d_in + o_jobs);
    A.Rwb = reinterpret_cast<const double *>(h->d_in + o_Rwb), A.twb = reinterpret_cast<const double *>(h->d_in + o_twb);
    A.vel_in = reinterpret_cast<const double *>(h->d_in + o_vel), A.old_bg = reinterpret_cast<const float *>(h->d_in + o_obg);
    A.order = reinterpret_cast<const int32_t *>(h->d_in + o_ord), A.edge_in = reinterpret_cast<const int32_t *>(h->d_in + o_ein);
    A.edge_out = reinterpret_cast<const int32_t *>(h->d_in + o_eout);
    A.kf1 = reinterpret_cast<const int32_t *>(h->d_in + o_kf1), A.kf2 = reinterpret_cast<const int32_t *>(h->d_in + o_kf2);
    A.pre = reinterpret_cast<const float *>(h->d_in + o_pre);
    const size_t cK = h->max_kf, cE = h->max_edges;
    double *w = h->d_ws;
    A.D0 = w, w += 6 * cK, A.C0 = w, w += 9 * cK, A.B0 = w, w += 30 * cK, A.velC = w, w += 3 * cK, A.velT = w, w += 3 * cK;
    A.info = w, w += 81 * cE, A.Jw = w, w += 144 * cE, A.EH = w;
    w = h->d_dbgv;
    A.dD = w, w += 6 * cK, A.dC = w, w += 9 * cK, A.dB = w, w += 30 * cK, A.dX = w, w += 3 * cK, A.dE0 = w;
    A.dbg = h->d_dbg;
    A.Rwg_out = reinterpret_cast<double *>(h->d_out + r_Rwg), A.scale_out = reinterpret_cast<double *>(h->d_out + r_s);
    A.bg_out = reinterpret_cast<double *>(h->d_out + r_bg), A.ba_out = reinterpret_cast<double *>(h->d_out + r_ba);
    A.vel_out = reinterpret_cast<double *>(h->d_out + r_vel), A.velf_out = reinterpret_cast<float *>(h->d_out + r_velf);
    A.reint = reinterpret_cast<uint8_t *>(h->d_out + r_re);
    A.iters = reinterpret_cast<int32_t *>(h->d_out + r_it), A.trials = reinterpret_cast<int32_t *>(h->d_out + r_tr);
    HIP_OK(hipMemsetAsync(h->d_dbg, 0, J * sizeof(InDebug), st));
    HIP_OK(hipMemsetAsync(h->d_dbgv, 0, (cK * kInDbgKf + cE * kInDbgEdge) * sizeof(double), st));
    const size_t lds = std::max((size_t)max_k * kInNode, (size_t)kInInfoLds) * sizeof(double);
    inertial_opt_kernel<<<n_jobs, kInT, lds, st>>>(A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h->h_out, h->d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // Rwg and scale come back only where the kernel wrote them (not in BIAS mode, not when nothing ran): otherwise the
    // caller's values stay, bit for bit
    const int32_t *it = reinterpret_cast<const int32_t *>(h->h_out + r_it);
    const double *oR = reinterpret_cast<const double *>(h->h_out + r_Rwg), *os = reinterpret_cast<const double *>(h->h_out + r_s);
    for (int j = 0; j < n_jobs; j++)
        if (mode[j] != OMV_INERTIAL_BIAS && it[j] > 0) {
            std::copy(oR + 9 * j, oR + 9 * j + 9, Rwg + 9 * j);
            scale[j] = os[j];
        }
    auto get = [&](size_t o, void *dst, size_t bytes) {
        if (bytes) std::copy(h->h_out + o, h->h_out + o + bytes, (char *)dst);
    };
    get(r_bg, bg, J * 24), get(r_ba, ba, J * 24), get(r_vel, vel, K8 * 24), get(r_velf, vel_f32, K8 * 12);
    get(r_re, reintegrate, K8), get(r_it, iterations, J * 4), get(r_tr, trials, J * 4);
    return OMV_OK;
}

omv_status omv_inertial_opt_debug(omv_inertial_opt *h, int job, double *e0, double *Hvv, double *Hvoff, double *border,
                                  double *bv, double *corner, double *bc, double *chi2, double *lambda_init, double *xv,
                                  double *xc, int32_t *iterations, int32_t *trials, int32_t *max_trials, float *err,
                                  int64_t *ticks, void *stream) {
    if (!h || job < 0 || job >= h->n_jobs) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int k0 = h->kf_start[job], K = h->kf_start[job + 1] - k0, e0i = h->edge_start[job], E = h->edge_start[job + 1] - e0i;
    const size_t cK = h->max_kf;
    std::vector<double> D(6 * (size_t)K), C(9 * (size_t)K), B(30 * (size_t)K), X(3 * (size_t)K), E0(9 * (size_t)E);
    InDebug d;
    const double *w = h->d_dbgv;
    HIP_OK(hipMemcpyAsync(&d, h->d_dbg + job, sizeof(d), hipMemcpyDeviceToHost, st));
    if (K > 0) {
        HIP_OK(hipMemcpyAsync(D.data(), w + 6 * (size_t)k0, D.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(C.data(), w + 6 * cK + 9 * (size_t)k0, C.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(B.data(), w + 15 * cK + 30 * (size_t)k0, B.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(X.data(), w + 45 * cK + 3 * (size_t)k0, X.size() * 8, hipMemcpyDeviceToHost, st));
    }
    if (E > 0) HIP_OK(hipMemcpyAsync(E0.data(), w + 48 * cK + 9 * (size_t)e0i, E0.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<int> pos((size_t)K);
    for (int p = 0; p < K; p++) pos[h->order[k0 + p]] = p;
    static const int sym[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    for (int k = 0; k < K; k++) {
        const int p = pos[k];
        for (int q = 0; q < 9; q++)
            if (Hvv) Hvv[9 * k + q] = D[6 * p + sym[q]];
        for (int i = 0; i < 3; i++) {
            for (int c = 0; c < 9; c++)
                if (border) border[27 * k + 9 * i + c] = B[30 * p + 10 * i + c];
            if (bv) bv[3 * k + i] = B[30 * p + 10 * i + 9];
            if (xv) xv[3 * k + i] = X[3 * p + i];
        }
    }
    for (int e = 0; e < E; e++) {
        const int p = pos[h->kf1[e0i + e]];
        for (int q = 0; q < 9; q++) {
            if (Hvoff) Hvoff[9 * e + q] = C[9 * p + q];
            if (e0) e0[9 * e + q] = E0[9 * e + q];
        }
    }
    if (corner) std::copy(d.corner, d.corner + 81, corner);
    if (bc) std::copy(d.bc, d.bc + 9, bc);
    if (xc) std::copy(d.xc, d.xc + 9, xc);
    if (chi2) *chi2 = d.chi2;
    if (lambda_init) *lambda_init = d.lambda_init;
    if (iterations) *iterations = d.iterations;
    if (trials) *trials = d.trials;
    if (max_trials) *max_trials = d.max_trials;
    if (err) err[0] = d.err[0], err[1] = d.err[1];
    if (ticks) std::copy(d.ticks, d.ticks + 3, ticks);
    return OMV_OK;
}

/* Test hook, host only: the planner of inertial_plan.h on one job. */
omv_status omv_inertial_opt_plan(int K, int E, const int32_t *kf1, const int32_t *kf2, int32_t *order, int32_t *pos_of,
                                 int32_t *edge_in, int32_t *edge_out, int32_t *n_paths) {
    omv_inertial::Plan P;
    if (!omv_inertial::plan_paths(K, E, kf1, kf2, &P)) return OMV_ERR_ARG;
    if (order) std::copy(P.order.begin(), P.order.end(), order);
    if (pos_of) std::copy(P.pos_of.begin(), P.pos_of.end(), pos_of);
    if (edge_in) std::copy(P.edge_in.begin(), P.edge_in.end(), edge_in);
    if (edge_out) std::copy(P.edge_out.begin(), P.edge_out.end(), edge_out);
    if (n_paths) *n_paths = P.n_paths;
    return OMV_OK;
}

}  // extern "C"
