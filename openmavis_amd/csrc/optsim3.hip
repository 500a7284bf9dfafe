// MI355X-native Optimizer::OptimizeSim3 (src/Optimizer.cc:2460-2726): the Sim3 refinement LoopClosing runs on every
// loop / merge candidate (src/LoopClosing.cc:658, :899, :935), batched over J independent candidate pairs ("jobs").
//
// The graph: one VertexSim3Expmap (g2o::Sim3 S12: quaternion, t, s; oplus = Sim3(update) * S12 with update[6] forced
// to 0 under _fix_scale) and per accepted correspondence the pair EdgeSim3ProjectXYZ (obs1 - project1(S12 X2)) /
// EdgeInverseSim3ProjectXYZ (obs2 - project2(S12^-1 X1)) on fixed points, Huber sqrt(th2).  Two rounds of g2o's
// Levenberg-Marquardt, the step control from omv_lm.h: optimize(10); the pairs whose stale chi2 exceeds th2
// removed, the rest without robust kernel; the return before the write-back when fewer than 10 are left; optimize(10
// or 5); a fresh computeError per kept pair.  The reference differentiates both edges numerically (linearizeOplus is
// commented out: central differences with delta 1e-9); here the Jacobians are analytic, with Y = S12 X2,
// Z = S12^-1 X1 and the update ordered (omega, upsilon, sigma):
//     d e12 / d u = -Jpi1(Y) [ -[Y]x | I | Y ]        d e21 / d u = -Jpi2(Z) (R^T / s) [ [X1]x | -I | -X1 ]
// One wavefront per job: lane l owns the pairs l, l + 64, ...; a pair's two chi2 values and its status live in the
// handle's per-entry arrays, touched by that lane only; the 28 + 7 + 1 sums of a buildSystem are accumulated per lane
// over the passes in pair order and summed over the wave by one fixed butterfly (wave_transpose_sum), so the result is
// the same run to run; the 7 x 7 solve is ldlt_pick_solve<7>; the estimate, the LM state and the Sim3 exponential are
// wave-uniform (every lane computes them).  No block barrier, no atomics.  The host side packs a call's arrays into
// one pinned block: one upload, one launch, one read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <vector>

#include "../../include/omv.h"
#include "g2o_types.h"
#include "omv_device.h"
#include "omv_host.h"
#include "omv_lm.h"

namespace {

using namespace omv_g2o;

struct OptSim3Job {
    int start, n, model1, model2, fix_scale;
    float th2;
    float pose1[12], pose2[12], cam1[8], cam2[8];
};
struct OptSim3Debug {   // the first buildSystem of a job and the LM counts per round
    double H[49], b[7], chi2, lambda_init, x[7];
    int32_t iterations[2], trials[2], max_trials[2];
};
struct OptSim3Args {
    const OptSim3Job *jobs;
    const float *Xw1, *Xw2, *obs1, *w1, *obs2_in, *w2;
    const uint8_t *has_kp2;
    float *X1, *X2, *obs2;     // prepared: P3D1c, P3D2c [n][3], obs2 [n][2]
    double *c12, *c21;         // the edges' chi2 of the last computeError
    double *e0;                // [n][4]: e12, e21 at the input estimate (debug)
    uint8_t *status;
    const double *S_in;        // [J][8] q (x y z w), t, s
    double *S;                 // the same, out
    int32_t *n_in;
    OptSim3Debug *dbg;
};
// Sim3d, sim3_exp, sim3_mul, sim3_inverse and sim3_map: g2o_types.h (the pose graph shares them).

__device__ __forceinline__ void os3_project(int model, const float *k, const double *X, double &u, double &v) {
    if (model == OMV_CAM_PINHOLE) pinhole_project(k, X, u, v);
    else kb8_project(k, X, u, v);
}
__device__ __forceinline__ void os3_project_jac(int model, const float *k, const double *X, double &u, double &v,
                                                double *pj) {
    if (model == OMV_CAM_PINHOLE) {
        pinhole_project(k, X, u, v);
        pinhole_jac(k, X, pj);
    } else {
        kb8_project(k, X, u, v);
        kb8_jac(k, X, pj);
    }
}

struct OptSim3Pair {
    double X1[3], X2[3], obs1[2], obs2[2], w1, w2;
};
__device__ __forceinline__ OptSim3Pair os3_pair(const OptSim3Args &A, size_t e) {
    OptSim3Pair p;
    for (int k = 0; k < 3; ++k) p.X1[k] = (double)A.X1[3 * e + k], p.X2[k] = (double)A.X2[3 * e + k];
    for (int k = 0; k < 2; ++k) p.obs1[k] = (double)A.obs1[2 * e + k], p.obs2[k] = (double)A.obs2[2 * e + k];
    p.w1 = (double)A.w1[e], p.w2 = (double)A.w2[e];
    return p;
}

constexpr int kOs3Sums = 36;   // 28 upper-triangle H terms, 7 b terms, the robust chi2

__global__ void __launch_bounds__(64) optimize_sim3_kernel(OptSim3Args A) {
    const int job = blockIdx.x, lane = threadIdx.x;
    __shared__ double Hs[49], Ad[49], gs[7], xs[7], Lm[49], sums[kOs3Sums];
    __shared__ int pick[8];
    const OptSim3Job &jp = A.jobs[job];
    const int n = jp.n, model1 = jp.model1, model2 = jp.model2;
    const size_t e0 = (size_t)jp.start;
    const bool fix_scale = jp.fix_scale != 0;
    float cam1[8], cam2[8];
    for (int k = 0; k < 8; ++k) cam1[k] = jp.cam1[k], cam2[k] = jp.cam2[k];
    const double th2 = (double)jp.th2;
    // const float deltaHuber = sqrt(th2)
    const double delta = (double)(float)sqrt((double)jp.th2), dsqr = delta * delta;

    // ---- the graph's numeric part (:2541-2653), float in the reference's order ----
    int n_corr = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool edge = false;
        if (i < n) {
            const size_t e = e0 + i;
            float Y1[3], Y2[3];
            for (int r = 0; r < 3; ++r) {   // P3D1c = R1w P3D1w + t1w: a 3-term sum left to right, then the translation
                Y1[r] = ((jp.pose1[3 * r] * A.Xw1[3 * e] + jp.pose1[3 * r + 1] * A.Xw1[3 * e + 1]) +
                         jp.pose1[3 * r + 2] * A.Xw1[3 * e + 2]) + jp.pose1[9 + r];
                Y2[r] = ((jp.pose2[3 * r] * A.Xw2[3 * e] + jp.pose2[3 * r + 1] * A.Xw2[3 * e + 1]) +
                         jp.pose2[3 * r + 2] * A.Xw2[3 * e + 2]) + jp.pose2[9 + r];
            }
            edge = !(Y2[2] < 0);   // `if (P3D2c(2) < 0) continue;`: not an edge, the match stays
            float u = A.obs2_in[2 * e], v = A.obs2_in[2 * e + 1];
            if (!A.has_kp2[e]) omv::cam_project_f(model2, jp.cam2, Y2, u, v);   // obs2 = pCamera2->project(P3D2c), float
            for (int r = 0; r < 3; ++r) A.X1[3 * e + r] = Y1[r], A.X2[3 * e + r] = Y2[r];
            A.obs2[2 * e] = u, A.obs2[2 * e + 1] = v;
            A.status[e] = edge ? 1 : 0;
            A.c12[e] = 0.0, A.c21[e] = 0.0;
            for (int k = 0; k < 4; ++k) A.e0[4 * e + k] = 0.0;
        }
        n_corr += __popcll(__ballot(edge));
    }

    Sim3d S;
    for (int k = 0; k < 4; ++k) S.q[k] = A.S_in[8 * job + k];
    for (int k = 0; k < 3; ++k) S.t[k] = A.S_in[8 * job + 4 + k];
    S.s = A.S_in[8 * job + 7];
    if (lane < 7) xs[lane] = 0.0;   // the dense solver's x: kept when a factorisation is not positive
    omv::wave_lds_sync();
    OptSim3Debug *dbg = A.dbg + job;
    int n_active = n_corr, n_bad = 0;

    for (int round = 0; round < 2; ++round) {
        const bool robust = round == 0;
        const int max_it = round == 0 ? 10 : (n_bad > 0 ? 10 : 5);
        int n_it = 0, n_trials = 0, most_trials = 0;
        omv_lm::LmState lm{0.0, 2.0, 0.0, 0.0, 0, 0};
        // initializeOptimization finds the vertex through its edges: without one optimize() returns at once
        for (int it = 0; it < max_it && n_active > 0; ++it) {
            // computeActiveErrors + buildSystem at the current estimate
            const Sim3d Sinv = sim3_inverse(S);
            double Rm[9], Rts[9];
            q_to_mat(S.q, Rm);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Rts[3 * r + c] = Rm[3 * c + r] / S.s;
            double acc[kOs3Sums];
            for (int q = 0; q < kOs3Sums; ++q) acc[q] = 0.0;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                if (i < n && A.status[e0 + i] == 1) {
                    const size_t e = e0 + i;
                    const OptSim3Pair p = os3_pair(A, e);
                    double Y[3], Z[3], pj[6], u, v, J12[14], J21[14], M[6];
                    sim3_map(S, p.X2, Y);
                    os3_project_jac(model1, cam1, Y, u, v, pj);
                    const double r12[2] = {p.obs1[0] - u, p.obs1[1] - v};
                    for (int r = 0; r < 2; ++r) {   // -Jpi1 [ -[Y]x | I | Y ]
                        const double a = pj[3 * r], b = pj[3 * r + 1], c = pj[3 * r + 2];
                        J12[7 * r + 0] = -(c * Y[1] - b * Y[2]);
                        J12[7 * r + 1] = -(a * Y[2] - c * Y[0]);
                        J12[7 * r + 2] = -(b * Y[0] - a * Y[1]);
                        J12[7 * r + 3] = -a, J12[7 * r + 4] = -b, J12[7 * r + 5] = -c;
                        J12[7 * r + 6] = fix_scale ? 0.0 : -(a * Y[0] + b * Y[1] + c * Y[2]);
                    }
                    sim3_map(Sinv, p.X1, Z);
                    os3_project_jac(model2, cam2, Z, u, v, pj);
                    const double r21[2] = {p.obs2[0] - u, p.obs2[1] - v};
                    for (int r = 0; r < 2; ++r)
                        for (int c = 0; c < 3; ++c)
                            M[3 * r + c] = pj[3 * r] * Rts[c] + pj[3 * r + 1] * Rts[3 + c] + pj[3 * r + 2] * Rts[6 + c];
                    for (int r = 0; r < 2; ++r) {   // -Jpi2 (R^T / s) [ [X1]x | -I | -X1 ]
                        const double a = M[3 * r], b = M[3 * r + 1], c = M[3 * r + 2];
                        J21[7 * r + 0] = -(b * p.X1[2] - c * p.X1[1]);
                        J21[7 * r + 1] = -(c * p.X1[0] - a * p.X1[2]);
                        J21[7 * r + 2] = -(a * p.X1[1] - b * p.X1[0]);
                        J21[7 * r + 3] = a, J21[7 * r + 4] = b, J21[7 * r + 5] = c;
                        J21[7 * r + 6] = fix_scale ? 0.0 : (a * p.X1[0] + b * p.X1[1] + c * p.X1[2]);
                    }
                    const double c12 = r12[0] * (p.w1 * r12[0]) + r12[1] * (p.w1 * r12[1]);
                    const double c21 = r21[0] * (p.w2 * r21[0]) + r21[1] * (p.w2 * r21[1]);
                    A.c12[e] = c12, A.c21[e] = c21;
                    if (round == 0 && it == 0) {
                        A.e0[4 * e] = r12[0], A.e0[4 * e + 1] = r12[1];
                        A.e0[4 * e + 2] = r21[0], A.e0[4 * e + 3] = r21[1];
                    }
                    double a0 = c12, a1 = 1.0, b0 = c21, b1 = 1.0;
                    if (robust) huber(c12, delta, dsqr, a0, a1), huber(c21, delta, dsqr, b0, b1);
                    const double wa = p.w1 * a1, wb = p.w2 * b1;
                    const double oa[2] = {-p.w1 * r12[0] * a1, -p.w1 * r12[1] * a1};
                    const double ob[2] = {-p.w2 * r21[0] * b1, -p.w2 * r21[1] * b1};
                    int q = 0;
#pragma unroll
                    for (int r = 0; r < 7; ++r)
#pragma unroll
                        for (int c = r; c < 7; ++c, ++q)
                            acc[q] += wa * (J12[r] * J12[c] + J12[7 + r] * J12[7 + c]) +
                                      wb * (J21[r] * J21[c] + J21[7 + r] * J21[7 + c]);
#pragma unroll
                    for (int r = 0; r < 7; ++r)
                        acc[28 + r] += (J12[r] * oa[0] + J12[7 + r] * oa[1]) + (J21[r] * ob[0] + J21[7 + r] * ob[1]);
                    acc[35] += a0 + b0;
                }
            }
            {
                const double tot = wave_transpose_sum<kOs3Sums>(acc, lane);
                if (lane < kOs3Sums) sums[lane] = tot;
                omv::wave_lds_sync();
                if (lane < 49) {
                    const int r = lane / 7, c = lane % 7, lo = min(r, c), hi = max(r, c);
                    Hs[lane] = sums[lo * 7 - lo * (lo - 1) / 2 + (hi - lo)];
                }
                if (lane < 7) gs[lane] = sums[28 + lane];
                omv::wave_lds_sync();
            }
            double md = 0;   // computeLambdaInit's maximum of |H_jj|
            if (it == 0)
                for (int j = 0; j < 7; ++j) md = fmax(fabs(Hs[8 * j]), md);
            omv_lm::lm_begin_iteration(lm, it, sums[35], omv_lm::lm_lambda_init(0.0, md));
            if (round == 0 && it == 0) {
                if (lane < 49) dbg->H[lane] = Hs[lane];
                if (lane < 7) dbg->b[lane] = gs[lane];
                if (lane == 0) dbg->chi2 = lm.currentChi, dbg->lambda_init = lm.lambda;
            }
            ++n_it;
            omv_lm::LmNext next;
            do {
                if (lane < 49) Ad[lane] = Hs[lane] + ((lane % 8 == 0) ? lm.lambda : 0.0);
                omv::wave_lds_sync();
                const bool ok = ldlt_pick_solve<7>(Ad, gs, xs, pick, Lm, lane);
                omv::wave_lds_sync();
                double x[7];
                for (int j = 0; j < 7; ++j) x[j] = xs[j];
                if (round == 0 && it == 0 && lm.qmax == 0 && lane < 7) dbg->x[lane] = xs[lane];
                if (fix_scale) x[6] = 0;   // oplusImpl
                const Sim3d St = sim3_mul(sim3_exp(x), S);
                const Sim3d Sti = sim3_inverse(St);
                // computeActiveErrors at the trial estimate
                double c = 0.0;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    if (i < n && A.status[e0 + i] == 1) {
                        const size_t e = e0 + i;
                        const OptSim3Pair p = os3_pair(A, e);
                        double Y[3], Z[3], u, v;
                        sim3_map(St, p.X2, Y);
                        os3_project(model1, cam1, Y, u, v);
                        const double r12[2] = {p.obs1[0] - u, p.obs1[1] - v};
                        sim3_map(Sti, p.X1, Z);
                        os3_project(model2, cam2, Z, u, v);
                        const double r21[2] = {p.obs2[0] - u, p.obs2[1] - v};
                        const double c12 = r12[0] * (p.w1 * r12[0]) + r12[1] * (p.w1 * r12[1]);
                        const double c21 = r21[0] * (p.w2 * r21[0]) + r21[1] * (p.w2 * r21[1]);
                        A.c12[e] = c12, A.c21[e] = c21;
                        double a0 = c12, a1, b0 = c21, b1;
                        if (robust) huber(c12, delta, dsqr, a0, a1), huber(c21, delta, dsqr, b0, b1);
                        c += a0 + b0;
                    }
                }
                for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
                double sc = 0;   // computeScale
                for (int j = 0; j < 7; ++j) sc += x[j] * (lm.lambda * x[j] + gs[j]);
                const omv_lm::LmTrial tr = omv_lm::lm_trial(lm, c, ok, sc);
                if (tr.accepted) S = St;   // else pop(): the estimate restored, the edges keep the rejected trial's errors
                ++n_trials;
                next = omv_lm::lm_next(lm, tr.rho, 10);
            } while (next == omv_lm::kLmTrial);
            most_trials = max(most_trials, lm.qmax);
            if (next == omv_lm::kLmStop) break;
        }
        if (lane == 0) dbg->iterations[round] = n_it, dbg->trials[round] = n_trials, dbg->max_trials[round] = most_trials;
        if (round == 0) {   // :2660-2696: the stale chi2 of the last computeActiveErrors decides
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                bool bad = false;
                if (i < n && A.status[e0 + i] == 1) {
                    bad = A.c12[e0 + i] > th2 || A.c21[e0 + i] > th2;   // false for a NaN
                    if (bad) A.status[e0 + i] = 2;
                }
                n_bad += __popcll(__ballot(bad));
            }
            n_active = n_corr - n_bad;
            if (n_corr - n_bad < 10) {   // return 0 before the write-back: g2oS12 stays, the round-one removals too
                for (int i = lane; i < n; i += 64)
                    if (A.status[e0 + i] == 1) A.status[e0 + i] = 0;
                if (lane < 8) A.S[8 * job + lane] = A.S_in[8 * job + lane];   // the input's bits
                if (lane == 0) {
                    A.n_in[job] = 0;
                    dbg->iterations[1] = dbg->trials[1] = dbg->max_trials[1] = 0;
                }
                return;
            }
        }
    }
    // e12->computeError(); e21->computeError(); on every kept pair at the final estimate
    const Sim3d Sinv = sim3_inverse(S);
    int n_in = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n && A.status[e0 + i] == 1) {
            const size_t e = e0 + i;
            const OptSim3Pair p = os3_pair(A, e);
            double Y[3], Z[3], u, v;
            sim3_map(S, p.X2, Y);
            os3_project(model1, cam1, Y, u, v);
            const double r12[2] = {p.obs1[0] - u, p.obs1[1] - v};
            sim3_map(Sinv, p.X1, Z);
            os3_project(model2, cam2, Z, u, v);
            const double r21[2] = {p.obs2[0] - u, p.obs2[1] - v};
            const double c12 = r12[0] * (p.w1 * r12[0]) + r12[1] * (p.w1 * r12[1]);
            const double c21 = r21[0] * (p.w2 * r21[0]) + r21[1] * (p.w2 * r21[1]);
            A.c12[e] = c12, A.c21[e] = c21;
            in = !(c12 > th2 || c21 > th2);
            if (!in) A.status[e] = 3;
        }
        n_in += __popcll(__ballot(in));
    }
    if (lane == 0) {
        for (int k = 0; k < 4; ++k) A.S[8 * job + k] = S.q[k];
        for (int k = 0; k < 3; ++k) A.S[8 * job + 4 + k] = S.t[k];
        A.S[8 * job + 7] = S.s;
        A.n_in[job] = n_in;
    }
}

}  // namespace

struct omv_optsim3 {
    int max_jobs = 0, max_entries = 0, n_jobs = 0;
    std::vector<int> start;   // entry_start of the last call
    // one upload and one read-back per call, through pinned host blocks laid out like the device ones:
    //   in:  jobs [J] | S [J][8] | Xw1 [3], Xw2 [3], obs1 [2], w1, obs2 [2], w2 (12 floats per entry, planar) | has_kp2
    //   out: S [J][8] | n_in [J] | status [entries]
    char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
    float *d_f = nullptr;        // prepared: X1 [3], X2 [3], obs2 [2] (8 floats per entry, planar)
    double *d_d = nullptr;       // c12, c21, e0 [4] (6 doubles per entry, planar)
    OptSim3Debug *d_dbg = nullptr;
    omv::DeviceArena mem;   // owns the device and pinned blocks
};

namespace {
constexpr size_t kOs3InJob = sizeof(OptSim3Job) + 8 * sizeof(double), kOs3InEntry = 12 * sizeof(float) + 1;
constexpr size_t kOs3OutJob = 8 * sizeof(double) + sizeof(int32_t), kOs3OutEntry = 1;
static_assert(sizeof(OptSim3Job) % 8 == 0, "S follows the jobs in the upload block");
}  // namespace

extern "C" {

omv_status omv_optimize_sim3_create(int max_jobs, int max_entries_total, omv_optsim3 **out) {
    if (!out || max_jobs <= 0 || max_entries_total < 0) return OMV_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OMV_ERR_NO_DEVICE;
    auto h = std::make_unique<omv_optsim3>();
    h->max_jobs = max_jobs, h->max_entries = max_entries_total;
    const size_t ne = (size_t)std::max(1, max_entries_total);
    const size_t in_bytes = max_jobs * kOs3InJob + ne * kOs3InEntry;
    const size_t out_bytes = max_jobs * kOs3OutJob + ne * kOs3OutEntry;
    omv::DeviceArena &mem = h->mem;
    if (!mem.alloc(&h->d_in, in_bytes) || !mem.alloc(&h->d_out, out_bytes) || !mem.alloc_pinned(&h->h_in, in_bytes) ||
        !mem.alloc_pinned(&h->h_out, out_bytes) || !mem.alloc(&h->d_f, ne * 8) || !mem.alloc(&h->d_d, ne * 6) ||
        !mem.alloc(&h->d_dbg, max_jobs))
        return OMV_ERR_HIP;
    *out = h.release();
    return OMV_OK;
}

omv_status omv_optimize_sim3_destroy(omv_optsim3 *h) {
    if (!h) return OMV_ERR_ARG;
    delete h;
    return OMV_OK;
}

omv_status omv_optimize_sim3(omv_optsim3 *h, int n_jobs, const int32_t *entry_start, const float *Xw1, const float *Xw2,
                             const float *obs1, const float *inv_sigma2_1, const uint8_t *has_kp2, const float *obs2,
                             const float *inv_sigma2_2, const float *pose1, const float *pose2, const float *cam1,
                             const float *cam2, const int32_t *model1, const int32_t *model2, const int32_t *fix_scale,
                             const float *th2, double *q, double *t, double *s, int32_t *n_in, uint8_t *status,
                             void *stream) {
    if (!h || n_jobs < 0 || n_jobs > h->max_jobs) return OMV_ERR_ARG;
    if (n_jobs > 0 && (!entry_start || !pose1 || !pose2 || !cam1 || !cam2 || !model1 || !model2 || !fix_scale || !th2 ||
                       !q || !t || !s || !n_in))
        return OMV_ERR_ARG;
    if (n_jobs > 0 && entry_start[0] != 0) return OMV_ERR_ARG;
    for (int j = 0; j < n_jobs; j++) {
        if (entry_start[j + 1] < entry_start[j]) return OMV_ERR_ARG;
        if ((model1[j] != OMV_CAM_KB8 && model1[j] != OMV_CAM_PINHOLE) ||
            (model2[j] != OMV_CAM_KB8 && model2[j] != OMV_CAM_PINHOLE))
            return OMV_ERR_ARG;
    }
    const int ne = n_jobs ? entry_start[n_jobs] : 0;
    if (ne > h->max_entries) return OMV_ERR_ARG;
    if (ne > 0 && (!Xw1 || !Xw2 || !obs1 || !inv_sigma2_1 || !has_kp2 || !obs2 || !inv_sigma2_2 || !status))
        return OMV_ERR_ARG;
    h->n_jobs = n_jobs;
    h->start.assign(entry_start, entry_start + (n_jobs ? n_jobs + 1 : 0));
    if (n_jobs == 0) return OMV_OK;
    // the upload block, packed for this call's sizes
    const size_t J = (size_t)n_jobs, E = (size_t)ne;
    const size_t o_S = J * sizeof(OptSim3Job), o_f = o_S + J * 8 * sizeof(double), o_b = o_f + E * 12 * sizeof(float);
    const size_t in_bytes = o_b + E, o_n = J * 8 * sizeof(double), o_st = o_n + J * sizeof(int32_t), out_bytes = o_st + E;
    OptSim3Job *jobs = reinterpret_cast<OptSim3Job *>(h->h_in);
    double *S = reinterpret_cast<double *>(h->h_in + o_S);
    for (int j = 0; j < n_jobs; j++) {
        OptSim3Job &p = jobs[j];
        p.start = entry_start[j], p.n = entry_start[j + 1] - entry_start[j];
        p.model1 = model1[j], p.model2 = model2[j], p.fix_scale = fix_scale[j] != 0, p.th2 = th2[j];
        for (int k = 0; k < 12; k++) p.pose1[k] = pose1[12 * j + k], p.pose2[k] = pose2[12 * j + k];
        for (int k = 0; k < 8; k++) p.cam1[k] = cam1[8 * j + k], p.cam2[k] = cam2[8 * j + k];
        for (int k = 0; k < 4; k++) S[8 * j + k] = q[4 * j + k];
        for (int k = 0; k < 3; k++) S[8 * j + 4 + k] = t[3 * j + k];
        S[8 * j + 7] = s[j];
    }
    if (ne > 0) {
        float *f = reinterpret_cast<float *>(h->h_in + o_f);
        std::copy(Xw1, Xw1 + 3 * E, f), std::copy(Xw2, Xw2 + 3 * E, f + 3 * E), std::copy(obs1, obs1 + 2 * E, f + 6 * E);
        std::copy(inv_sigma2_1, inv_sigma2_1 + E, f + 8 * E), std::copy(obs2, obs2 + 2 * E, f + 9 * E);
        std::copy(inv_sigma2_2, inv_sigma2_2 + E, f + 11 * E);
        std::copy(has_kp2, has_kp2 + E, reinterpret_cast<uint8_t *>(h->h_in + o_b));
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t cap = (size_t)std::max(1, h->max_entries);
    HIP_OK(hipMemcpyAsync(h->d_in, h->h_in, in_bytes, hipMemcpyHostToDevice, st));
    OptSim3Args A;
    const float *f = reinterpret_cast<const float *>(h->d_in + o_f);
    A.jobs = reinterpret_cast<const OptSim3Job *>(h->d_in);
    A.S_in = reinterpret_cast<const double *>(h->d_in + o_S);
    A.Xw1 = f, A.Xw2 = f + 3 * E, A.obs1 = f + 6 * E, A.w1 = f + 8 * E, A.obs2_in = f + 9 * E, A.w2 = f + 11 * E;
    A.has_kp2 = reinterpret_cast<const uint8_t *>(h->d_in + o_b);
    A.X1 = h->d_f, A.X2 = h->d_f + 3 * cap, A.obs2 = h->d_f + 6 * cap;
    A.c12 = h->d_d, A.c21 = h->d_d + cap, A.e0 = h->d_d + 2 * cap;
    A.S = reinterpret_cast<double *>(h->d_out);
    A.n_in = reinterpret_cast<int32_t *>(h->d_out + o_n);
    A.status = reinterpret_cast<uint8_t *>(h->d_out + o_st);
    A.dbg = h->d_dbg;
    HIP_OK(hipMemsetAsync(h->d_dbg, 0, n_jobs * sizeof(OptSim3Debug), st));
    optimize_sim3_kernel<<<n_jobs, 64, 0, st>>>(A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h->h_out, h->d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const double *So = reinterpret_cast<const double *>(h->h_out);
    for (int j = 0; j < n_jobs; j++) {
        for (int k = 0; k < 4; k++) q[4 * j + k] = So[8 * j + k];
        for (int k = 0; k < 3; k++) t[3 * j + k] = So[8 * j + 4 + k];
        s[j] = So[8 * j + 7];
    }
    const int32_t *no = reinterpret_cast<const int32_t *>(h->h_out + o_n);
    std::copy(no, no + n_jobs, n_in);
    if (ne > 0) std::copy(h->h_out + o_st, h->h_out + o_st + E, reinterpret_cast<char *>(status));
    return OMV_OK;
}

omv_status omv_optimize_sim3_debug(omv_optsim3 *h, int job, double *H, double *b, double *chi2, double *lambda_init,
                                   double *x, double *e12, double *e21, int32_t *iterations, int32_t *trials,
                                   int32_t *max_trials, void *stream) {
    if (!h || job < 0 || job >= h->n_jobs) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    OptSim3Debug d;
    const int e0 = h->start[job], n = h->start[job + 1] - e0;
    std::vector<double> e(4 * (size_t)n);
    const size_t cap = (size_t)std::max(1, h->max_entries);
    HIP_OK(hipMemcpyAsync(&d, h->d_dbg + job, sizeof(d), hipMemcpyDeviceToHost, st));
    if (n > 0)
        HIP_OK(hipMemcpyAsync(e.data(), h->d_d + 2 * cap + 4 * (size_t)e0, e.size() * sizeof(double),
                              hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (H) std::copy(d.H, d.H + 49, H);
    if (b) std::copy(d.b, d.b + 7, b);
    if (chi2) *chi2 = d.chi2;
    if (lambda_init) *lambda_init = d.lambda_init;
    if (x) std::copy(d.x, d.x + 7, x);
    for (int i = 0; i < n; i++) {
        if (e12) e12[2 * i] = e[4 * i], e12[2 * i + 1] = e[4 * i + 1];
        if (e21) e21[2 * i] = e[4 * i + 2], e21[2 * i + 1] = e[4 * i + 3];
    }
    for (int r = 0; r < 2; r++) {
        if (iterations) iterations[r] = d.iterations[r];
        if (trials) trials[r] = d.trials[r];
        if (max_trials) max_trials[r] = d.max_trials[r];
    }
    return OMV_OK;
}

}  // extern "C"
