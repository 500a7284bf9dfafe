// MI355X-native pose graphs of loop closing and map merging: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:
// 1826-2119), its merge overload (:2121-2458) and Optimizer::OptimizeEssentialGraph4DoF (:6171-6480) as g2o's
// Levenberg-Marquardt on device-resident state, the third client of the block LDL^T solver (omv_ldlt.h) after
// LocalBundleAdjustment and FullInertialBA.
//
// Per LM iteration (the step control is omv_lm.h's, on the device: LmCtl):
//   linearise   1 wavefront / edge: g2o's numeric Jacobians (base_binary_edge.hpp:131-205) -- the central difference at
//               delta = 1e-9 of the restated error, one evaluation per lane (2 vertices x 7 or 4 columns x 2 signs, plus
//               the centre), a column formed by a lane-pair subtraction; then the edge's J^T Omega J blocks, J^T Omega e
//               vectors and chi2 into its own record
//   assemble    1 workgroup / stored 16x16 block: the host-planned list of edge contributions in edge order (no
//               floating-point atomics: a run repeats bit for bit); H is built once per iteration, as in g2o
//   per trial:  H + lambda on the variables' diagonal (pad rows: diagonal 1, zero right-hand side), the LDL^T solve,
//               oplus into the second state buffer + computeScale, the trial's chi2 in fixed-order partial sums, then
//               the accept / reject decision and the next step's gates
// Every launch is gated by the control block, so optimize() enqueues iterations x max_trials steps in stream order and
// waits once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/omv.h"
#include "essgraph_plan.h"
#include "g2o_types.h"
#include "omv_device.h"
#include "omv_ldlt_host.h"
#include "omv_lm.h"

namespace {

using namespace omv_g2o;
using namespace omv_essgraph_plan;
static_assert(sizeof(Int2) == sizeof(int2) && alignof(Int2) == alignof(int2), "the plan's records are the kernels' int2");
static_assert(sizeof(Int4) == sizeof(int4) && alignof(Int4) == alignof(int4), "the plan's records are the kernels' int4");

// Per kind: variables per vertex, error rows, doubles of a vertex's state, of a measurement, of a caller's vertex.
// 4DoF state: DR 9 | Rwb 9 | twb 3 | Rcw 9 | tcw 3 (ImuCamPose's members that VertexPose4DoF and Edge4DoF read; Rwb0
// is constant and lives beside the state); caller's vertex: Rcw 9 | tcw 3 | Rwb 9 | twb 3.
template <int K>
struct Kd {
    static constexpr int V = K == OMV_ESSGRAPH_SIM3 ? 7 : 4;
    static constexpr int D = K == OMV_ESSGRAPH_SIM3 ? 7 : 6;
    static constexpr int NS = K == OMV_ESSGRAPH_SIM3 ? 8 : 33;
    static constexpr int NM = K == OMV_ESSGRAPH_SIM3 ? 8 : 12;
    static constexpr int NC = K == OMV_ESSGRAPH_SIM3 ? 8 : 24;
    static constexpr int REC = 4 * V * V + 2 * V;   // an edge's record: H (2V x 2V, side-major) | b (2V)
};
constexpr int k4DR = 0, k4Rwb = 9, k4twb = 18, k4Rcw = 21, k4tcw = 30;
constexpr double kNumDelta = 1e-9;   // base_binary_edge.hpp:147

struct EssGraph {   // what the kernels read of the problem
    int n_v, n_e, n_opt, fix_scale;
    const int *ei, *ej, *et;
    const int *row_of;      // [n_v] first row of the vertex in the system, -1: fixed
    const int *opt_v;       // [n_opt]
    const double *Sa, *Sb;  // [n_v][8]
    double *meas;           // [n_e][NM]
    double *st[2];          // the push / pop double buffer
    const double *Rwb0;     // 4DoF: [n_v][9]
    double Rcb[9], tcb[3];  // 4DoF: the rig's Tcb (camera 0)
};

__device__ __forceinline__ Sim3d load_sim3(const double *p) {
    Sim3d s;
    for (int k = 0; k < 4; ++k) s.q[k] = p[k];
    for (int k = 0; k < 3; ++k) s.t[k] = p[4 + k];
    s.s = p[7];
    return s;
}
__device__ __forceinline__ void store_sim3(const Sim3d &s, double *p) {
    for (int k = 0; k < 4; ++k) p[k] = s.q[k];
    for (int k = 0; k < 3; ++k) p[4 + k] = s.t[k];
    p[7] = s.s;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 under _fix_scale -- in the caller's
// buffer, so the numeric Jacobian's step and computeScale's x see the zero too.
__device__ __forceinline__ Sim3d sim3_oplus(double *u, int fix_scale, const Sim3d &est) {
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), est);
}
// EdgeSim3::computeError (:106-114)
__device__ __forceinline__ void sim3_edge_error(const Sim3d &C, const Sim3d &Si, const Sim3d &Sj, double *e) {
    sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)), e);
}

// VertexPose4DoF::oplusImpl = ImuCamPose::UpdateW((0, 0, u0, u1, u2, u3)) (G2oTypes.h:147-157, G2oTypes.cc:237-267) of
// the 33-double state `in` into `out`: DR = Exp(ur) DR, Rwb = DR Rwb0, twb += ut; with `norm` (the fifth kept update)
// four entries of DR are zeroed and DR renormalised -- after Rwb was formed, which is not recomputed.
__device__ __forceinline__ void pose4_oplus(const EssGraph &G, const double *Rwb0, const double *u, bool norm, const double *in,
                                            double *out) {
    const double ur[3] = {0.0, 0.0, u[0]};
    double dR[9], DR[9], Rwb[9], Rbw[9], twb[3], tbw[3];
    exp_so3(ur, dR);
    mm3(dR, in + k4DR, DR);
    mm3(DR, Rwb0, Rwb);
    for (int q = 0; q < 3; ++q) twb[q] = in[k4twb + q] + u[1 + q];
    if (norm) {
        DR[2] = 0.0, DR[5] = 0.0, DR[6] = 0.0, DR[7] = 0.0;
        polar3(DR);
    }
    tr3(Rwb, Rbw);
    mv3(Rbw, twb, tbw);
    for (int q = 0; q < 3; ++q) tbw[q] = -tbw[q];
    mm3(G.Rcb, Rbw, out + k4Rcw);
    mv3(G.Rcb, tbw, out + k4tcw);
    for (int q = 0; q < 3; ++q) out[k4tcw + q] += G.tcb[q];
    for (int q = 0; q < 9; ++q) out[k4DR + q] = DR[q], out[k4Rwb + q] = Rwb[q];
    for (int q = 0; q < 3; ++q) out[k4twb + q] = twb[q];
}
// Edge4DoF::computeError (G2oTypes.h:763-771) from the two vertices' (Rcw, tcw) and the measurement [dRij | dtij]
__device__ __forceinline__ void pose4_edge_error(const double *m, const double *Ri, const double *ti, const double *Rj,
                                                 const double *tj, double *e) {
    double Rjt[9], A[9], dRt[9], B[9], v[3], w[3];
    tr3(Rj, Rjt);
    mm3(Ri, Rjt, A);
    tr3(m, dRt);
    mm3(A, dRt, B);
    log_so3(B, e);
    mv3(Rjt, tj, v);
    for (int q = 0; q < 3; ++q) v[q] = -v[q];
    mv3(Ri, v, w);
    for (int q = 0; q < 3; ++q) e[3 + q] = w[q] + ti[q] - m[9 + q];
}

// The error of edge e with vertex `side` (0 / 1; -1: neither) moved by oplus(u) on a copy.
template <int K>
__device__ __forceinline__ void edge_error(const EssGraph &G, const double *X, int e, int side, double *u, double *err) {
    const int i = G.ei[e], j = G.ej[e];
    const double *m = G.meas + (size_t)e * Kd<K>::NM;
    if constexpr (K == OMV_ESSGRAPH_SIM3) {
        Sim3d Si = load_sim3(X + 8 * (size_t)i), Sj = load_sim3(X + 8 * (size_t)j);
        if (side == 0) Si = sim3_oplus(u, G.fix_scale, Si);
        if (side == 1) Sj = sim3_oplus(u, G.fix_scale, Sj);
        sim3_edge_error(load_sim3(m), Si, Sj, err);
    } else {
        double moved[33];
        const double *pi = X + 33 * (size_t)i, *pj = X + 33 * (size_t)j;
        if (side == 0) pose4_oplus(G, G.Rwb0 + 9 * (size_t)i, u, false, pi, moved), pi = moved;
        if (side == 1) pose4_oplus(G, G.Rwb0 + 9 * (size_t)j, u, false, pj, moved), pj = moved;
        pose4_edge_error(m, pi + k4Rcw, pi + k4tcw, pj + k4Rcw, pj + k4tcw, err);
    }
}
// The information's diagonal: I7; diag(1e3, 1e3, 1, 1, 1, 1) -- the reference sets (0, 0) twice and never (2, 2)
// (Optimizer.cc:6241-6244).
template <int K>
__device__ __forceinline__ double info_diag(int r) {
    return K == OMV_ESSGRAPH_4DOF && r < 2 ? 1e3 : 1.0;
}
template <int K>
__device__ __forceinline__ double edge_chi2(const double *e) {   // _error.dot(information() * _error)
    double c = 0;
    for (int r = 0; r < Kd<K>::D; ++r) c += e[r] * (info_diag<K>(r) * e[r]);
    return c;
}

__device__ __forceinline__ int cur_buf(const LmCtl *c, int role) { return c ? ((c->cur ^ role) & 1) : role; }

// The measurements, composed in double at set_problem: EdgeSim3's C = S_table[j] S_table[i]^-1 (Optimizer.cc:1927,
// :1976 ...), Edge4DoF's rotation matrix and translation of S_table[i] S_table[j]^-1 (:6266-6270).
template <int K>
__global__ void __launch_bounds__(256) meas_kernel(EssGraph G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.n_e) return;
    const double *T = G.et[e] ? G.Sb : G.Sa;
    const Sim3d Si = load_sim3(T + 8 * (size_t)G.ei[e]), Sj = load_sim3(T + 8 * (size_t)G.ej[e]);
    double *m = G.meas + (size_t)e * Kd<K>::NM;
    if constexpr (K == OMV_ESSGRAPH_SIM3) {
        store_sim3(sim3_mul(Sj, sim3_inverse(Si)), m);
    } else {
        const Sim3d Sij = sim3_mul(Si, sim3_inverse(Sj));
        q_to_mat(Sij.q, m);
        for (int q = 0; q < 3; ++q) m[9 + q] = Sij.t[q];
    }
}

// linearizeOplus + constructQuadraticForm of every edge at the current state (buffer cur_buf(ctl, 0)), one wavefront per
// edge.  Lane l < 4V evaluates the error with vertex l / 2V moved by (+, -)[l & 1] delta along column (l % 2V) / 2; lane
// 4V the error itself.  A fixed vertex has no block: its lanes idle and its columns are zero.
template <int K>
__global__ void __launch_bounds__(256) lin_kernel(EssGraph G, const LmCtl *ctl, int gate, double *rec, double *chi2,
                                                  double *err_out, double *ji_out, double *jj_out) {
    constexpr int V = Kd<K>::V, D = Kd<K>::D, W2 = 2 * V, REC = Kd<K>::REC;
    __shared__ double sJ[4][D][W2], sE[4][D];
    if (!gate_open(ctl, gate)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave;
    if (e >= G.n_e) return;   // (wave-uniform; nothing below synchronises across wavefronts)
    const double *X = G.st[cur_buf(ctl, 0)];
    const bool fixed_i = G.row_of[G.ei[e]] < 0, fixed_j = G.row_of[G.ej[e]] < 0;
    const int side = lane / W2, col = (lane % W2) >> 1;
    const bool moved = lane < 2 * W2, centre = lane == 2 * W2;
    const bool work = centre || (moved && !(side ? fixed_j : fixed_i));
    double ev[D];
    for (int r = 0; r < D; ++r) ev[r] = 0.0;
    if (work) {
        double u[V];
        for (int q = 0; q < V; ++q) u[q] = 0.0;
        if (moved) {
            const double step = (lane & 1) ? -kNumDelta : kNumDelta;
            for (int q = 0; q < V; ++q) u[q] = q == col ? step : 0.0;
        }
        edge_error<K>(G, X, e, moved ? side : -1, u, ev);
    }
    const double scalar = 1.0 / (2 * kNumDelta);
    for (int r = 0; r < D; ++r) {
        const double other = __shfl_xor(ev[r], 1, 64);   // the (-) evaluation to the (+) lane
        if (moved && !(lane & 1)) sJ[wave][r][side * V + col] = work ? scalar * (ev[r] - other) : 0.0;
        if (centre) sE[wave][r] = ev[r];
    }
    wave_sync<0>();
    double *R = rec + (size_t)e * REC;
    // A^T Omega A, A^T Omega B, B^T Omega B (AtO = A^T Omega first, :77-89) on the lower triangle, mirrored: exactly symmetric
    for (int idx = lane; idx < W2 * W2; idx += 64) {
        const int a = idx / W2, c = idx % W2, hi = a > c ? a : c, lo = a > c ? c : a;
        double h = 0;
        for (int k = 0; k < D; ++k) h += (sJ[wave][k][hi] * info_diag<K>(k)) * sJ[wave][k][lo];
        R[idx] = h;
    }
    if (lane < W2) {   // b += J^T omega_r, omega_r = -Omega e (:74-78)
        double b = 0;
        for (int k = 0; k < D; ++k) b += sJ[wave][k][lane] * (-(info_diag<K>(k) * sE[wave][k]));
        R[W2 * W2 + lane] = b;
    }
    if (centre) {
        chi2[e] = edge_chi2<K>(ev);
        if (err_out)
            for (int r = 0; r < D; ++r) err_out[(size_t)e * D + r] = ev[r];
    }
    if (ji_out)
        for (int idx = lane; idx < D * V; idx += 64) {
            ji_out[(size_t)e * D * V + idx] = sJ[wave][idx / V][idx % V];
            jj_out[(size_t)e * D * V + idx] = sJ[wave][idx / V][V + idx % V];
        }
}

struct EssGather {   // the plan's contribution lists (EssPlan) on the device
    const int *cb_start;
    const int4 *cb;
    const int *cv_start;
    const int4 *cv;
    const uint8_t *real_row;
};

// One workgroup per stored block: its contributions in list order; on a diagonal block the pad rows' unit diagonal,
// the block's right-hand side and the largest |H(j, j)| of its variables (computeLambdaInit).
template <int K>
__global__ void __launch_bounds__(256) ess_assemble_kernel(EssGather A, BlockPat P, const double *rec, double *H, double *b,
                                                           double *diag_max, const LmCtl *ctl, int gate) {
    constexpr int V = Kd<K>::V, W2 = 2 * V, REC = Kd<K>::REC;
    __shared__ double dg[16];
    if (!gate_open(ctl, gate)) return;
    const int t = blockIdx.x, tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    const int kr = P.slot_kr[t], kc = P.slot_kc[t];
    const bool diag = kr == kc;
    double v = 0;
    for (int q = A.cb_start[t]; q < A.cb_start[t + 1]; ++q) {
        const int4 cq = A.cb[q];
        const int r0 = cq.w >> 4, c0 = cq.w & 15;
        if (r >= r0 && r < r0 + V && c >= c0 && c < c0 + V)
            v += rec[(size_t)cq.x * REC + (cq.y * V + r - r0) * W2 + cq.z * V + c - c0];
    }
    const bool real = A.real_row[16 * kr + r] != 0;
    if (diag && r == c && !real) v = 1.0;
    H[(size_t)t * 256 + sw16(r, c)] = v;
    if (!diag) return;
    if (r == c) dg[r] = real ? fabs(v) : 0.0;
    __syncthreads();
    if (tid < 16) {
        double bv = 0;
        for (int q = A.cv_start[kr]; q < A.cv_start[kr + 1]; ++q) {
            const int4 cq = A.cv[q];
            if (tid >= cq.z && tid < cq.z + V) bv += rec[(size_t)cq.x * REC + W2 * W2 + cq.y * V + tid - cq.z];
        }
        b[16 * kr + tid] = bv;
    }
    if (tid == 0) {
        double m = 0;
        for (int q = 0; q < 16; ++q) m = fmax(m, dg[q]);
        diag_max[kr] = m;
    }
}

// Sum of n doubles in a fixed order: thread-strided partials, then the block's tree (the same routine sums the current
// state's chi2 and a trial's, so an accepted trial's chi2 is the next iteration's to the bit).
__device__ double fixed_sum(const double *v, int n, double *sh) {
    double s = 0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) s += v[q];
    const double t = block_reduce_sum(s, sh);
    __syncthreads();
    return t;
}

__device__ __forceinline__ void ess_set_gates(LmCtl *c) {
    c->g_active = !c->done;
    c->g_build = !c->done && c->need_build;
    c->g_errA = 0;
}

// optimize()'s start.  lambda_init > 0: setUserLambdaInit; otherwise computeLambdaInit at the first iteration.
__global__ void ess_ctl_reset_kernel(LmCtl *c, int opt_it, int max_trials, double lambda_init, int *any_fail) {
    c->errors_of_current = 1;
    c->cur = c->last = 0;
    c->need_build = 1;
    c->it = c->trials = c->its = 0;
    c->opt_it = opt_it, c->max_trials = max_trials, c->lambda_init = lambda_init;
    omv_lm::lm_begin_iteration(c->lm, 0, 0.0, lambda_init);
    c->rho = 0, c->accepted = 0, c->n_acc = 0;
    c->done = opt_it <= 0;
    c->init_pending = 1;
    c->err0 = c->errors_chi = c->cur_chi = 0;
    *any_fail = 0;
    ess_set_gates(c);
}

// The start of solve(iteration) (optimization_algorithm_levenberg.cpp:82-101) after the iteration's linearisation:
// currentChi = activeChi2 of the current state, lambda_0 on iteration 0.  only_chi: optimize(0), the initial chi alone.
__global__ void __launch_bounds__(256) ess_begin_kernel(LmCtl *c, const double *chi2, int n_e, const double *diag_max, int nb,
                                                        int only_chi) {
    __shared__ double sh[8], mx[256];
    if (!only_chi && !c->g_build) return;
    const double chi = fixed_sum(chi2, n_e, sh);
    double m = 0;
    if (!only_chi)
        for (int q = threadIdx.x; q < nb; q += blockDim.x) m = fmax(m, diag_max[q]);
    mx[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int q = 1; q < 256; ++q) m = fmax(m, mx[q]);
    if (c->init_pending) c->err0 = c->errors_chi = chi, c->init_pending = 0;
    c->cur_chi = chi;
    if (only_chi) return;
    ++c->its;
    omv_lm::lm_begin_iteration(c->lm, c->it, chi, omv_lm::lm_lambda_init(c->lambda_init, m));
}

// The trial's matrix: H with lambda on the variables' diagonal (entry (r, r) of a block sits at 16 r).
__global__ void __launch_bounds__(256) ess_damp_kernel(EssGather A, BlockPat P, const double *H, double *S, double lambda,
                                                       const LmCtl *ctl) {
    if (!gate_open(ctl, kGateTrial)) return;
    if (ctl) lambda = ctl->lm.lambda;
    const int t = blockIdx.x, q = threadIdx.x;
    double v = H[(size_t)t * 256 + q];
    if ((q & 15) == 0 && P.slot_kr[t] == P.slot_kc[t] && A.real_row[16 * P.slot_kr[t] + (q >> 4)]) v += lambda;
    S[(size_t)t * 256 + q] = v;
}

// update(x) into the trial buffer and this vertex's term of computeScale, sum x_j (lambda x_j + b_j) over its rows.
template <int K>
__global__ void __launch_bounds__(64) ess_oplus_kernel(EssGraph G, const LmCtl *ctl, const double *x, const double *b,
                                                       double *scale_part) {
    constexpr int V = Kd<K>::V, NS = Kd<K>::NS;
    if (!gate_open(ctl, kGateTrial)) return;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= G.n_opt) return;
    const int v = G.opt_v[o], row = G.row_of[v];
    const double *in = G.st[cur_buf(ctl, 0)] + (size_t)v * NS;
    double *out = G.st[cur_buf(ctl, 1)] + (size_t)v * NS;
    double u[V];
    for (int q = 0; q < V; ++q) u[q] = x[row + q];
    if constexpr (K == OMV_ESSGRAPH_SIM3) {
        store_sim3(sim3_oplus(u, G.fix_scale, load_sim3(in)), out);
    } else {
        pose4_oplus(G, G.Rwb0 + 9 * (size_t)v, u, ctl->n_acc % 5 == 4, in, out);
    }
    const double lambda = ctl->lm.lambda;
    double s = 0;
    for (int q = 0; q < V; ++q) s += u[q] * (lambda * u[q] + b[row + q]);
    scale_part[o] = s;
}

// computeActiveErrors of the trial state: chi2 per edge.
template <int K>
__global__ void __launch_bounds__(64) ess_err_kernel(EssGraph G, const LmCtl *ctl, double *chi2) {
    if (!gate_open(ctl, kGateTrial)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.n_e) return;
    double ev[Kd<K>::D], u[Kd<K>::V];
    edge_error<K>(G, G.st[cur_buf(ctl, 1)], e, -1, u, ev);
    chi2[e] = edge_chi2<K>(ev);
}

// One trial's bookkeeping (omv_lm.h: lm_trial, lm_next) and the next step's gates.
__global__ void __launch_bounds__(256) ess_finish_kernel(LmCtl *c, const double *chi2_trial, int n_e, const double *scale_part,
                                                         int n_opt, const int *fail, int *any_fail) {
    __shared__ double sh[8];
    if (!c->g_active) return;
    const double chi = fixed_sum(chi2_trial, n_e, sh);
    const double ssum = fixed_sum(scale_part, n_opt, sh);
    if (threadIdx.x != 0) return;
    const int trial_buf = c->cur ^ 1;
    c->last = trial_buf;
    const bool ok = *fail == 0;
    if (!ok) *any_fail = 1;
    c->errors_chi = chi;
    c->errors_of_current = 0;
    const omv_lm::LmTrial tr = omv_lm::lm_trial(c->lm, chi, ok, ok ? ssum : 0.0);
    c->rho = tr.rho;
    ++c->trials;
    c->accepted = tr.accepted ? 1 : 0;
    if (tr.accepted) {
        ++c->n_acc;
        c->errors_of_current = 1;
        c->cur = trial_buf, c->cur_chi = chi;
    }
    const omv_lm::LmNext next = omv_lm::lm_next(c->lm, tr.rho, c->max_trials);
    c->need_build = next != omv_lm::kLmTrial;
    if (c->need_build) {
        if (next == omv_lm::kLmStop) c->done = 1;
        if (++c->it >= c->opt_it) c->done = 1;
    }
    ess_set_gates(c);
}

// optimize()'s end: the current state into buffer 0 when the last accepted trial left it in buffer 1, and into the
// staging block in the caller's layout.
template <int K>
__global__ void __launch_bounds__(256) ess_settle_kernel(EssGraph G, const LmCtl *ctl, double *stage) {
    constexpr int NS = Kd<K>::NS, NC = Kd<K>::NC;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.n_v) return;
    const int cur = cur_buf(ctl, 0);
    const double *s = G.st[cur] + (size_t)v * NS;
    double *o = stage + (size_t)v * NC;
    if constexpr (K == OMV_ESSGRAPH_SIM3) {
        for (int q = 0; q < 8; ++q) o[q] = s[q];
    } else {
        for (int q = 0; q < 9; ++q) o[q] = s[k4Rcw + q], o[12 + q] = s[k4Rwb + q];
        for (int q = 0; q < 3; ++q) o[9 + q] = s[k4tcw + q], o[21 + q] = s[k4twb + q];
    }
    if (cur)
        for (int q = 0; q < NS; ++q) G.st[0][(size_t)v * NS + q] = s[q];
}
__global__ void ess_ctl_settle_kernel(LmCtl *c) { c->cur = 0; }

// Eigen's squaredNorm of four coefficients (x y z w) as its packet reduction adds them, then the division.
template <typename T>
__device__ __forceinline__ void quat_normalize(T *q) {
    const T n2 = (q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]);
    T n;
    if constexpr (sizeof(T) == 4) n = omv::sqrtf_cr(n2);
    else n = sqrt(n2);
    for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}
// The vertex's estimate as the g2o::Sim3 the epilogues read: the estimate, or Sim3(Rcw, tcw, 1.) (Optimizer.cc:6446).
template <int K>
__device__ __forceinline__ Sim3d vertex_sim3(const double *s) {
    if constexpr (K == OMV_ESSGRAPH_SIM3) {
        return load_sim3(s);
    } else {
        Sim3d r;
        os3_q_from_mat(s + k4Rcw, r.q);
        for (int q = 0; q < 3; ++q) r.t[q] = s[k4tcw + q];
        r.s = 1.0;
        return r;
    }
}
// The epilogue, elementwise: threads 0 .. n_v-1 the SE3f of SetPose, threads n_v .. the corrected map points.
template <int K>
__global__ void __launch_bounds__(256) ess_recover_kernel(EssGraph G, int mode, float *poses, int n_points, float *points,
                                                          const int *point_ref) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < G.n_v) {
        if (!poses) return;
        const Sim3d S = vertex_sim3<K>(G.st[0] + (size_t)t * Kd<K>::NS);
        float *o = poses + 7 * (size_t)t;
        if (mode == OMV_ESSGRAPH_RECOVER_LOOP) {   // SE3f(rotation().cast<float>(), translation().cast<float>() / s)
            float q[4] = {(float)S.q[0], (float)S.q[1], (float)S.q[2], (float)S.q[3]};
            quat_normalize(q);
            for (int k = 0; k < 4; ++k) o[k] = q[k];
            for (int k = 0; k < 3; ++k) o[4 + k] = (float)S.t[k] / (float)S.s;
        } else {   // SE3d(rotation(), translation() / s).cast<float>(); 4DoF: s = 1, no division
            double q[4] = {S.q[0], S.q[1], S.q[2], S.q[3]};
            quat_normalize(q);
            for (int k = 0; k < 4; ++k) o[k] = (float)q[k];
            for (int k = 0; k < 3; ++k) o[4 + k] = (float)(mode == OMV_ESSGRAPH_RECOVER_MERGE ? S.t[k] / S.s : S.t[k]);
        }
        return;
    }
    const int p = t - G.n_v;
    if (p >= n_points) return;
    const int r = point_ref[p];
    if (r < 0) return;
    const Sim3d Srw = load_sim3(G.Sa + 8 * (size_t)r);
    const Sim3d Swr = sim3_inverse(vertex_sim3<K>(G.st[0] + (size_t)r * Kd<K>::NS));
    const double P[3] = {(double)points[3 * (size_t)p], (double)points[3 * (size_t)p + 1], (double)points[3 * (size_t)p + 2]};
    double Pr[3], Pw[3];
    sim3_map(Srw, P, Pr);
    sim3_map(Swr, Pr, Pw);
    for (int k = 0; k < 3; ++k) points[3 * (size_t)p + k] = (float)Pw[k];
}

}  // namespace

struct omv_essgraph {
    int kind = 0, max_vertices = 0, max_edges = 0;
    omv::DeviceArena mem;    // the handle's own blocks: d_ctl, h_ctl
    omv::DeviceArena prob;   // the current problem's device buffers and the pinned staging block
    LmCtl *d_ctl = nullptr, *h_ctl = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    bool lds_ok = false;
    double last_ms = 0;
    // the problem
    bool has = false;
    EssPlan plan;
    EssGraph G{};
    EssGather A{};
    LdltSolver ldlt{};   // the uploaded pattern (ldlt.pat) and the solver's launch on it
    double *d_init = nullptr;    // the uploaded state (reset)
    double *d_rec = nullptr, *d_chi2 = nullptr, *d_chi2_trial = nullptr, *d_H = nullptr, *d_S = nullptr, *d_b = nullptr;
    double *d_zero = nullptr, *d_x = nullptr, *d_scratch = nullptr, *d_diag = nullptr, *d_scale = nullptr;
    double *d_stage = nullptr, *h_stage = nullptr;
    int *d_fail = nullptr, *d_any_fail = nullptr, *h_any_fail = nullptr;
    ~omv_essgraph() {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

void free_problem(omv_essgraph *h) {
    h->prob.reset();
    h->has = false;
    h->plan = EssPlan{};
    h->G = EssGraph{}, h->A = EssGather{}, h->ldlt = LdltSolver{};
}

size_t state_doubles(const omv_essgraph *h) { return (size_t)h->G.n_v * (h->kind == OMV_ESSGRAPH_SIM3 ? 8 : 33); }
size_t caller_doubles(const omv_essgraph *h) { return (size_t)h->G.n_v * (h->kind == OMV_ESSGRAPH_SIM3 ? 8 : 24); }

// The device side of set_problem: the checked plan and the caller's arrays into the problem arena.
omv_status upload_problem(omv_essgraph *h, const omv_essgraph_problem *p) {
    const EssPlan &pl = h->plan;
    const LbaPlan &L = pl.L;
    const int n_v = pl.n_v, n_e = pl.n_e, nb = L.nb, nred = L.n_red, n_slots = L.n_slots;
    const bool sim3 = h->kind == OMV_ESSGRAPH_SIM3;
    omv::Uploader up{h->prob};
    EssGraph &G = h->G;
    G.n_v = n_v, G.n_e = n_e, G.n_opt = pl.n_opt, G.fix_scale = sim3 && p->fix_scale ? 1 : 0;
    std::vector<double> init, rwb0;
    if (sim3) {
        init.assign(p->vertices, p->vertices + 8 * (size_t)n_v);
    } else {   // ImuCamPose's posegraph members: Rwb0 = Rwb, DR = I (G2oTypes.cc:137-139, :163-165)
        init.assign(33 * (size_t)n_v, 0.0), rwb0.resize(9 * (size_t)n_v);
        for (int v = 0; v < n_v; ++v) {
            const double *c = p->vertices + 24 * (size_t)v;
            double *s = init.data() + 33 * (size_t)v;
            s[k4DR] = s[k4DR + 4] = s[k4DR + 8] = 1.0;
            for (int q = 0; q < 9; ++q) s[k4Rcw + q] = c[q], s[k4Rwb + q] = rwb0[9 * (size_t)v + q] = c[12 + q];
            for (int q = 0; q < 3; ++q) s[k4tcw + q] = c[9 + q], s[k4twb + q] = c[21 + q];
        }
        for (int q = 0; q < 9; ++q) G.Rcb[q] = p->Rcb[q];
        for (int q = 0; q < 3; ++q) G.tcb[q] = p->tcb[q];
        G.Rwb0 = up.copy(rwb0);
    }
    G.st[0] = up.copy(init), G.st[1] = up.copy(init), h->d_init = up.copy(init);
    G.ei = up.copy(p->edge_i, (size_t)n_e), G.ej = up.copy(p->edge_j, (size_t)n_e);
    G.et = up.copy(p->edge_table, (size_t)n_e);
    G.row_of = up.copy(pl.row_of), G.opt_v = up.copy(pl.opt_v);
    G.Sa = up.copy(p->S_a, 8 * (size_t)n_v), G.Sb = up.copy(p->S_b, 8 * (size_t)n_v);
    up.buffer(&G.meas, (size_t)n_e * 12);
    h->A = EssGather{up.copy(pl.cb_start), (const int4 *)up.copy(pl.cb), up.copy(pl.cv_start), (const int4 *)up.copy(pl.cv),
                     up.copy(pl.real_row)};
    h->ldlt = LdltSolver::upload(L, up);
    if (!up.ok) return OMV_ERR_HIP;
    const size_t rec = sim3 ? Kd<0>::REC : Kd<1>::REC;
    up.buffer(&h->d_rec, (size_t)n_e * rec), up.buffer(&h->d_chi2, n_e), up.buffer(&h->d_chi2_trial, n_e);
    up.buffer(&h->d_H, (size_t)n_slots * 256), up.buffer(&h->d_S, (size_t)n_slots * 256), up.buffer(&h->d_b, nred);
    up.buffer(&h->d_zero, nred), up.buffer(&h->d_x, nred), up.buffer(&h->d_scratch, LdltSolver::scratch_doubles(L));
    up.buffer(&h->d_fail, 1), up.buffer(&h->d_any_fail, 1);
    up.buffer(&h->d_diag, nb), up.buffer(&h->d_scale, pl.n_opt), up.buffer(&h->d_stage, caller_doubles(h));
    if (!up.ok || !h->prob.alloc_pinned(&h->h_stage, caller_doubles(h)) || !h->prob.alloc_pinned(&h->h_any_fail, 1))
        return OMV_ERR_HIP;
    HIP_OK(hipMemset(h->d_zero, 0, nred * sizeof(double)));
    HIP_OK(hipMemset(h->d_fail, 0, sizeof(int)));
    if (n_e > 0) {
        if (sim3) meas_kernel<0><<<(n_e + 255) / 256, 256, 0, h->stream>>>(G);
        else meas_kernel<1><<<(n_e + 255) / 256, 256, 0, h->stream>>>(G);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(h->stream));
    return OMV_OK;
}

// The launches below pick the kind's instantiation.
#define ESS_KIND(h, call)                        \
    do {                                         \
        if ((h)->kind == OMV_ESSGRAPH_SIM3) {    \
            constexpr int K = OMV_ESSGRAPH_SIM3; \
            call;                                \
        } else {                                 \
            constexpr int K = OMV_ESSGRAPH_4DOF; \
            call;                                \
        }                                        \
    } while (0)

omv_status launch_linearise(omv_essgraph *h, const LmCtl *c, int gate, double *err, double *ji, double *jj) {
    const EssGraph &G = h->G;
    if (G.n_e > 0)
        ESS_KIND(h, (lin_kernel<K><<<(G.n_e + 3) / 4, 256, 0, h->stream>>>(G, c, gate, h->d_rec, h->d_chi2, err, ji, jj)));
    const BlockPat &BP = h->ldlt.pat;
    ESS_KIND(h, (ess_assemble_kernel<K><<<BP.n_slots, 256, 0, h->stream>>>(h->A, BP, h->d_rec, h->d_H, h->d_b, h->d_diag, c,
                                                                           gate)));
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

omv_status launch_solve(omv_essgraph *h, const LmCtl *c, double lambda) {
    ess_damp_kernel<<<h->ldlt.pat.n_slots, 256, 0, h->stream>>>(h->A, h->ldlt.pat, h->d_H, h->d_S, lambda, c);
    h->ldlt.launch(h->stream, h->d_S, h->d_b, h->d_zero, h->d_x, h->d_scratch, h->d_fail, c);
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

// One LM step: the iteration's linearisation when one starts (gated), then a trial.
omv_status launch_step(omv_essgraph *h) {
    LmCtl *c = h->d_ctl;
    const EssGraph &G = h->G;
    omv_status rs;
    if ((rs = launch_linearise(h, c, kGateBuild, nullptr, nullptr, nullptr)) != OMV_OK) return rs;
    ess_begin_kernel<<<1, 256, 0, h->stream>>>(c, h->d_chi2, G.n_e, h->d_diag, h->ldlt.pat.nb, 0);
    if ((rs = launch_solve(h, c, 0.0)) != OMV_OK) return rs;
    ESS_KIND(h, (ess_oplus_kernel<K><<<(G.n_opt + 63) / 64, 64, 0, h->stream>>>(G, c, h->d_x, h->d_b, h->d_scale)));
    if (G.n_e > 0) ESS_KIND(h, (ess_err_kernel<K><<<(G.n_e + 63) / 64, 64, 0, h->stream>>>(G, c, h->d_chi2_trial)));
    ess_finish_kernel<<<1, 256, 0, h->stream>>>(c, h->d_chi2_trial, G.n_e, h->d_scale, G.n_opt, h->d_fail, h->d_any_fail);
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

}  // namespace

extern "C" {

omv_status omv_essgraph_create(int kind, int max_vertices, int max_edges, omv_essgraph **out) {
    if (!out || (kind != OMV_ESSGRAPH_SIM3 && kind != OMV_ESSGRAPH_4DOF) || max_vertices < 1 || max_edges < 0)
        return OMV_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OMV_ERR_NO_DEVICE;
    auto h = std::make_unique<omv_essgraph>();
    h->kind = kind, h->max_vertices = max_vertices, h->max_edges = max_edges;
    HIP_OK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (auto &e : h->ev) HIP_OK(hipEventCreate(&e));
    if (!h->mem.alloc_pinned(&h->h_ctl, 1) || !h->mem.alloc(&h->d_ctl, 1)) return OMV_ERR_HIP;
    h->lds_ok = LdltSolver::opt_in_lds();
    *out = h.release();
    return OMV_OK;
}

omv_status omv_essgraph_destroy(omv_essgraph *h) {
    if (!h) return OMV_ERR_ARG;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return OMV_OK;
}

omv_status omv_essgraph_set_problem(omv_essgraph *h, const omv_essgraph_problem *p) {
    if (!h || !p || !p->vertices || !p->S_a || !p->S_b || (h->kind == OMV_ESSGRAPH_4DOF && (!p->Rcb || !p->tcb)))
        return OMV_ERR_ARG;
    EssPlan plan;
    const EssLimits lim{h->max_vertices, h->max_edges};
    if (plan_essgraph(h->kind, p->n_vertices, p->fixed, p->n_edges, p->edge_i, p->edge_j, p->edge_table, lim, h->lds_ok,
                      plan) != OMV_OK)
        return OMV_ERR_ARG;
    HIP_OK(hipStreamSynchronize(h->stream));
    free_problem(h);
    h->plan = std::move(plan);
    const omv_status rs = upload_problem(h, p);
    if (rs != OMV_OK) {
        free_problem(h);
        return rs;
    }
    h->has = true;
    return OMV_OK;
}

omv_status omv_essgraph_optimize(omv_essgraph *h, int iterations, int max_trials, omv_essgraph_result *r) {
    if (!h || !r || !h->has || max_trials < 1 || iterations < 0) return OMV_ERR_ARG;
    hipStream_t st = h->stream;
    const EssGraph &G = h->G;
    LmCtl *c = h->d_ctl;
    // setUserLambdaInit(1e-16) (Optimizer.cc:1846); the 4DoF graph leaves it to computeLambdaInit
    const double lambda_init = h->kind == OMV_ESSGRAPH_SIM3 ? 1e-16 : 0.0;
    HIP_OK(hipEventRecord(h->ev[0], st));
    ess_ctl_reset_kernel<<<1, 1, 0, st>>>(c, iterations, max_trials, lambda_init, h->d_any_fail);
    HIP_OK(hipGetLastError());
    omv_status rs;
    if (iterations == 0) {   // the initial chi alone
        if ((rs = launch_linearise(h, nullptr, kGateAlways, nullptr, nullptr, nullptr)) != OMV_OK) return rs;
        ess_begin_kernel<<<1, 256, 0, st>>>(c, h->d_chi2, G.n_e, h->d_diag, h->ldlt.pat.nb, 1);
        HIP_OK(hipGetLastError());
    }
    const long long steps = (long long)iterations * max_trials;
    for (long long s = 0; s < steps; ++s)
        if ((rs = launch_step(h)) != OMV_OK) return rs;
    ESS_KIND(h, (ess_settle_kernel<K><<<(G.n_v + 255) / 256, 256, 0, st>>>(G, c, h->d_stage)));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h->h_ctl, c, sizeof(LmCtl), hipMemcpyDeviceToHost, st));
    ess_ctl_settle_kernel<<<1, 1, 0, st>>>(c);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h->h_stage, h->d_stage, caller_doubles(h) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h->h_any_fail, h->d_any_fail, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(h->ev[1], st));
    HIP_OK(hipStreamSynchronize(st));   // the one wait
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms = ms;
    const LmCtl &hc = *h->h_ctl;
    r->err = hc.err0, r->err_end = hc.cur_chi, r->iterations = hc.its, r->trials = hc.trials;
    r->solver_failed = *h->h_any_fail, r->lambda = hc.lm.lambda;
    if (r->vertices) std::memcpy(r->vertices, h->h_stage, caller_doubles(h) * sizeof(double));
    return OMV_OK;
}

omv_status omv_essgraph_evaluate(omv_essgraph *h, double *err, double *jac_i, double *jac_j, double *meas, double *chi2) {
    if (!h || !h->has) return OMV_ERR_ARG;
    const bool sim3 = h->kind == OMV_ESSGRAPH_SIM3;
    const size_t E = (size_t)h->G.n_e, D = sim3 ? 7 : 6, V = sim3 ? 7 : 4, NM = sim3 ? 8 : 12;
    omv::DeviceArena ws;
    double *d_err = nullptr, *d_ji = nullptr, *d_jj = nullptr;
    if (!ws.alloc(&d_err, E * D) || !ws.alloc(&d_ji, E * D * V) || !ws.alloc(&d_jj, E * D * V)) return OMV_ERR_HIP;
    const omv_status rs = launch_linearise(h, nullptr, kGateAlways, d_err, d_ji, d_jj);
    if (rs != OMV_OK) return rs;
    HIP_OK(hipStreamSynchronize(h->stream));
    if (E == 0) return OMV_OK;
    if (err) HIP_OK(hipMemcpy(err, d_err, E * D * sizeof(double), hipMemcpyDeviceToHost));
    if (jac_i) HIP_OK(hipMemcpy(jac_i, d_ji, E * D * V * sizeof(double), hipMemcpyDeviceToHost));
    if (jac_j) HIP_OK(hipMemcpy(jac_j, d_jj, E * D * V * sizeof(double), hipMemcpyDeviceToHost));
    if (chi2) HIP_OK(hipMemcpy(chi2, h->d_chi2, E * sizeof(double), hipMemcpyDeviceToHost));
    if (meas) {
        std::vector<double> m(E * 12);
        HIP_OK(hipMemcpy(m.data(), h->G.meas, E * NM * sizeof(double), hipMemcpyDeviceToHost));
        std::memcpy(meas, m.data(), E * NM * sizeof(double));
    }
    return OMV_OK;
}

omv_status omv_essgraph_reset(omv_essgraph *h) {
    if (!h || !h->has) return OMV_ERR_ARG;
    HIP_OK(hipStreamSynchronize(h->stream));
    for (double *s : h->G.st) HIP_OK(hipMemcpy(s, h->d_init, state_doubles(h) * sizeof(double), hipMemcpyDeviceToDevice));
    return OMV_OK;
}

omv_status omv_essgraph_blocks(omv_essgraph *h, int *n_blocks, int *n_levels) {
    if (!h || !n_blocks || !n_levels) return OMV_ERR_ARG;
    *n_blocks = h->has ? h->ldlt.pat.nb : 0, *n_levels = h->has ? h->ldlt.pat.n_lev : 0;
    return OMV_OK;
}

omv_status omv_essgraph_debug_solve(omv_essgraph *h, double lambda, double *S, double *rhs, double *x, int32_t *fail,
                                    int32_t *plan, int plan_cap) {
    if (!h || !S || !rhs || !x || !fail || !plan || !(lambda > 0.0) || !std::isfinite(lambda) || !h->has) return OMV_ERR_ARG;
    if (plan_cap < 4 + h->ldlt.pat.n_lev) return OMV_ERR_ARG;
    omv_status rs;
    if ((rs = launch_linearise(h, nullptr, kGateAlways, nullptr, nullptr, nullptr)) != OMV_OK) return rs;
    if ((rs = launch_solve(h, nullptr, lambda)) != OMV_OK) return rs;
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipMemcpy(rhs, h->d_b, 16 * (size_t)h->ldlt.pat.nb * sizeof(double), hipMemcpyDeviceToHost));
    return h->ldlt.read_solved(h->plan.L, h->d_S, h->d_x, h->d_fail, S, x, fail, plan);
}

omv_status omv_essgraph_recover(omv_essgraph *h, int mode, float *poses, int n_points, float *points,
                                const int32_t *point_ref) {
    if (!h || !h->has || n_points < 0 || (n_points > 0 && (!points || !point_ref))) return OMV_ERR_ARG;
    const bool sim3 = h->kind == OMV_ESSGRAPH_SIM3;
    if (sim3 ? (mode != OMV_ESSGRAPH_RECOVER_LOOP && mode != OMV_ESSGRAPH_RECOVER_MERGE) : mode != OMV_ESSGRAPH_RECOVER_4DOF)
        return OMV_ERR_ARG;
    const int n_v = h->G.n_v;
    for (int p = 0; p < n_points; ++p)
        if (point_ref[p] < -1 || point_ref[p] >= n_v) return OMV_ERR_ARG;
    omv::DeviceArena ws;
    float *d_poses = nullptr, *d_pts = nullptr;
    int *d_ref = nullptr;
    if ((poses && !ws.alloc(&d_poses, 7 * (size_t)n_v)) || !ws.alloc(&d_pts, 3 * (size_t)n_points) ||
        !ws.alloc(&d_ref, (size_t)n_points))
        return OMV_ERR_HIP;
    hipStream_t st = h->stream;
    if (n_points > 0) {
        HIP_OK(hipMemcpyAsync(d_pts, points, 3 * (size_t)n_points * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_ref, point_ref, (size_t)n_points * sizeof(int), hipMemcpyHostToDevice, st));
    }
    const int n = n_v + n_points;
    ESS_KIND(h, (ess_recover_kernel<K><<<(n + 255) / 256, 256, 0, st>>>(h->G, mode, d_poses, n_points, d_pts, d_ref)));
    HIP_OK(hipGetLastError());
    if (poses) HIP_OK(hipMemcpyAsync(poses, d_poses, 7 * (size_t)n_v * sizeof(float), hipMemcpyDeviceToHost, st));
    if (n_points > 0) HIP_OK(hipMemcpyAsync(points, d_pts, 3 * (size_t)n_points * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return OMV_OK;
}

omv_status omv_essgraph_set_comm(omv_essgraph *, int, int, omv_allreduce_fn, void *) { return OMV_ERR_ARG; }

omv_status omv_essgraph_last_ms(omv_essgraph *h, double *ms) {
    if (!h || !ms) return OMV_ERR_ARG;
    *ms = h->last_ms;
    return OMV_OK;
}

}  // extern "C"
