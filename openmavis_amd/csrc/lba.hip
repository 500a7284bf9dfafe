// MI355X-native LocalInertialBA inner loop (Optimizer::LocalInertialBA's optimize(),
// src/Optimizer.cc:3270-3321): g2o's Levenberg-Marquardt over EdgeMono / EdgeInertial / EdgeGyroRW /
// EdgeAccRW with the landmark Schur complement, as batched gfx950 kernels on device-resident state.
//
// Per LM iteration (g2o's Levenberg-Marquardt; its step control is omv_lm.h's):
//   errors   1 thread / visual edge (+1 thread / inertial edge): residual, chi2, Huber rho; deterministic
//            two-level chi2 reduction (computeActiveErrors + activeRobustChi2)
//   build    1 thread / landmark (edges sorted landmark-major): EdgeMono / EdgeStereo Jacobians, the
//            landmark's Hll / bl and per-keyframe Hpl blocks in registers; 1 workgroup / optimisable
//            keyframe gathers its edges for the pose-diagonal JpT W Jp and JpT W e (fixed-order reduction);
//            1 wavefront / inertial edge writes its 30x30 quadratic form (EdgeInertial + random walks),
//            added into the reduced system colour by colour (no two edges of a colour share a keyframe)
//   per trial (lambda):
//     schur    1 thread / landmark: Dinv = (Hll + lambda I)^-1, BD = Hpl Dinv and Hpl Dinv bl per slot;
//              1 workgroup / reduced-system block gathers its (slot a, slot b) terms BD_a Hpl_b^T and, on the
//              diagonal, the keyframe's coefficients — fixed-order sums throughout, no float atomics, so a
//              solve is bitwise identical run to run
//     ldlt     1 workgroup: block LDL^T of the reduced system (keyframe blocks of 15 / 6) on the
//              symbolic block pattern (host-computed fill-in), the nonzero blocks staged in LDS,
//              then block forward / backward substitution (SimplicialLDLT semantics: no pivoting,
//              failure on a zero or non-finite pivot)
//     update   1 thread / landmark: back-substitution xl = Dinv (bl - Hpl^T xp) and the point update;
//              1 thread / keyframe: ImuCamPose::Update (body-frame SE3 with ExpSO3) + v, bg, ba;
//              the step's computeScale term; errors of the trial state
//   The accept / reject decision (rho, lambda schedule, push/pop) runs on the device (finish_trial_kernel,
//   LmCtl) with one read-back per optimize(); a host-driven loop with the same decisions is kept for
//   sharded solves and parity checks.  Push/pop is a double-buffered state.
// The same solver has a visual kind (omv_vba: Optimizer::LocalBundleAdjustment's graph, SE3Quat keyframes, the
// EdgeSE3ProjectXYZ family): see Kind<V> below; only the kernels the pose parameterisation reaches are templates on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/omv.h"
#include "g2o_types.h"
#include "lba_plan.h"
#include "omv_device.h"
#include "omv_ldlt_host.h"
#include "omv_lm.h"

namespace {

using namespace omv_g2o;
using namespace omv_lba_plan;   // the group and LDS limits, LbaPlan / plan_lba (host-only: lba_plan.h)
static_assert(sizeof(Int2) == sizeof(int2) && alignof(Int2) == alignof(int2), "the plan's records are the kernels' int2");
static_assert(sizeof(Int4) == sizeof(int4) && alignof(Int4) == alignof(int4), "the plan's records are the kernels' int4");
static_assert(kPreintCov == PreView::C, "the plan reads the covariance where the kernels do");

// The device LM control block (LmCtl), its gates and the solver it gates: omv_ldlt.h.
__device__ __forceinline__ double lm_lambda(const LmCtl *c, double lambda) { return c ? c->lm.lambda : lambda; }

struct ErrBufs {   // per-edge errors of one state: visual [2E], stereo row [E], chi2 [E], inertial [19 NI]
    double *err, *err3, *chi2, *err9;
};
// Buffer of a role (0 = current, 1 = trial): by the control block's `cur` on the device driver, the role itself
// without one (the host driver passes the state it means as the first of the pair).
__device__ __forceinline__ int role_buf(const LmCtl *c, int role) { return c ? ((c->cur ^ role) & 1) : role; }

// EdgeMono / EdgeStereo error of edge e at point X (G2oTypes.h:293-299, :364-402): residual, chi2 into the error
// buffers; returns the robust chi2 (Huber rho_0) for activeRobustChi2.
__device__ __forceinline__ double mono_err_edge(const Rig &rig, const double *R, const double *t, const Edges &E, int e,
                                                const double *X, double delta, double dsqr, double delta_st,
                                                double dsqr_st, double *err, double *err3, double *chi2) {
    const int c = E.cam[e];
    double Xc[3];
    mv3(R, X, Xc);
    Xc[0] += t[0], Xc[1] += t[1], Xc[2] += t[2];
    double u, v;
    cam_project(rig, c, Xc, u, v);
    const double e0 = E.obs[2 * e] - u, e1 = E.obs[2 * e + 1] - v;
    const double w = (double)E.w[e];
    double c2 = e0 * w * e0 + e1 * w * e1;
    err[2 * e] = e0, err[2 * e + 1] = e1;
    const float ur = E.ur[e];
    if (ur >= 0.f) {   // EdgeStereo
        const double e2 = (double)ur - stereo_ur(u, rig.bf, Xc[2]);
        err3[e] = e2;
        c2 += e2 * w * e2;
    }
    chi2[e] = c2;
    double r0, r1;
    if (ur >= 0.f) huber(c2, delta_st, dsqr_st, r0, r1);
    else huber(c2, delta, dsqr, r0, r1);
    return r0;
}

// ---- the visual kind (omv_vba: Optimizer::LocalBundleAdjustment / BundleAdjustment) ---------------------------------
// The same solver on another parameterisation: the keyframe state is the SE3Quat Tcw of camera 0, q (x y z w) in the
// first four doubles of the keyframe's Rwb slot and t in its twb slot, updated by VertexSE3Expmap::oplusImpl; the rig's
// Rcb / tcb hold the constant camera c <- camera 0 transforms (mTrl / mTsll / mTsrl, identity for camera 0), and the
// per-camera Rcw / tcw are derived from (q, t) after every update as `mTrl * T` and toRotationMatrix do.  Kernels that
// depend on the parameterisation are templates on the kind; Kind<false> is empty, so the inertial instantiations are
// the code they were.
template <bool V>
struct Kind {};
template <>
struct Kind<true> {
    double qc0[kMaxCams][4];     // rotation of camera c <- camera 0 (its matrix is rig.Rcb[c], its translation rig.tcb[c])
    double fx, fy, cx, cy, bf;   // g2o::EdgeStereoSE3ProjectXYZ's own pinhole
    const double *huber;         // [2] device: Huber delta of the 2-row edges / the stereo edges; 0 = no kernel
    const uint8_t *level;        // [E] device order: 1 = the edge is excluded (setLevel(1) / initializeOptimization(0))
};

// Huber with delta > 0, the plain chi2 with delta == 0 (setRobustKernel(0))
__device__ __forceinline__ void huber0(double e2, double delta, double &r0, double &r1) {
    if (delta > 0) huber(e2, delta, delta * delta, r0, r1);
    else r0 = e2, r1 = 1.0;
}

// Camera c's pose of a keyframe from camera 0's (q, t): SE3Quat::operator* (se3quat.h:104-110) and toRotationMatrix.
__device__ __forceinline__ void vis_cam_pose(const Rig &rig, const Kind<true> &vis, int c, const double *q, const double *t,
                                             double Rc[9], double tc[3]) {
    if (c == 0) {   // the vertex's own camera: T itself
        q_to_mat(q, Rc);
        for (int i = 0; i < 3; ++i) tc[i] = t[i];
        return;
    }
    double qc[4], rt[3];
    q_rot(vis.qc0[c], t, rt);
    for (int i = 0; i < 3; ++i) tc[i] = rig.tcb[c][i] + rt[i];
    q_mul(vis.qc0[c], q, qc);
    q_normalize_pos(qc);
    q_to_mat(qc, Rc);
}

// computeError of EdgeSE3ProjectXYZ / ...ToBody (OptimizableTypes.h:142-148, :174-180: obs - pCamera->project) and of
// g2o::EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:190-197: invz and bf * invz are floats) where ur >= 0, at the
// edge camera's pose (R, t); residual and chi2 into the error buffers.  Returns the robust chi2; an excluded edge's
// chi2 is still written, and it adds nothing to activeRobustChi2.
__device__ __forceinline__ double vis_err_edge(const Rig &rig, const Kind<true> &vis, const double *R, const double *t,
                                               const Edges &E, int e, const double *X, double *err, double *err3,
                                               double *chi2) {
    double Xc[3];
    mv3(R, X, Xc);
    Xc[0] += t[0], Xc[1] += t[1], Xc[2] += t[2];
    const double w = (double)E.w[e];
    const float ur = E.ur[e];
    double e0, e1, c2;
    if (ur >= 0.f) {
        const float invz = (float)(1.0 / Xc[2]);
        const double u = Xc[0] * (double)invz * vis.fx + vis.cx, v = Xc[1] * (double)invz * vis.fy + vis.cy;
        const double e2 = (double)ur - (u - (double)((float)vis.bf * invz));
        e0 = E.obs[2 * e] - u, e1 = E.obs[2 * e + 1] - v;
        err3[e] = e2;
        c2 = e0 * w * e0 + e1 * w * e1 + e2 * w * e2;
    } else {
        double u, v;
        cam_project(rig, E.cam[e], Xc, u, v);
        e0 = E.obs[2 * e] - u, e1 = E.obs[2 * e + 1] - v;
        c2 = e0 * w * e0 + e1 * w * e1;
    }
    err[2 * e] = e0, err[2 * e + 1] = e1;
    chi2[e] = c2;
    double r0, r1;
    huber0(c2, vis.huber[ur >= 0.f ? 1 : 0], r0, r1);
    return vis.level[e] ? 0.0 : r0;
}

// linearizeOplus of the five edges at the current errors, in the reference's own form: JX = _jacobianOplusXi (nr x 3),
// JP = _jacobianOplusXj (nr x 6, (omega, upsilon) order), w and om as edge_jacobians.
//   EdgeSE3ProjectXYZ (OptimizableTypes.cpp:202-221) and the three ToBody edges (:252-371): -projectJac(X_c) R_cw and
//   -projectJac(X_c) R_c0 SE3deriv(X_l), X_l in camera 0 (R_c0 the identity there);
//   g2o::EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:228-274), entry by entry.
// An excluded edge has zero Jacobians and weights: it adds nothing to the system.
__device__ __forceinline__ int vis_edge_jacobians(const Rig &rig, const Kind<true> &vis, const State &s, const Edges &E,
                                                  int e, const double *err, const double *err3, const double *chi2,
                                                  double JX[9], double JP[18], double &w, double om[3]) {
    const bool st = E.ur[e] >= 0.f;
    if (vis.level[e]) {
#pragma unroll
        for (int q = 0; q < 9; ++q) JX[q] = 0.0;
#pragma unroll
        for (int q = 0; q < 18; ++q) JP[q] = 0.0;
        w = 0.0, om[0] = om[1] = om[2] = 0.0;
        return st ? 3 : 2;
    }
    const int k = E.kf[e], c = E.cam[e], C = rig.n_cams;
    const double *R = s.Rcw + ((size_t)k * C + c) * 9, *t = s.tcw + ((size_t)k * C + c) * 3;
    const double *X = s.pts + (size_t)E.pt[e] * 3;
    double Xc[3];
    mv3(R, X, Xc);
    for (int q = 0; q < 3; ++q) Xc[q] += t[q];
    if (st) {
        const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z, fx = vis.fx, fy = vis.fy, bf = vis.bf;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            JX[q] = -fx * R[q] / z + fx * x * R[6 + q] / z_2;
            JX[3 + q] = -fy * R[3 + q] / z + fy * y * R[6 + q] / z_2;
            JX[6 + q] = JX[q] - bf * R[6 + q] / z_2;
        }
        JP[0] = x * y / z_2 * fx, JP[1] = -(1 + (x * x / z_2)) * fx, JP[2] = y / z * fx;
        JP[3] = -1. / z * fx, JP[4] = 0, JP[5] = x / z_2 * fx;
        JP[6] = (1 + y * y / z_2) * fy, JP[7] = -x * y / z_2 * fy, JP[8] = -x / z * fy;
        JP[9] = 0, JP[10] = -1. / z * fy, JP[11] = y / z_2 * fy;
        JP[12] = JP[0] - bf * y / z_2, JP[13] = JP[1] + bf * x / z_2, JP[14] = JP[2];
        JP[15] = JP[3], JP[16] = 0, JP[17] = JP[5] - bf / z_2;
    } else {
        const double *R0 = s.Rcw + (size_t)k * C * 9, *t0 = s.tcw + (size_t)k * C * 3;
        double Xl[3], pj[6], pr[6];
        mv3(R0, X, Xl);
        for (int q = 0; q < 3; ++q) Xl[q] += t0[q];
        cam_jac(rig, c, Xc, pj);
#pragma unroll
        for (int q = 0; q < 6; ++q) pj[q] = -pj[q];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                JX[3 * r + q] = pj[3 * r] * R[q] + pj[3 * r + 1] * R[3 + q] + pj[3 * r + 2] * R[6 + q];
                pr[3 * r + q] = pj[3 * r] * rig.Rcb[c][q] + pj[3 * r + 1] * rig.Rcb[c][3 + q] + pj[3 * r + 2] * rig.Rcb[c][6 + q];
            }
        const double x = Xl[0], y = Xl[1], z = Xl[2];
        const double se3[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                JP[6 * r + q] = pr[3 * r] * se3[q] + pr[3 * r + 1] * se3[6 + q] + pr[3 * r + 2] * se3[12 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) JX[6 + q] = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) JP[12 + q] = 0.0;
    }
    double r0, r1;
    huber0(chi2[e], vis.huber[st ? 1 : 0], r0, r1);
    const double wi = (double)E.w[e];
    w = wi * r1;
    om[0] = -wi * err[2 * e] * r1, om[1] = -wi * err[2 * e + 1] * r1;
    om[2] = st ? -wi * err3[e] * r1 : 0.0;
    return st ? 3 : 2;
}

// EdgeInertial i with its random-walk edges at state s: the errors and chi2 into err9; returns the robust chi2.
__device__ __forceinline__ double imu_err_edge(const State &s, const Imu &I, int i, double delta, double dsqr, double *err9) {
    double r0 = 0;
    double e[9];
    imu_error(s, I, i, e, err9 + (size_t)10 * I.n + 9 * (size_t)i);   // + the rotation error for buildSystem
    const double *W = I.info9 + (size_t)i * 81;
    double c2 = 0;
    for (int r = 0; r < 9; ++r) {
        double t = 0;
        for (int c = 0; c < 9; ++c) t += W[r * 9 + c] * e[c];
        c2 += e[r] * t;
    }
    for (int q = 0; q < 9; ++q) err9[9 * (size_t)i + q] = e[q];
    err9[(size_t)9 * I.n + i] = c2;   // chi2 after the errors
    if (I.robust[i]) {
        double r1;
        huber(c2, delta, dsqr, r0, r1);
    } else {
        r0 = c2;
    }
    const int k1 = I.kf1[i], k2 = I.kf2[i];
    double eg[3], ea[3];
    for (int q = 0; q < 3; ++q) eg[q] = s.bg[3 * k2 + q] - s.bg[3 * k1 + q], ea[q] = s.ba[3 * k2 + q] - s.ba[3 * k1 + q];
    double tg[3], ta[3];
    mv3(I.infoG + 9 * i, eg, tg);
    mv3(I.infoA + 9 * i, ea, ta);
    r0 += eg[0] * tg[0] + eg[1] * tg[1] + eg[2] * tg[2];
    r0 += ea[0] * ta[0] + ea[1] * ta[1] + ea[2] * ta[2];
    return r0;
}

// EdgeInertial + random-walk errors of the first kImuLead edges, one block, one edge per thread (threads >= I.n
// contribute 0 to the fixed-order sum).  A whole map has more edges than that: imu_err_rest_kernel takes the others.
constexpr int kImuLead = 256;
__device__ __forceinline__ void imu_err_block(double *sh, State s, Imu I, double delta, double dsqr, double *err9,
                                              double *partial) {
    const int i = threadIdx.x;
    double r0 = 0;
    if (i < I.n) r0 = imu_err_edge(s, I, i, delta, dsqr, err9);
    const double t = block_reduce_sum(r0, sh);
    if (threadIdx.x == 0) partial[0] = t;
}

// The inertial edges from kImuLead on, launched after err_kernel only for a problem that has any (err_kernel's block 0
// has written the state they are evaluated at): one block, thread t takes edges kImuLead + t, + blockDim.x, .. and
// adds their robust chi2 in that order, then the block's fixed-order sum onto the inertial partial.  A kernel of its
// own because the same loop inside err_kernel takes that kernel from 146 to 241 VGPRs for every window that never
// has such edges.  Gated and buffered like err_kernel.
__global__ void __launch_bounds__(256) imu_err_rest_kernel(State s0, State s1, Imu I, double delta, double dsqr, ErrBufs e0,
                                                           ErrBufs e1, double *imu_partial, const LmCtl *ctl, int gate,
                                                           int role) {
    __shared__ double sh[8];
    if (!gate_open(ctl, gate)) return;
    const int bi = role_buf(ctl, role);
    const State s = bi ? s1 : s0;
    const ErrBufs eb = bi ? e1 : e0;
    double acc = 0;
    for (int i = kImuLead + threadIdx.x; i < I.n; i += blockDim.x) acc += imu_err_edge(s, I, i, delta, dsqr, eb.err9);
    const double t = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0) imu_partial[0] += t;
}

// activeRobustChi2: inertial partial + visual partials in a fixed order (one block of 256).
__device__ __forceinline__ double sum_chi(const double *mono_partial, int n_mono_blocks, const double *imu_partial,
                                          double *sh) {
    double v = 0;
    for (int i = threadIdx.x; i < n_mono_blocks; i += blockDim.x) v += mono_partial[i];
    const double t = block_reduce_sum(v, sh);
    return imu_partial[0] + t;
}

// The next step's gates from the LM state: a trial runs unless the optimisation ended; it starts a new
// iteration (buildSystem) after an iteration ended, and first recomputes the current state's errors when the
// last computed errors were a rejected trial's.
__device__ __forceinline__ void set_gates(LmCtl *c) {
    c->g_active = !c->done;
    c->g_build = !c->done && c->need_build;
    c->g_errA = 0;   // the current errors stay in their buffer (double-buffered): never recomputed
}

// The LM state reset of optimize()'s start: iteration 0's, for the kernels that read lambda before the first step's
// bookkeeping; the initial chi comes with that step.
struct LmReset {
    LmCtl *c;   // null: no reset
    int opt_it, max_trials;
    double lambda_init;
};
__device__ __forceinline__ void ctl_reset(const LmReset &r) {
    LmCtl *c = r.c;
    c->errors_of_current = 1;
    c->cur = c->last = 0;
    c->need_build = 1;
    c->it = c->trials = c->its = 0;
    c->opt_it = r.opt_it, c->max_trials = r.max_trials, c->lambda_init = r.lambda_init;
    omv_lm::lm_begin_iteration(c->lm, 0, 0.0, r.lambda_init);
    c->rho = 0, c->accepted = 0, c->n_acc = 0;
    c->done = r.opt_it <= 0;
    set_gates(c);
}

// optimize()'s start: err = activeRobustChi2 of the initial state (Optimizer.cc:3273-3274), LM state reset
// (used when no step follows, opt_it <= 0; otherwise the initial error launch resets the control block and the
// first step's bookkeeping sums the initial chi -- one launch less per optimize()).
__global__ void __launch_bounds__(256) ctl_init_kernel(LmCtl *c, const double *mono_partial, int n_mono_blocks,
                                                       const double *imu_partial, int opt_it, int max_trials,
                                                       double lambda_init, const double *pre) {
    __shared__ double sh[8];
    const double chi = pre ? pre[1] : sum_chi(mono_partial, n_mono_blocks, imu_partial, sh);
    if (threadIdx.x == 0) {
        ctl_reset(LmReset{c, opt_it, max_trials, lambda_init});
        c->err0 = c->errors_chi = c->cur_chi = chi;
        c->init_pending = 0;
    }
}

// One step's LM bookkeeping (omv_lm.h), after the trial's errors:
//   a step that started an iteration: ++its, the iteration begins at activeRobustChi2 of the current state (kept with
//   its buffer: after a rejected trial the reference recomputes the same errors and gets the same sum);
//   the trial: an accepted trial's state becomes current; then what comes next, and the next step's gates.
__device__ void finish_trial_body(double *sh, LmCtl *c, const double *mono_partial, int n_mono_blocks,
                                  const double *imu_partial, const double *scale_partial, int n_scale, const int *fail,
                                  const double *pre, const double *mono_partial0, const double *imu_partial0) {
    if (!c->g_active) return;
    const bool initp = c->init_pending != 0;
    double chi, ssum, chi0 = 0;
    if (pre) {   // a sharded solve: [initial chi (first step), chi, computeScale] summed over the ranks
        chi0 = pre[0], chi = pre[1], ssum = pre[2];
    } else {
        if (initp) {   // optimize()'s initial errors (their own partial buffers)
            chi0 = sum_chi(mono_partial0, n_mono_blocks, imu_partial0, sh);
            __syncthreads();
        }
        chi = sum_chi(mono_partial, n_mono_blocks, imu_partial, sh);
        double sc = 0;
        for (int i = threadIdx.x; i < n_scale; i += blockDim.x) sc += scale_partial[i];
        __syncthreads();
        ssum = block_reduce_sum(sc, sh);
    }
    if (threadIdx.x != 0) return;
    if (initp) c->err0 = c->errors_chi = c->cur_chi = chi0, c->init_pending = 0;
    if (c->g_build) {   // iteration start: the current state's activeRobustChi2 (its errors are in buffer cur)
        ++c->its;
        omv_lm::lm_begin_iteration(c->lm, c->it, c->cur_chi, c->lambda_init);
    }
    const int trial_buf = c->cur ^ 1;
    c->last = trial_buf;
    const bool ok = *fail == 0;
    c->errors_chi = chi;
    c->errors_of_current = 0;   // the last computed errors belong to the trial state
    const omv_lm::LmTrial tr = omv_lm::lm_trial(c->lm, chi, ok, ok ? ssum : 0.0);   // a failed solve: no step, no scale
    c->rho = tr.rho;
    ++c->trials;
    c->accepted = tr.accepted ? 1 : 0;
    if (tr.accepted) {
        ++c->n_acc;
        c->errors_of_current = 1;
        c->cur = trial_buf, c->cur_chi = chi;   // the trial's buffers become current
    }
    const omv_lm::LmNext next = omv_lm::lm_next(c->lm, tr.rho, c->max_trials);
    c->need_build = next != omv_lm::kLmTrial;   // kLmTrial: another trial of this iteration
    if (c->need_build) {
        if (next == omv_lm::kLmStop) c->done = 1;
        if (++c->it >= c->opt_it) c->done = 1;
    }
    set_gates(c);
}

// The current state into buffer 0 at optimize()'s end, when the last accepted trial left it in buffer 1 (one
// contiguous copy of the state block; idempotent).
__global__ void cur_copy_kernel(const LmCtl *c, const double *B, double *A, size_t n) {
    if (!c->cur) return;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) A[q] = B[q];
}

// One LM step's bookkeeping after the trial's errors (one block of 256).
__global__ void __launch_bounds__(256) finish_trial_kernel(LmCtl *c, const double *mono_partial, int n_mono_blocks,
                                                           const double *imu_partial, const double *scale_partial,
                                                           int n_scale, const int *fail, const double *pre,
                                                           const double *mono_partial0, const double *imu_partial0) {
    __shared__ double sh[8];
    finish_trial_body(sh, c, mono_partial, n_mono_blocks, imu_partial, scale_partial, n_scale, fail, pre,
                      mono_partial0, imu_partial0);
}

// A sharded solve's per-rank scalars, all-reduced before the LM bookkeeping: out = [0 (unused), chi of the trial,
// this rank's computeScale terms] (ctl == nullptr: out[1] = chi of the errors just computed, optimize()'s initial
// err).  Gated like the trial.
__global__ void __launch_bounds__(256) trial_scalars_kernel(const LmCtl *c, const double *mono_partial, int n_mono_blocks,
                                                            const double *imu_partial, const double *scale_partial,
                                                            int n_scale, double *out, const double *mono_partial0,
                                                            const double *imu_partial0) {
    __shared__ double sh[8];
    if (c && !c->g_active) return;
    double chiA = 0;   // the initial chi while the first step's bookkeeping still has to take it
    if (c && c->init_pending) {
        chiA = sum_chi(mono_partial0, n_mono_blocks, imu_partial0, sh);
        __syncthreads();
    }
    const double chi = sum_chi(mono_partial, n_mono_blocks, imu_partial, sh);
    double sc = 0;
    if (c)
        for (int i = threadIdx.x; i < n_scale; i += blockDim.x) sc += scale_partial[i];
    __syncthreads();
    const double ssum = block_reduce_sum(sc, sh);
    if (threadIdx.x == 0) out[0] = chiA, out[1] = chi, out[2] = ssum;
}

// Final chi2 = imu partial + visual partials (fixed order); also finishes the computeScale sums.
__global__ void __launch_bounds__(256) finish_kernel(const double *mono_partial, int n_mono_blocks, const double *imu_partial,
                                                     const double *scale_partial, int n_scale, const int *fail,
                                                     double *out) {
    __shared__ double sh[8];
    double v = 0;
    for (int i = threadIdx.x; i < n_mono_blocks; i += blockDim.x) v += mono_partial[i];
    double t = block_reduce_sum(v, sh);
    double s = 0;
    for (int i = threadIdx.x; i < n_scale; i += blockDim.x) s += scale_partial[i];
    __syncthreads();
    const double st = block_reduce_sum(s, sh);
    if (threadIdx.x == 0) {
        out[0] = imu_partial[0] + t;   // activeRobustChi2
        out[1] = st;                   // computeScale
        out[2] = fail ? (double)*fail : 0.0;   // the linear solve of this trial failed
    }
}

// ---- build: landmark groups with the Schur complement on f64 MFMA ---------------------------------------
// buildSystem (block_solver.hpp:381-432) and the landmark Schur complement (:353-486) of one trial in one pass over the
// edges.  A landmark group is a run of whole landmarks (<= 256 edges, <= 128 landmarks, <= 128 slots, <= 32 distinct
// optimisable keyframes; a slot = one landmark's edges on one keyframe).  Per group, on one workgroup:
//   1. one thread per edge: EdgeMono / EdgeStereo Jacobians (JX 3x3, JP 3x6, the robust weight, -W e) into LDS;
//   2. one thread per landmark: Hll = sum w JX^T JX and bl = sum JX^T (-W e) in edge order, the Cholesky factor
//      R R^T = Hll + lambda I and y = R^-1 bl; beside it one thread per slot: Hpl_s = sum w JP^T JX over the slot's
//      edges (in order), then M_s = Hpl_s R^-T, so that Hpl Dinv Hpl^T = M M^T and Hpl Dinv bl = M y;
//   3. the group's share of the reduced system as ONE zero-routed product on v_mfma_f64_16x16x4f64: rows / columns are
//      the group's keyframes in elimination order, 8 per keyframe (6 pose rows, then a Schur right-hand-side column and
//      a gradient column), and the K dimension is [3 per landmark: M routed to its slots' rows, -M to the columns,
//      y to the rhs column] ++ [each residual row of each edge: JP to its keyframe's rows, w JP to the columns, -W e
//      to the gradient column] -- so one accumulation gives  sum JP^T W JP - sum Hpl Dinv Hpl^T  per keyframe pair, the
//      keyframe gradients and the Schur right-hand side, with the cross-landmark and cross-edge sums done by the
//      matrix core in its fixed order (no float atomics: bitwise identical run to run);
//   4. the group's blocks (keyframe pairs it co-observes) and per-keyframe [b | Schur rhs] rows into its own record;
//      assemble_kernel sums the records of a reduced-system block in group order.
// The per-landmark (R^-1, y, bl) and per-slot M_s stay for the back-substitution xl = R^-T (y - sum M_s^T xp_s).
// lambda enters through R, so the build runs every trial (a rejected trial rebuilds at the same linearisation point:
// the current state and its errors are untouched, so the Jacobians are the same numbers; g2o rebuilds only the Schur).
struct Land {
    const int *edge_start;   // [P+1]
    const int *slot_start;   // [P+1]
    const int *slot_kf;      // [nslots]
    const int *slot_edge;    // [nslots+1] first edge of each slot (slots are the keyframe runs of the landmark-major edges)
    const int16_t *slot_lkf; // [nslots] the slot keyframe's index in its group's keyframe list, -1 for a fixed keyframe
    double *lnd;             // [P][12]: R^-1 (lower: 00 10 11 20 21 22) | y = R^-1 bl | bl
    double *M;               // [nslots][18]: M_s = Hpl_s R^-T (6 x 3, row-major), optimisable slots only
    int n;
    const int *grp_pt;       // [n_grp+1] landmarks of each group
    const int *grp_w;        // [n_grp] optimisable keyframes of the group (w); -w - 1: a one-landmark group past the
                             //   LDS limits, built by the scalar path
    const int *grp_tp;       // [n_grp+1] the group's 16x16 output tiles (ti >= tj), as pairs in `tp`
    const uint8_t *tp;       // [2 per tile]
    const int *grp_blk;      // [n_grp] index in blkoff of the group's w(w+1)/2 keyframe pairs (a >= b)
    const int *blkoff;       //   the pair's record in `rec` (36 doubles), -1 if the group's landmarks do not co-observe it
    const int *grp_kf;       // [n_grp] index in rhsoff of the group's w keyframes
    const int *rhsoff;       //   the keyframe's record in `rec_rhs` (12 doubles: gradient 6 | Schur rhs 6)
    double *rec;             // per reduced-system block its groups' 6x6 records, contiguous in group order
    double *rec_rhs;         // per optimisable keyframe its groups' [gradient | Schur rhs] records, in group order
};

// Inertial work lists (host-built once per problem, ascending): per reduced-system block its inertial edges.
struct Gather {
    const int *blk_start;    // [n_slots+1] per reduced-system block: its run of group records in Land::rec
    const int *rhs_start;    // [nb+1] per optimisable keyframe: its run of [gradient | Schur rhs] in Land::rec_rhs
    const int4 *imu_blk;     // per block: inertial edges (edge, side of the block row, side of the column)
    const int *ib_start;     // [n_slots+1]
    const int2 *imu_vec;     // per keyframe: inertial edges (edge, side)
    const int *iv_start;     // [nb+1]
    const double *contrib;   // [n_imu][30 x 30 + 30] per-edge inertial quadratic forms
};

struct Red {   // reduced (non-marginalised) system: 16 rows per optimisable keyframe
    int n;
    const int *offP;   // per keyframe, -1 for fixed
    int n_kf;
};

// One visual edge at the current errors (EdgeMono, or EdgeStereo when ur >= 0): the point Jacobian JX (nr x 3),
// the pose Jacobian JP (nr x 6, ImuCamPose order), the robust weight w = invSigma2 * rho' and the weighted
// residual om = -invSigma2 * rho' * e (constructQuadraticForm, base_binary_edge.hpp:55-116).  Row 2 is zero on an
// EdgeMono.
__device__ __forceinline__ int edge_jacobians(const Rig &rig, const State &s, const Edges &E, int e, double delta,
                                              double dsqr, double delta_st, double dsqr_st, const double *err,
                                              const double *err3, const double *chi2, double JX[9], double JP[18],
                                              double &w, double om[3]) {
    const int k = E.kf[e], c = E.cam[e], C = rig.n_cams;
    const double *Rcw = s.Rcw + ((size_t)k * C + c) * 9, *tcw = s.tcw + ((size_t)k * C + c) * 3;
    const double *X = s.pts + (size_t)E.pt[e] * 3;
    double Xc[3], Xb[3];
    mv3(Rcw, X, Xc);
    for (int q = 0; q < 3; ++q) Xc[q] += tcw[q];
    mv3(rig.Rbc[c], Xc, Xb);
    for (int q = 0; q < 3; ++q) Xb[q] += rig.tbc[c][q];
    const bool st = E.ur[e] >= 0.f;   // EdgeStereo: proj_jac row 2 = row 0, (2,2) += bf / z^2
    double pj[9];
    cam_jac(rig, c, Xc, pj);
    const int nr = st ? 3 : 2;
    if (st) {
        const double inv_z2 = 1.0 / (Xc[2] * Xc[2]);
        pj[6] = pj[0], pj[7] = pj[1], pj[8] = pj[2] + rig.bf * inv_z2;
    } else {
        pj[6] = pj[7] = pj[8] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            JX[3 * r + q] = -(pj[3 * r] * Rcw[q] + pj[3 * r + 1] * Rcw[3 + q] + pj[3 * r + 2] * Rcw[6 + q]);
    {
        double pr[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                pr[3 * r + q] = pj[3 * r] * rig.Rcb[c][q] + pj[3 * r + 1] * rig.Rcb[c][3 + q] + pj[3 * r + 2] * rig.Rcb[c][6 + q];
        const double x = Xb[0], y = Xb[1], z = Xb[2];
        const double se3[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                JP[6 * r + q] = pr[3 * r] * se3[q] + pr[3 * r + 1] * se3[6 + q] + pr[3 * r + 2] * se3[12 + q];
    }
    double r0, r1;
    if (st) huber(chi2[e], delta_st, dsqr_st, r0, r1);
    else huber(chi2[e], delta, dsqr, r0, r1);
    const double wi = (double)E.w[e];
    w = wi * r1;
    om[0] = -wi * err[2 * e] * r1, om[1] = -wi * err[2 * e + 1] * r1;
    om[2] = st ? -wi * err3[e] * r1 : 0.0;
    return nr;
}

// The kind's edge Jacobians / edge error.
template <bool V>
__device__ __forceinline__ int kind_jacobians(const Rig &rig, const Kind<V> &kd, const State &s, const Edges &E, int e,
                                              double delta, double dsqr, double delta_st, double dsqr_st, const double *err,
                                              const double *err3, const double *chi2, double JX[9], double JP[18],
                                              double &w, double om[3]) {
    if constexpr (V) return vis_edge_jacobians(rig, kd, s, E, e, err, err3, chi2, JX, JP, w, om);
    else return edge_jacobians(rig, s, E, e, delta, dsqr, delta_st, dsqr_st, err, err3, chi2, JX, JP, w, om);
}
template <bool V>
__device__ __forceinline__ double kind_err_edge(const Rig &rig, const Kind<V> &kd, const double *R, const double *t,
                                                const Edges &E, int e, const double *X, double delta, double dsqr,
                                                double delta_st, double dsqr_st, double *err, double *err3, double *chi2) {
    if constexpr (V) return vis_err_edge(rig, kd, R, t, E, e, X, err, err3, chi2);
    else return mono_err_edge(rig, R, t, E, e, X, delta, dsqr, delta_st, dsqr_st, err, err3, chi2);
}

// sum over the residual rows r of A[r][ia] B[r][ib] (row-major, row strides lda / ldb): the EdgeStereo row last
// (zero on an EdgeMono, where the sum is the two-row sum exactly)
__device__ __forceinline__ double rows3(const double *A, int ia, int lda, const double *B, int ib, int ldb) {
    return A[ia] * B[ib] + A[lda + ia] * B[ldb + ib] + A[2 * lda + ia] * B[2 * ldb + ib];
}

// Cholesky factor of D = Hll + lambda I (lower, R R^T = D) inverted: Ri = R^-1 as (00 10 11 20 21 22); y = R^-1 bl.
// Then Dinv = R^-T R^-1, so Hpl Dinv Hpl^T = (Hpl R^-T)(Hpl R^-T)^T and Hpl Dinv bl = (Hpl R^-T) y.  A non-positive
// pivot (D not positive definite, e.g. lambda = 0 on a two-edge-free landmark) gives NaN and the trial's solve fails,
// as the explicit inverse's infinities did.
__device__ __forceinline__ void chol3_inv(const double *H, double lambda, const double *bl, double Ri[6], double y[3]) {
    const double d00 = H[0] + lambda, d10 = H[3], d11 = H[4] + lambda, d20 = H[6], d21 = H[7], d22 = H[8] + lambda;
    const double l00 = sqrt(d00), i00 = 1.0 / l00;
    const double l10 = d10 * i00, l20 = d20 * i00;
    const double l11 = sqrt(d11 - l10 * l10), i11 = 1.0 / l11;
    const double l21 = (d21 - l20 * l10) * i11;
    const double l22 = sqrt(d22 - l20 * l20 - l21 * l21), i22 = 1.0 / l22;
    const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
    Ri[0] = i00, Ri[1] = i10, Ri[2] = i11, Ri[3] = i20, Ri[4] = i21, Ri[5] = i22;
    y[0] = i00 * bl[0];
    y[1] = i10 * bl[0] + i11 * bl[1];
    y[2] = i20 * bl[0] + i21 * bl[1] + i22 * bl[2];
}
// M = Hpl R^-T (6 x 3): M[r][c] = sum_{q <= c} Hpl[r][q] Ri[c][q]
__device__ __forceinline__ void m_of(const double *Hpl, const double Ri[6], double M[18]) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double h0 = Hpl[3 * r], h1 = Hpl[3 * r + 1], h2 = Hpl[3 * r + 2];
        M[3 * r] = h0 * Ri[0];
        M[3 * r + 1] = h0 * Ri[1] + h1 * Ri[2];
        M[3 * r + 2] = h0 * Ri[3] + h1 * Ri[4] + h2 * Ri[5];
    }
}

// LDS of one landmark group (doubles, edge / slot / landmark-major rows): kLdsE (lba_plan.h) per edge JP | w | -W e
constexpr int kLdsX = 9 * kGrpEdges;      // per edge JX (3 x 3)
constexpr int kLdsL = 3 * kGrpLand + 27 * kGrpW;   // per landmark y (3); per landmark R^-1 (6), then per keyframe
                                                   //   the group's 27 diagonal terms
constexpr size_t kBuildLds = (size_t)(kLdsE + kLdsX + kLdsL) * 8 + kGrpLand * kGrpW;
static_assert(6 * kGrpLand <= 27 * kGrpW, "R^-1 rows fit under the diagonal terms");
static_assert(27 * kGrpSlots <= kLdsE, "the slots' diagonal terms fit the edge region");


template <bool V>
__device__ __forceinline__ void land_group(int g, double *sm, const Rig &rig, const Kind<V> &kd, const State &s, const Edges &E,
                                           const Land &L, double lambda, double delta, double dsqr, double delta_st,
                                           double dsqr_st, const double *err, const double *err3, const double *chi2) {
    double *SE = sm, *SX = sm + kLdsE, *SY = SX + kLdsX, *SR = SY + 3 * kGrpLand;
    uint8_t *map = (uint8_t *)(SY + kLdsL);
    const int tid = threadIdx.x;
#ifdef OMV_BUILD_PROFILE
    long long tp0 = wall_clock64(), tp1 = 0, tp2 = 0, tp3 = 0, tq[4] = {0, 0, 0, 0};
#define OMV_TQ(k) tq[k] = wall_clock64()
#else
#define OMV_TQ(k)
#endif
    const int p0 = L.grp_pt[g], p1 = L.grp_pt[g + 1], np = p1 - p0;
    const int e0 = L.edge_start[p0], ne = L.edge_start[p1] - e0;
    const int s0 = L.slot_start[p0], ns = L.slot_start[p1] - s0;
    const int w = L.grp_w[g], ntile = (w + 1) >> 1, kpad = (3 * np + 3) & ~3;
    for (int q = tid; q < np * kGrpW; q += blockDim.x) map[q] = 0xFF;
    // phase 1: one thread per edge: Jacobians, weight, -W e into LDS (edge-major rows)
    if (tid < ne) {
        double JX[9], JP[18], wt, om[3];
        kind_jacobians<V>(rig, kd, s, E, e0 + tid, delta, dsqr, delta_st, dsqr_st, err, err3, chi2, JX, JP, wt, om);
        double *o = SE + kSE * tid;
#pragma unroll
        for (int q = 0; q < 18; ++q) o[q] = JP[q];
        o[18] = wt;
#pragma unroll
        for (int q = 0; q < 3; ++q) o[19 + q] = om[q];
#pragma unroll
        for (int q = 0; q < 9; ++q) SX[9 * tid + q] = JX[q];
    }
    __syncthreads();
#ifdef OMV_BUILD_PROFILE
    tp1 = wall_clock64();
#endif
    // phase 2a: threads 0..127 one landmark each (Hll, bl in edge order; Cholesky), 128..255 one slot each (Hpl and the
    // slot's keyframe-diagonal terms: 21 of sum w JP^T JP and 6 of sum JP^T (-W e), in edge order)
    double Hpl[18], Ps[27];
    int my_slot = -1, my_pl = 0;
    if (tid < kGrpLand) {
        if (tid < np) {
            const int p = p0 + tid;
            double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
            for (int f = L.edge_start[p] - e0, f1 = L.edge_start[p + 1] - e0; f < f1; ++f) {
                double jx[9], om[3];
#pragma unroll
                for (int q = 0; q < 9; ++q) jx[q] = SX[9 * f + q];
#pragma unroll
                for (int q = 0; q < 3; ++q) om[q] = SE[kSE * f + 19 + q];
                const double wt = SE[kSE * f + 18];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    bl[r] += rows3(jx, r, 3, om, 0, 1);
#pragma unroll
                    for (int q = 0; q < 3; ++q) H[3 * r + q] += wt * rows3(jx, r, 3, jx, q, 3);
                }
            }
            double Ri[6], y[3];
            chol3_inv(H, lambda, bl, Ri, y);
#pragma unroll
            for (int q = 0; q < 6; ++q) SR[6 * tid + q] = Ri[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) SY[3 * tid + q] = y[q];
            double *o = L.lnd + (size_t)p * 12;
#pragma unroll
            for (int q = 0; q < 6; ++q) o[q] = Ri[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) o[6 + q] = y[q], o[9 + q] = bl[q];
            for (int sl = L.slot_start[p], s1 = L.slot_start[p + 1]; sl < s1; ++sl) {
                const int a = L.slot_lkf[sl];
                if (a >= 0) map[tid * kGrpW + a] = (uint8_t)(sl - s0);
            }
        }
    } else if (tid - kGrpLand < ns) {
        my_slot = s0 + tid - kGrpLand;
        if (L.slot_lkf[my_slot] >= 0) {
#pragma unroll
            for (int q = 0; q < 18; ++q) Hpl[q] = 0;
#pragma unroll
            for (int q = 0; q < 27; ++q) Ps[q] = 0;
            for (int f = L.slot_edge[my_slot] - e0, f1 = L.slot_edge[my_slot + 1] - e0; f < f1; ++f) {
                double jx[9], jp[18], om[3];
#pragma unroll
                for (int q = 0; q < 9; ++q) jx[q] = SX[9 * f + q];
#pragma unroll
                for (int q = 0; q < 18; ++q) jp[q] = SE[kSE * f + q];
#pragma unroll
                for (int q = 0; q < 3; ++q) om[q] = SE[kSE * f + 19 + q];
                const double wt = SE[kSE * f + 18];
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) Hpl[3 * r + q] += wt * rows3(jp, r, 6, jx, q, 3);
                int q = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) Ps[q++] += wt * rows3(jp, r, 6, jp, c, 6);
#pragma unroll
                for (int r = 0; r < 6; ++r) Ps[21 + r] += rows3(jp, r, 6, om, 0, 1);
            }
            my_pl = E.pt[L.slot_edge[my_slot]] - p0;   // the slot's landmark
        } else {
            my_slot = -1;
        }
    }
    __syncthreads();
    OMV_TQ(0);
    // phase 2b: M_s = Hpl_s R^-T (kept in registers for the panels); the slot's diagonal terms into LDS (slot-major)
    double M[18];
    if (my_slot >= 0) {
        double Ri[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) Ri[q] = SR[6 * my_pl + q];
        m_of(Hpl, Ri, M);
        double *o = L.M + (size_t)my_slot * 18;
#pragma unroll
        for (int q = 0; q < 18; ++q) o[q] = M[q];
        const int sl = tid - kGrpLand;
#pragma unroll
        for (int q = 0; q < 27; ++q) SE[27 * sl + q] = Ps[q];
    }
    __syncthreads();
    OMV_TQ(1);
    // phase 2c: the keyframe-diagonal terms of the group, per keyframe a the slots' terms in landmark order
    // (SR's R^-1 rows are dead: the sums take their place)
    double *SP = SR;
    for (int q = tid; q < w * 27; q += blockDim.x) {
        const int a = q / 27, e = q - 27 * a;
        double v = 0;
        int pl = 0;
        for (; pl + 4 <= np; pl += 4) {
            int sl[4];
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) sl[u] = map[(pl + u) * kGrpW + a];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = SE[27 * (sl[u] & 127) + e];
#pragma unroll
            for (int u = 0; u < 4; ++u) v += sl[u] != 0xFF ? x[u] : 0.0;
        }
        for (; pl < np; ++pl) {
            const int sl = map[pl * kGrpW + a];
            const double x = SE[27 * (sl & 127) + e];
            v += sl != 0xFF ? x : 0.0;
        }
        SP[q] = v;
    }
    __syncthreads();
    OMV_TQ(2);
    // phase 3a: the MFMA operand panels, one per 16-row tile (keyframes 2t, 2t + 1): panel t holds for K = 3 pl + c
    // the 16 values of rows 16 t .. 16 t + 15: M_{pl, a}[r][c] at row 8 a + r, y_pl[c] at row 8 a + 6 (where landmark pl
    // has a slot on keyframe a), zero elsewhere -- zero-filled, then scattered by the slot threads
    double *PN = SE;
    const int npan = ntile * kpad * 16;
    for (int q = tid; q < npan; q += blockDim.x) PN[q] = 0.0;
    __syncthreads();
    if (my_slot >= 0) {
        const int a = L.slot_lkf[my_slot];
        double *o = PN + ((size_t)(a >> 1) * kpad + 3 * my_pl) * 16 + 8 * (a & 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int r = 0; r < 6; ++r) o[16 * c + r] = M[3 * r + c];
            o[16 * c + 6] = SY[3 * my_pl + c];
        }
    }
    __syncthreads();
#ifdef OMV_BUILD_PROFILE
    tp2 = wall_clock64();
#endif
    // phase 3b: Out(tile ti, tj) = init + sum_K A[.][K] B[K][.] on v_mfma_f64_16x16x4f64, A = panel ti (pose rows only),
    // B = -panel tj on the pose columns, +panel tj on the Schur rhs column, 0 on the gradient column; a diagonal tile
    // starts from the keyframes' diagonal terms, so each block comes out as sum JP^T W JP - sum Hpl Dinv Hpl^T and the
    // gradient / Schur rhs columns as b / sum Hpl Dinv bl.  Operand loads are affine in the step: no dependent chains.
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, kk = lane >> 4;
    const int t0 = L.grp_tp[g], nt = L.grp_tp[g + 1] - t0;
    const int nsteps = kpad >> 2;
    const int *blkoff = L.blkoff + L.grp_blk[g], *rhsoff = L.rhsoff + L.grp_kf[g];
    for (int it = wave; it < nt; it += (int)(blockDim.x >> 6)) {
        const int ti = L.tp[2 * (t0 + it)], tj = L.tp[2 * (t0 + it) + 1];
        const int ar = li & 7, bc = li & 7;
        const double amask = ar < 6 ? 1.0 : 0.0, bsign = bc < 6 ? -1.0 : (bc == 6 ? 1.0 : 0.0);
        const int b_kf = 2 * tj + (li >> 3);
        v4d acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // rows 16 ti + kk + 4 j of column 16 tj + li
            const int R = 16 * ti + kk + 4 * j, a = R >> 3, r = R & 7;
            double v = 0;
            if (a == b_kf && a < w && r < 6) {
                if (bc < 6) v = SP[27 * a + (r >= bc ? r * (r + 1) / 2 + bc : bc * (bc + 1) / 2 + r)];
                else if (bc == 7) v = SP[27 * a + 21 + r];
            }
            acc[j] = v;
        }
        const double *pa = PN + (size_t)ti * kpad * 16 + 16 * kk + li, *pb = PN + (size_t)tj * kpad * 16 + 16 * kk + li;
        for (int st = 0; st < nsteps; st += 4) {
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = st + u < nsteps ? 64 * (st + u) : 0;
                av[u] = pa[o], bv[u] = pb[o];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double m = st + u < nsteps ? 1.0 : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u] * amask * m, bv[u] * bsign, acc, 0, 0, 0);
            }
        }
        // out: each block / keyframe row to its place in the block's (keyframe's) contiguous record run
        if (b_kf >= w) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = 16 * ti + kk + 4 * j, a = R >> 3, r = R & 7;
            if (r >= 6 || a >= w) continue;
            if (bc < 6) {
                if (a >= b_kf) {
                    const int o = blkoff[a * (a + 1) / 2 + b_kf];
                    if (o >= 0) L.rec[(size_t)o * 36 + 6 * r + bc] = acc[j];
                }
            } else if (a == b_kf) {
                L.rec_rhs[(size_t)rhsoff[a] * 12 + (bc == 7 ? 0 : 6) + r] = acc[j];
            }
        }
    }
#ifdef OMV_BUILD_PROFILE
    __syncthreads();
    tp3 = wall_clock64();
    if (tid == 0 && ((g & 63) == 0 || tp3 - tp0 > 2000))
        printf("build group %d: edges %d landmarks %d slots %d w %d tiles %d | ticks(100MHz) jac %lld land %lld (2a %lld 2b %lld 2c %lld 3a %lld) mfma %lld\n",
               g, ne, np, ns, w, nt, tp1 - tp0, tp2 - tp1, tq[0] - tp1, tq[1] - tq[0], tq[2] - tq[1], tp2 - tq[2], tp3 - tp2);
#endif
#undef OMV_TQ
}

// A one-landmark group past the LDS limits (> 256 edges, > 128 slots or > 32 optimisable keyframes): the same
// quantities by the scalar path.  Windows of 64 edges: per edge its 30 landmark terms and 27 pose terms in LDS,
// thread 0 walks them in edge order (Hll, bl, per slot Hpl and the pose terms), then one thread per slot forms M_s,
// one thread per keyframe pair the block.
constexpr int kBigWin = 64;
template <bool V>
__device__ __forceinline__ void land_group_big(int g, double *sm, const Rig &rig, const Kind<V> &kd, const State &s, const Edges &E,
                                            const Land &L, double lambda, double delta, double dsqr, double delta_st,
                                            double dsqr_st, const double *err, const double *err3, const double *chi2) {
    double *T = sm;                       // [57][kBigWin]
    double *SL = sm + kLdsE + kLdsX;      // R^-1 | y of the landmark
    int *inv = (int *)(sm + kLdsE);       // keyframe index -> slot (the JX region as ints)
    const int tid = threadIdx.x;
    const int p = L.grp_pt[g], w = -L.grp_w[g] - 1, nblk = w * (w + 1) / 2;
    const int e0 = L.edge_start[p], e1 = L.edge_start[p + 1];
    const int *blkoff = L.blkoff + L.grp_blk[g], *rhsoff = L.rhsoff + L.grp_kf[g];
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0}, Hp[18], P[27];
    int cur = -1;
    auto flush = [&]() {   // thread 0: the finished slot `cur`
        const int a = L.slot_lkf[cur];
        if (a < 0) return;
        double *o = L.M + (size_t)cur * 18;
        for (int q = 0; q < 18; ++q) o[q] = Hp[q];
        double *B = L.rec + (size_t)blkoff[a * (a + 1) / 2 + a] * 36;
        int q = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c <= r; ++c, ++q) B[6 * r + c] = B[6 * c + r] = P[q];
        for (int r = 0; r < 6; ++r) L.rec_rhs[(size_t)rhsoff[a] * 12 + r] = P[21 + r];
    };
    for (int base = e0; base < e1; base += kBigWin) {
        if (tid < kBigWin && base + tid < e1) {
            double JX[9], JP[18], wt, om[3];
            kind_jacobians<V>(rig, kd, s, E, base + tid, delta, dsqr, delta_st, dsqr_st, err, err3, chi2, JX, JP, wt, om);
            for (int r = 0; r < 3; ++r) {
                T[(9 + r) * kBigWin + tid] = rows3(JX, r, 3, om, 0, 1);
                for (int q = 0; q < 3; ++q) T[(3 * r + q) * kBigWin + tid] = wt * rows3(JX, r, 3, JX, q, 3);
            }
            for (int r = 0; r < 6; ++r)
                for (int q = 0; q < 3; ++q) T[(12 + 3 * r + q) * kBigWin + tid] = wt * rows3(JP, r, 6, JX, q, 3);
            int q = 0;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c <= r; ++c, ++q) T[(30 + q) * kBigWin + tid] = wt * rows3(JP, r, 6, JP, c, 6);
            for (int r = 0; r < 6; ++r) T[(51 + r) * kBigWin + tid] = rows3(JP, r, 6, om, 0, 1);
        }
        __syncthreads();
        if (tid == 0)
            for (int f = base; f < min(base + kBigWin, e1); ++f) {
                const int le = f - base;
                for (int q = 0; q < 3; ++q) bl[q] += T[(9 + q) * kBigWin + le];
                for (int q = 0; q < 9; ++q) H[q] += T[q * kBigWin + le];
                const int sl = E.slot[f];
                if (sl != cur) {
                    if (cur >= 0) flush();
                    for (int q = 0; q < 18; ++q) Hp[q] = 0;
                    for (int q = 0; q < 27; ++q) P[q] = 0;
                    cur = sl;
                }
                for (int q = 0; q < 18; ++q) Hp[q] += T[(12 + q) * kBigWin + le];
                for (int q = 0; q < 27; ++q) P[q] += T[(30 + q) * kBigWin + le];
            }
        __syncthreads();
    }
    if (tid == 0) {
        if (cur >= 0) flush();
        double Ri[6], y[3];
        chol3_inv(H, lambda, bl, Ri, y);
        double *o = L.lnd + (size_t)p * 12;
        for (int q = 0; q < 6; ++q) o[q] = Ri[q], SL[q] = Ri[q];
        for (int q = 0; q < 3; ++q) o[6 + q] = y[q], o[9 + q] = bl[q], SL[6 + q] = y[q];
    }
    for (int sl = L.slot_start[p] + tid; sl < L.slot_start[p + 1]; sl += blockDim.x)
        if (L.slot_lkf[sl] >= 0) inv[L.slot_lkf[sl]] = sl;
    __threadfence_block();
    __syncthreads();
    for (int sl = L.slot_start[p] + tid; sl < L.slot_start[p + 1]; sl += blockDim.x) {
        if (L.slot_lkf[sl] < 0) continue;
        double h[18], M[18], Ri[6];
        double *o = L.M + (size_t)sl * 18;
        for (int q = 0; q < 18; ++q) h[q] = o[q];
        for (int q = 0; q < 6; ++q) Ri[q] = SL[q];
        m_of(h, Ri, M);
        for (int q = 0; q < 18; ++q) o[q] = M[q];
    }
    __threadfence_block();
    __syncthreads();
    for (int q = tid; q < nblk; q += blockDim.x) {
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= q) ++a;
        const int b = q - a * (a + 1) / 2;
        const double *Ma = L.M + (size_t)inv[a] * 18, *Mb = L.M + (size_t)inv[b] * 18;
        double *B = L.rec + (size_t)blkoff[q] * 36;
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                const double t = Ma[3 * r] * Mb[3 * c] + Ma[3 * r + 1] * Mb[3 * c + 1] + Ma[3 * r + 2] * Mb[3 * c + 2];
                B[6 * r + c] = (a == b ? B[6 * r + c] : 0.0) - t;
            }
    }
    for (int a = tid; a < w; a += blockDim.x) {
        const double *Ma = L.M + (size_t)inv[a] * 18;
        for (int r = 0; r < 6; ++r)
            L.rec_rhs[(size_t)rhsoff[a] * 12 + 6 + r] = Ma[3 * r] * SL[6] + Ma[3 * r + 1] * SL[7] + Ma[3 * r + 2] * SL[8];
    }
}

// ---- build: inertial + random-walk edges, one wavefront each -------------------------------------

// Inertial + random-walk edges of one EdgeInertial i (one wavefront): the 30 x 30 quadratic form and 30 gradient
// over the edge's local variables [P1 V1 G1 A1 P2 V2 G2 A2] (EdgeInertial over the first 24, EdgeGyroRW on
// G1 / G2, EdgeAccRW on A1 / A2), written to its own slot; assemble_kernel adds the slots into the reduced system.
constexpr int kImuLoc = 30, kImuContrib = kImuLoc * kImuLoc + kImuLoc;
__device__ __forceinline__ void imu_contrib_block(int i, double *sm, State s, Imu I, double delta, double dsqr,
                                                  const double *err9, double *contrib) {
    double *J = sm, *WJ = sm + 216, *om = sm + 432;   // J (9 x 24), Omega' J (9 x 24), -Omega' e
    const int lane = threadIdx.x, nt = blockDim.x;
    for (int q = lane; q < 216; q += nt) J[q] = 0;
    __syncthreads();
    imu_jacobian_par(s, I, i, err9 + (size_t)10 * I.n + 9 * (size_t)i, err9 + 9 * (size_t)i, J, WJ);   // WJ: RJ scratch
    __syncthreads();
    const double *e = err9 + 9 * i;
    const double c2 = err9[(size_t)9 * I.n + i];
    double r0, r1 = 1.0;
    if (I.robust[i]) huber(c2, delta, dsqr, r0, r1);
    const double *W = I.info9 + (size_t)i * 81;
    for (int q = lane; q < 216; q += nt) {
        const int r = q / 24, c = q % 24;
        double t = 0;
        for (int k = 0; k < 9; ++k) t += W[r * 9 + k] * J[k * 24 + c];
        WJ[q] = t * r1;
    }
    if (lane < 9) {
        double t = 0;
        for (int k = 0; k < 9; ++k) t += W[lane * 9 + k] * e[k];
        om[lane] = -t * r1;
    }
    __syncthreads();
    const int k1 = I.kf1[i], k2 = I.kf2[i];
    double *Hc = contrib + (size_t)i * kImuContrib, *bc = Hc + kImuLoc * kImuLoc;
    const double *Ig = I.infoG + 9 * i, *Ia = I.infoA + 9 * i;
    for (int q = lane; q < kImuLoc * kImuLoc; q += nt) {
        const int a = q / kImuLoc, b = q % kImuLoc;
        double t = 0;
        if (a < 24 && b < 24)
            for (int k = 0; k < 9; ++k) t += J[k * 24 + a] * WJ[k * 24 + b];
        // random walks: H += J^T Info J with J1 = -I (G1 / A1), J2 = I (G2 / A2)
        const int ga = a >= 9 && a < 12 ? 0 : (a >= 24 && a < 27 ? 1 : -1), gb = b >= 9 && b < 12 ? 0 : (b >= 24 && b < 27 ? 1 : -1);
        const int aa = a >= 12 && a < 15 ? 0 : (a >= 27 ? 1 : -1), ab = b >= 12 && b < 15 ? 0 : (b >= 27 ? 1 : -1);
        if (ga >= 0 && gb >= 0) {
            const int r = a - (ga ? 24 : 9), c = b - (gb ? 24 : 9);
            t += (ga == gb ? 1.0 : -1.0) * Ig[3 * r + c];
        }
        if (aa >= 0 && ab >= 0) {
            const int r = a - (aa ? 27 : 12), c = b - (ab ? 27 : 12);
            t += (aa == ab ? 1.0 : -1.0) * Ia[3 * r + c];
        }
        Hc[q] = t;
    }
    if (lane < kImuLoc) {
        double t = 0;
        if (lane < 24)
            for (int k = 0; k < 9; ++k) t += J[k * 24 + lane] * om[k];
        // random walks: b -= J^T Info e, e = b2 - b1 (+ on the first keyframe's bias, - on the second's)
        int which = -1, r = 0;   // 0 gyro, 1 acc
        if (lane >= 9 && lane < 15) which = lane >= 12, r = lane - (lane >= 12 ? 12 : 9);
        else if (lane >= 24) which = lane >= 27, r = lane - (lane >= 27 ? 27 : 24);
        if (which >= 0) {
            const double *bv = which ? s.ba : s.bg, *Iw = which ? Ia : Ig;
            double ee[3];
            for (int q = 0; q < 3; ++q) ee[q] = bv[3 * k2 + q] - bv[3 * k1 + q];
            const double Oe = Iw[3 * r] * ee[0] + Iw[3 * r + 1] * ee[1] + Iw[3 * r + 2] * ee[2];
            t += lane < 24 ? Oe : -Oe;
        }
        bc[lane] = t;
    }
}

// The whole build in one launch: blocks [0, n_imu) the inertial edges' quadratic forms, blocks from n_imu_pad (n_imu
// rounded up to 8, so the landmark groups keep their XCD-aware order) the landmark groups.  Independent halves, side by
// side.  Dynamic LDS: kBuildLds.
template <bool V>
__global__ void __launch_bounds__(kGrpEdges) build_all_kernel(Rig rig, Kind<V> kd, State s0, State s1, Edges E, Land L, int n_grp,
                                                              Imu I, int n_imu, int n_imu_pad, double lambda,
                                                              double delta, double dsqr, double delta_st, double dsqr_st,
                                                              double delta_imu, double dsqr_imu, ErrBufs e0, ErrBufs e1,
                                                              double *contrib, const LmCtl *ctl) {
    extern __shared__ double sm[];
    if (!gate_open(ctl, kGateTrial)) return;
    lambda = lm_lambda(ctl, lambda);
    const int bi = role_buf(ctl, 0);   // the current state and its errors
    const State s = bi ? s1 : s0;
    const ErrBufs eb = bi ? e1 : e0;
    const int b = blockIdx.x;
    if (b < n_imu_pad) {
#ifdef OMV_BUILD_PROFILE
        const long long ti0 = wall_clock64();
#endif
        if (b < n_imu) imu_contrib_block(b, sm, s, I, delta_imu, dsqr_imu, eb.err9, contrib);
#ifdef OMV_BUILD_PROFILE
        __syncthreads();
        if (threadIdx.x == 0 && b == 0) printf("build imu block 0: ticks(100MHz) %lld\n", wall_clock64() - ti0);
#endif
        return;
    }
    const int bl = b - n_imu_pad, chunk = (n_grp + 7) >> 3;
    const int g = (bl & 7) * chunk + (bl >> 3);
    if (g >= n_grp) return;
    if (L.grp_w[g] < 0) return;   // build_big_kernel's
    land_group<V>(g, sm, rig, kd, s, E, L, lambda, delta, dsqr, delta_st, dsqr_st, eb.err, eb.err3, eb.chi2);
}

// The one-landmark groups past the LDS limits (rare: a landmark with > 256 edges, > 128 slots or > 32 optimisable
// keyframes), one workgroup each, launched only when the problem has any.
template <bool V>
__global__ void __launch_bounds__(kGrpEdges) build_big_kernel(Rig rig, Kind<V> kd, State s0, State s1, Edges E, Land L,
                                                              const int *big, int n_big, double lambda, double delta,
                                                              double dsqr, double delta_st, double dsqr_st, ErrBufs e0,
                                                              ErrBufs e1, const LmCtl *ctl) {
    extern __shared__ double sm[];
    if (!gate_open(ctl, kGateTrial) || (int)blockIdx.x >= n_big) return;
    lambda = lm_lambda(ctl, lambda);
    const int bi = role_buf(ctl, 0);
    const State s = bi ? s1 : s0;
    const ErrBufs eb = bi ? e1 : e0;
    land_group_big<V>(big[blockIdx.x], sm, rig, kd, s, E, L, lambda, delta, dsqr, delta_st, dsqr_st, eb.err, eb.err3, eb.chi2);
}

// ---- trial: the reduced system, assembled per block -------------------------------------------------------
// (the 16x16 block storage, sw16 and BlockPat: omv_ldlt.h)
// One block per reduced-system block: the group records of the block in group order (each sum JP^T W JP - sum
// Hpl Dinv Hpl^T over the group's edges / landmarks), the inertial edges touching it, + lambda on the diagonal; on a
// diagonal block the keyframe's b and Schur right-hand side from the records' rows.  `pose_lambda` is 0 on the ranks
// > 0 of a sharded solve (lambda enters once).
// sum of n runs of `stride` doubles (entry `off` of each), in run order; eight loads in flight, the same order of adds
__device__ __forceinline__ double run_sum(const double *base, int n, int stride, int off) {
    double v = 0;
    int q = 0;
    for (; q + 8 <= n; q += 8) {
        double a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = base[(size_t)(q + u) * stride + off];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += a[u];
    }
    for (; q < n; ++q) v += base[(size_t)q * stride + off];
    return v;
}

// One block per reduced-system block: its run of group records in group order (each sum JP^T W JP - sum
// Hpl Dinv Hpl^T over one group's edges / landmarks), the inertial edges touching it, + lambda on the diagonal; on a
// diagonal block the keyframe's b and Schur right-hand side from its run of [gradient | Schur rhs] records.
// `pose_lambda` is 0 on the ranks > 0 of a sharded solve (lambda enters once).
// The record runs are long (a block's records come from every landmark group touching it): each of the 36 entries'
// runs (and, on a diagonal block, the 12 right-hand-side runs) is cut into kAsmSplit fixed contiguous pieces summed by
// separate threads, the pieces then added in piece order -- a fixed order, so the result is the same run to run.
constexpr int kAsmSplit = 7;

// FullInertialBA's bInit form (Optimizer.cc:441-450, :484-487, :544-563): one VertexGyroBias / VertexAccBias pair for
// every keyframe, as block `blk` of the reduced system (rows 9..14 of its 16; -1: every keyframe has its own pair, the
// other members unused).  An inertial edge then has three sides (LbaPlan::imu_blk): side 2 is the pair's block and
// takes the G / A variables of the edge's form, local 9..14 (kf1's in the per-keyframe form; the residual reads
// bg[kf1], and every bImu keyframe holds the pair's value), sides 0 / 1 keep P and V (local 0..8, 15..23).
// EdgePriorGyro / EdgePriorAcc (G2oTypes.h:704-747, G2oTypes.cc:787-795): error 0 - b, Jacobian -I, information
// prior * I3, no robust kernel: prior on the block's diagonal, -J^T Omega e = prior * (0 - b) in its gradient.
struct SharedB {
    int blk, kf;               // the pair's block; a keyframe holding its value
    double prior_g, prior_a;   // infoPriorG / infoPriorA (floats widened, :554, :560)
    const double *bg[2], *ba[2];   // the two state buffers' bias arrays
};
__device__ __forceinline__ int imu_loc(int side, int r) { return side == 2 ? r : 15 * side + r; }
__device__ __forceinline__ bool imu_loc_ok(int side, int r) { return side == 2 ? r >= 9 : r < 9; }

__global__ void __launch_bounds__(256) assemble_kernel(Gather G, Imu I, BlockPat P, SharedB B, const double *rec,
                                                       const double *rec_rhs, double lambda, int pose_lambda, double *S,
                                                       double *bvec, double *coef, const LmCtl *ctl) {
    if (!gate_open(ctl, kGateTrial)) return;
    __shared__ double part[kAsmSplit][36], rpart[kAsmSplit][12];
    lambda = lm_lambda(ctl, lambda);
    const int t = blockIdx.x, tid = threadIdx.x;
    const int kr = P.slot_kr[t], kc = P.slot_kc[t];
    const bool diag = kr == kc;
    const bool shared = B.blk >= 0;   // launch-uniform
    if (tid < 36 * kAsmSplit) {
        const int pair = tid % 36, piece = tid / 36;
        const int g0 = G.blk_start[t], n = G.blk_start[t + 1] - g0, chunk = (n + kAsmSplit - 1) / kAsmSplit;
        const int q0 = min(n, piece * chunk), q1 = min(n, q0 + chunk);
        const bool need = !diag || (pair % 6) <= (pair / 6);
        part[piece][pair] = need ? run_sum(rec + (size_t)(g0 + q0) * 36, q1 - q0, 36, pair) : 0.0;
    }
    if (diag) {   // (block-uniform) the right-hand-side pieces on threads 0..83 once their record pieces are done
        __syncthreads();
        if (tid < 12 * kAsmSplit) {
            const int col = tid % 12, piece = tid / 12;
            const int k0 = G.rhs_start[kr], n = G.rhs_start[kr + 1] - k0, chunk = (n + kAsmSplit - 1) / kAsmSplit;
            const int q0 = min(n, piece * chunk), q1 = min(n, q0 + chunk);
            rpart[piece][col] = run_sum(rec_rhs + (size_t)(k0 + q0) * 12, q1 - q0, 12, col);
        }
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15;
    double v = 0;
    if (!diag || c <= r) {
        if (r < 6 && c < 6)
            for (int piece = 0; piece < kAsmSplit; ++piece) v += part[piece][6 * r + c];
        if (shared) {
            if (r < 15 && c < 15) {   // three-sided inertial edges (a keyframe with one is bImu: the plan's check)
                for (int q = G.ib_start[t]; q < G.ib_start[t + 1]; ++q) {
                    const int4 e = G.imu_blk[q];
                    if (imu_loc_ok(e.y, r) && imu_loc_ok(e.z, c))
                        v += G.contrib[(size_t)e.x * kImuContrib + imu_loc(e.y, r) * kImuLoc + imu_loc(e.z, c)];
                }
                if (kr == B.blk && diag && r == c && r >= 9) v += r < 12 ? B.prior_g : B.prior_a;   // the two priors
            }
        } else if (r < 15 && c < 15) {   // inertial edges touching the block (variable groups present in the system)
            const bool rows_ok = r < 6 || I.offV[kr] >= 0, cols_ok = c < 6 || I.offV[kc] >= 0;
            if (rows_ok && cols_ok)
                for (int q = G.ib_start[t]; q < G.ib_start[t + 1]; ++q) {
                    const int4 e = G.imu_blk[q];
                    v += G.contrib[(size_t)e.x * kImuContrib + (15 * e.y + r) * kImuLoc + 15 * e.z + c];
                }
        }
        if (diag && r == c && pose_lambda) v += lambda;
    }
    S[(size_t)t * 256 + sw16(r, c)] = v;
    if (diag && tid < 16) {   // b and the Schur right-hand side of keyframe kr
        double bv = 0, cf = 0;
        if (tid < 6)
            for (int piece = 0; piece < kAsmSplit; ++piece) bv += rpart[piece][tid], cf += rpart[piece][6 + tid];
        if (shared) {
            if (tid < 15)
                for (int q = G.iv_start[kr]; q < G.iv_start[kr + 1]; ++q) {
                    const int2 e = G.imu_vec[q];
                    if (imu_loc_ok(e.y, tid)) bv += G.contrib[(size_t)e.x * kImuContrib + kImuLoc * kImuLoc + imu_loc(e.y, tid)];
                }
            if (kr == B.blk && tid >= 9 && tid < 15) {   // the priors at the current state's pair
                const int cur = role_buf(ctl, 0);
                bv += tid < 12 ? B.prior_g * (0.0 - B.bg[cur][3 * B.kf + tid - 9]) : B.prior_a * (0.0 - B.ba[cur][3 * B.kf + tid - 12]);
            }
        } else if (tid < 15 && (tid < 6 || I.offV[kr] >= 0))
            for (int q = G.iv_start[kr]; q < G.iv_start[kr + 1]; ++q) {
                const int2 e = G.imu_vec[q];
                bv += G.contrib[(size_t)e.x * kImuContrib + kImuLoc * kImuLoc + 15 * e.y + tid];
            }
        bvec[16 * kr + tid] = bv;
        coef[16 * kr + tid] = cf;
    }
}

// ---- trial: keyframe update (in the errors kernel) -----------------------------------------------------------
// ImuCamPose::Update (G2oTypes.cc:211-235): the new body pose of optimisable keyframe k from the current state a and the
// solution xp (keyframe order), and camera c's Rcw / tcw of it.
__device__ __forceinline__ void kf_trial_pose(const Rig &rig, const State &a, const double *u, int k, int c, bool norm,
                                              double Rn[9], double twb[3], double Rc[9], double tc[3]) {
    double Rwb[9], dRw[9], tt[3];
    for (int q = 0; q < 9; ++q) Rwb[q] = a.Rwb[9 * k + q];
    mv3(Rwb, u + 3, tt);
    for (int q = 0; q < 3; ++q) twb[q] = a.twb[3 * k + q] + tt[q];
    exp_so3(u, dRw);
    mm3(Rwb, dRw, Rn);
    if (norm) polar3(Rn);   // NormalizeRotation after every third update (:220-225)
    double Rbw[9], tbw[3];
    tr3(Rn, Rbw);
    mv3(Rbw, twb, tbw);
    for (int q = 0; q < 3; ++q) tbw[q] = -tbw[q];
    mm3(rig.Rcb[c], Rbw, Rc);
    mv3(rig.Rcb[c], tbw, tc);
    for (int q = 0; q < 3; ++q) tc[q] += rig.tcb[c][q];
}

// The kind's keyframe update.  Visual: VertexSE3Expmap::oplusImpl, exp(u) * T with u = (omega, upsilon); the new q
// comes back in Rn[0..3] (the rest of the slot zero) and the new t in twb.
template <bool V>
__device__ __forceinline__ void kind_trial_pose(const Rig &rig, const Kind<V> &kd, const State &a, const double *u, int k,
                                                int c, bool norm, double Rn[9], double twb[3], double Rc[9], double tc[3]) {
    if constexpr (V) {
        se3_oplus(u, a.Rwb + 9 * k, a.twb + 3 * k, Rn, twb);
        for (int q = 4; q < 9; ++q) Rn[q] = 0.0;
        vis_cam_pose(rig, kd, c, Rn, twb, Rc, tc);
    } else {
        kf_trial_pose(rig, a, u, k, c, norm, Rn, twb, Rc, tc);
    }
}

// ---- trial: block LDL^T of the reduced system: ldlt_kernel and its helpers, omv_ldlt.h --------------------------

// ---- errors: computeActiveErrors, one workgroup per landmark group --------------------------------------
// Block 0 (when there are inertial edges or a trial): on a trial (xp) the keyframe update of every optimisable keyframe
// into the trial state (one thread per keyframe and camera) and the pose part of computeScale (scale_partial[0]), then
// the inertial / random-walk errors of that state (this block wrote it: a block-scope fence orders it).  Blocks 1..:
// the landmark groups of the build (whole landmarks and their edges), XCD-contiguous.  On a trial a group first
// back-substitutes its landmarks, xl = Dinv (bl - sum_s Hpl_s^T xp_s) = R^-T (y - sum_s M_s^T xp_s) from the build's
// R^-1, y and M_s (the trial point into the trial state and LDS; the landmark part of computeScale into
// scale_partial[1 + g]) while its other threads form the trial Rcw / tcw of the group's keyframes in LDS (the same
// arithmetic as block 0's: no block reads another's writes), then its edges' errors.  Without xp the points and poses
// are the state's.  The state / error buffers are the role's (role_buf); the updates start from the role-0 state.
struct ErrTrial {
    const double *xp;        // the solution (keyframe order), or null: no update
    int norm;                // host driver: this trial normalises the keyframe rotations (the device driver reads it
                             // from the control block)
    const double *b;         // the assembled gradient (keyframe order)
    double lambda;
    const int *offV, *offG, *offA;
    int n_opt;
    const int16_t *e_lkf;    // [E] the edge keyframe's index in its group's list, -1 fixed
    const int *lkf_kf;       // per group (at Land::grp_kf[g]) its keyframes
    // the shared bias pair (SharedB; shared_kf < 0: none): the fixed keyframes n_opt .. bias_end - 1 take its step too
    // (offG / offA of every bImu keyframe are the pair's rows), and its two prior edges add prior * |b|^2 to the chi2
    int shared_kf, bias_end;
    double prior_g, prior_a;
};
template <bool V>
__global__ void __launch_bounds__(256) err_kernel(int n_grp, int lead, int has_imu, Rig rig, Kind<V> kd, State s0, State s1, Edges E,
                                                  Land L, Red R, ErrTrial T, double delta, double dsqr, double delta_st,
                                                  double dsqr_st, ErrBufs e0, ErrBufs e1, double *partial,
                                                  double *scale_partial, Imu I, double delta_imu, double dsqr_imu,
                                                  double *imu_partial, const LmCtl *ctl, int gate, int role,
                                                  LmReset reset) {
    __shared__ double sh[8];
    extern __shared__ double dyn[];   // 3 per landmark, then 12 per (group keyframe, camera)
    if (reset.c && blockIdx.x == 0 && threadIdx.x == 0) ctl_reset(reset), reset.c->init_pending = 1;
    if (!gate_open(ctl, gate)) return;
    const int bi = role_buf(ctl, role);
    const State s = bi ? s1 : s0;
    const State a = role_buf(ctl, 0) ? s1 : s0;
    const ErrBufs eb = bi ? e1 : e0;
    const bool trial = T.xp != nullptr;
    const bool norm = ctl ? ctl->n_acc % 3 == 2 : T.norm != 0;
    const double lambda = trial ? lm_lambda(ctl, T.lambda) : 0.0;
    const int tid = threadIdx.x, C = rig.n_cams;
    int bid = blockIdx.x;
    if (lead) {
        if (bid == 0) {
            if (trial) {
                for (int t = tid; t < T.n_opt * C; t += blockDim.x) {
                    const int k = t / C, c = t - k * C;
                    double Rn[9], twb[3], Rc[9], tc[3];
                    kind_trial_pose<V>(rig, kd, a, T.xp + R.offP[k], k, c, norm, Rn, twb, Rc, tc);
                    for (int q = 0; q < 9; ++q) s.Rcw[((size_t)k * C + c) * 9 + q] = Rc[q];
                    for (int q = 0; q < 3; ++q) s.tcw[((size_t)k * C + c) * 3 + q] = tc[q];
                    if (c == 0) {
                        for (int q = 0; q < 9; ++q) s.Rwb[9 * k + q] = Rn[q];
                        for (int q = 0; q < 3; ++q) {
                            s.twb[3 * k + q] = twb[q];
                            s.vel[3 * k + q] = a.vel[3 * k + q] + (T.offV[k] >= 0 ? T.xp[T.offV[k] + q] : 0.0);
                            s.bg[3 * k + q] = a.bg[3 * k + q] + (T.offG[k] >= 0 ? T.xp[T.offG[k] + q] : 0.0);
                            s.ba[3 * k + q] = a.ba[3 * k + q] + (T.offA[k] >= 0 ? T.xp[T.offA[k] + q] : 0.0);
                        }
                    }
                }
                for (int k = T.n_opt + tid; k < T.bias_end; k += blockDim.x)   // (shared pair only) fixed bImu keyframes
                    if (T.offG[k] >= 0)
                        for (int q = 0; q < 3; ++q) {
                            s.bg[3 * k + q] = a.bg[3 * k + q] + T.xp[T.offG[k] + q];
                            s.ba[3 * k + q] = a.ba[3 * k + q] + T.xp[T.offA[k] + q];
                        }
                double sc = 0;   // pose part of sum_j x_j (lambda x_j + b_j); b is the assembled gradient (bvec)
                for (int q = tid; q < R.n; q += blockDim.x) sc += T.xp[q] * (lambda * T.xp[q] + T.b[q]);
                const double tt = block_reduce_sum(sc, sh);
                if (tid == 0) scale_partial[0] = tt;
                __threadfence_block();
                __syncthreads();
            }
            if (has_imu) imu_err_block(sh, s, I, delta_imu, dsqr_imu, eb.err9, imu_partial);
            if (T.shared_kf >= 0 && tid == 0) {   // EdgePriorGyro + EdgePriorAcc (thread 0 wrote the partial itself)
                const double *g = s.bg + 3 * T.shared_kf, *ac = s.ba + 3 * T.shared_kf;
                imu_partial[0] += T.prior_g * (g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) +
                                  T.prior_a * (ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
            }
            return;
        }
        --bid;
    }
    const int chunk = (n_grp + 7) >> 3, g = (bid & 7) * chunk + (bid >> 3);
    if (g >= n_grp) return;
    const int p0 = L.grp_pt[g], np = L.grp_pt[g + 1] - p0;
    const int f0 = L.edge_start[p0], ne = L.edge_start[p0 + np] - f0;
    const int w = L.grp_w[g];   // < 0: a one-landmark group past the LDS limits (its poses per edge)
    double *X = dyn, *PS = dyn + 3 * kGrpLand;
    double sc = 0;
    if (tid < np) {
        const int p = p0 + tid;
        double Xp[3];
        if (trial) {
            const double *l = L.lnd + (size_t)p * 12;
            double Ri[6], c[3], bl[3];
            for (int q = 0; q < 6; ++q) Ri[q] = l[q];
            for (int q = 0; q < 3; ++q) c[q] = l[6 + q], bl[q] = l[9 + q];
            for (int sl = L.slot_start[p]; sl < L.slot_start[p + 1]; ++sl) {
                const int o = R.offP[L.slot_kf[sl]];
                if (o < 0) continue;
                const double *M = L.M + (size_t)sl * 18;
                for (int q = 0; q < 3; ++q)
                    for (int r = 0; r < 6; ++r) c[q] -= M[3 * r + q] * T.xp[o + r];
            }
            const double xl[3] = {Ri[0] * c[0] + Ri[1] * c[1] + Ri[3] * c[2], Ri[2] * c[1] + Ri[4] * c[2], Ri[5] * c[2]};
            for (int q = 0; q < 3; ++q) {
                Xp[q] = a.pts[(size_t)p * 3 + q] + xl[q];
                s.pts[(size_t)p * 3 + q] = Xp[q];
                sc += xl[q] * (lambda * xl[q] + bl[q]);
            }
        } else {
            for (int q = 0; q < 3; ++q) Xp[q] = s.pts[(size_t)p * 3 + q];
        }
        for (int q = 0; q < 3; ++q) X[3 * tid + q] = Xp[q];
    } else if (tid >= kGrpLand && trial && w > 0) {   // threads 128..: the trial poses of the group's keyframes
        for (int t = tid - kGrpLand; t < w * C; t += blockDim.x - kGrpLand) {
            const int la = t / C, c = t - la * C, k = T.lkf_kf[L.grp_kf[g] + la];
            double Rn[9], twb[3];
            kind_trial_pose<V>(rig, kd, a, T.xp + R.offP[k], k, c, norm, Rn, twb, PS + 12 * t, PS + 12 * t + 9);
        }
    }
    __syncthreads();
    double r0 = 0;
    for (int f = tid; f < ne; f += blockDim.x) {
        const int e = f0 + f, la = trial ? T.e_lkf[e] : -1, cam = E.cam[e];
        double Rc[9], tc[3];   // the edge camera's pose, in registers
        if (la < 0) {          // a fixed keyframe (identical in both buffers), or not a trial
            const size_t o = (size_t)E.kf[e] * C + cam;
            for (int q = 0; q < 9; ++q) Rc[q] = s.Rcw[o * 9 + q];
            for (int q = 0; q < 3; ++q) tc[q] = s.tcw[o * 3 + q];
        } else if (w > 0) {
            const double *o = PS + 12 * (la * C + cam);
            for (int q = 0; q < 9; ++q) Rc[q] = o[q];
            for (int q = 0; q < 3; ++q) tc[q] = o[9 + q];
        } else {   // the scalar group: per edge
            double Rn[9], twb[3];
            kind_trial_pose<V>(rig, kd, a, T.xp + R.offP[E.kf[e]], E.kf[e], cam, norm, Rn, twb, Rc, tc);
        }
        r0 += kind_err_edge<V>(rig, kd, Rc, tc, E, e, X + 3 * (E.pt[e] - p0), delta, dsqr, delta_st, dsqr_st, eb.err,
                               eb.err3, eb.chi2);
    }
    const double t = block_reduce_sum(r0, sh);
    if (tid == 0) partial[g] = t;
    if (trial) {
        __syncthreads();
        const double ts = block_reduce_sum(sc, sh);
        if (tid == 0) scale_partial[1 + g] = ts;
    }
}

// The optimisation's epilogue on the device (single rank): per visual edge the reference's outlier test
// (Optimizer.cc:3282-3311: EdgeMono chi2 > 5.991, or > 1.5 * 5.991 when the point's trackDepth < 10, or a
// non-positive depth; EdgeStereo chi2 > 7.815) at the final state, written in the caller's edge order with
// the chi2, and the points in the caller's order; the host reads one staging block.
// The visual kind: chi2 > 5.991 (7.815 on a stereo edge) || !isDepthPositive on every edge (Optimizer.cc:1729-1783), the
// depth being the z of the edge's own camera.
template <bool V>
__global__ void epilogue_kernel(Rig rig, State s0, State s1, size_t n_state, Edges E, const int *perm_edge,
                                int n_mono_all, const float *track_depth, const int *perm_pt, int n_pts, uint8_t *flags,
                                double *chi2_out, double *pts_out, const double *chi2_0, const double *chi2_1,
                                const LmCtl *ctl, double *head, int n_head) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const double *chi2 = ctl && ctl->last ? chi2_1 : chi2_0;   // the last computed errors (a rejected trial's too)
    // the device driver's current state (double-buffered); buffer 1 is also copied into buffer 0, where the next
    // optimize() starts
    const bool in1 = ctl && ctl->cur;
    const State s = in1 ? s1 : s0;
    if (in1)
        for (size_t k = q; k < n_state; k += (size_t)gridDim.x * blockDim.x) s0.Rwb[k] = s1.Rwb[k];
    if (q < n_head) head[q] = s.Rwb[q];   // the keyframe part of the state (it precedes the points)
    if (q < E.n) {
        const int e = q, o = perm_edge[e];
        const double c2 = chi2[e];
        uint8_t f;
        if constexpr (V) {
            const int k = E.kf[e], c = E.cam[e], p = E.pt[e], C = rig.n_cams;
            const double *R = s.Rcw + ((size_t)k * C + c) * 9, *t = s.tcw + ((size_t)k * C + c) * 3;
            const double *X = s.pts + 3 * (size_t)p;
            const bool depth_pos = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]) > 0.0;
            f = (c2 > (o >= n_mono_all ? 7.815 : 5.991) || !depth_pos) ? 1 : 0;
        } else if (o >= n_mono_all) {
            f = c2 > 7.815f ? 1 : 0;
        } else {
            const int k = E.kf[e], c = E.cam[e], p = E.pt[e], C = rig.n_cams;
            const double *R = s.Rcw + ((size_t)k * C + c) * 9, *t = s.tcw + ((size_t)k * C + c) * 3;
            const double *X = s.pts + 3 * (size_t)p;
            const bool depth_pos = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]) > 0.0;
            const bool close = track_depth[p] < 10.f;
            f = ((c2 > 5.991f && !close) || (c2 > 1.5f * 5.991f && close) || !depth_pos) ? 1 : 0;
        }
        flags[o] = f;
        if (chi2_out) chi2_out[o] = c2;
    }
    if (q < n_pts)
        for (int d = 0; d < 3; ++d) pts_out[3 * (size_t)perm_pt[q] + d] = s.pts[3 * (size_t)q + d];
}

// ---- evaluation helpers for parity ---------------------------------------------------------------
// [9] / [18] per edge: 3 residual rows (the third is zero on an EdgeMono)
__global__ void mono_jac_kernel(Rig rig, State s, Edges E, double *jx, double *jp) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E.n) return;
    const int k = E.kf[e], c = E.cam[e], C = rig.n_cams;
    const double *Rcw = s.Rcw + ((size_t)k * C + c) * 9, *tcw = s.tcw + ((size_t)k * C + c) * 3;
    const double *X = s.pts + (size_t)E.pt[e] * 3;
    double Xc[3], Xb[3];
    mv3(Rcw, X, Xc);
    for (int q = 0; q < 3; ++q) Xc[q] += tcw[q];
    mv3(rig.Rbc[c], Xc, Xb);
    for (int q = 0; q < 3; ++q) Xb[q] += rig.tbc[c][q];
    double pj[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    cam_jac(rig, c, Xc, pj);
    if (E.ur[e] >= 0.f) {
        const double inv_z2 = 1.0 / (Xc[2] * Xc[2]);
        pj[6] = pj[0], pj[7] = pj[1], pj[8] = pj[2] + rig.bf * inv_z2;
    }
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q)
            jx[9 * e + 3 * r + q] = -(pj[3 * r] * Rcw[q] + pj[3 * r + 1] * Rcw[3 + q] + pj[3 * r + 2] * Rcw[6 + q]);
    double pr[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q)
            pr[3 * r + q] = pj[3 * r] * rig.Rcb[c][q] + pj[3 * r + 1] * rig.Rcb[c][3 + q] + pj[3 * r + 2] * rig.Rcb[c][6 + q];
    const double x = Xb[0], y = Xb[1], z = Xb[2];
    const double se3[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 6; ++q)
            jp[18 * e + 6 * r + q] = pr[3 * r] * se3[q] + pr[3 * r + 1] * se3[6 + q] + pr[3 * r + 2] * se3[12 + q];
}

// The visual kind's Jacobians for parity, in the same layout.
__global__ void vis_jac_kernel(Rig rig, Kind<true> kd, State s, Edges E, const double *err, const double *err3,
                               const double *chi2, double *jx, double *jp) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E.n) return;
    double JX[9], JP[18], w, om[3];
    vis_edge_jacobians(rig, kd, s, E, e, err, err3, chi2, JX, JP, w, om);
    for (int q = 0; q < 9; ++q) jx[9 * (size_t)e + q] = JX[q];
    for (int q = 0; q < 18; ++q) jp[18 * (size_t)e + q] = JP[q];
}

// Every keyframe's per-camera Rcw / tcw from its (q, t) (set_problem: the same arithmetic as a trial's).
__global__ void vis_cams_kernel(Rig rig, Kind<true> kd, State s, int n_kf) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, C = rig.n_cams;
    if (q >= n_kf * C) return;
    const int k = q / C, c = q - k * C;
    double Rc[9], tc[3];
    vis_cam_pose(rig, kd, c, s.Rwb + 9 * k, s.twb + 3 * k, Rc, tc);
    for (int i = 0; i < 9; ++i) s.Rcw[(size_t)q * 9 + i] = Rc[i];
    for (int i = 0; i < 3; ++i) s.tcw[(size_t)q * 3 + i] = tc[i];
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp:171-185): max |H(j,j)| over the active vertices at the
// current errors -- block k < n_opt: keyframe k's sum w JP^T JP diagonal over its edges (kf_edge, ascending: a fixed
// order); block n_opt + g: the landmarks of group g, one thread each (sum w JX^T JX diagonal in edge order) -- one
// maximum per block into `out`.  Runs at the first step of an optimize() whose lambda_init is <= 0.
__global__ void __launch_bounds__(256) vis_diag_kernel(Rig rig, Kind<true> kd, State s0, Edges E, Land L, int n_opt,
                                                       const int *kf_edge_start, const int *kf_edge, ErrBufs eb,
                                                       double *out, const LmCtl *c) {
    __shared__ double sh[8];
    __shared__ double mx[256];
    if (!c->init_pending || c->lambda_init > 0) return;
    const int tid = threadIdx.x, b = blockIdx.x;
    double m = 0;
    if (b < n_opt) {
        double d[6] = {0, 0, 0, 0, 0, 0};
        for (int q = kf_edge_start[b] + tid; q < kf_edge_start[b + 1]; q += blockDim.x) {
            double JX[9], JP[18], w, om[3];
            vis_edge_jacobians(rig, kd, s0, E, kf_edge[q], eb.err, eb.err3, eb.chi2, JX, JP, w, om);
            for (int j = 0; j < 6; ++j) d[j] += w * rows3(JP, j, 6, JP, j, 6);
        }
        for (int j = 0; j < 6; ++j) {
            const double t = block_reduce_sum(d[j], sh);
            m = fmax(m, fabs(t));
        }
        if (tid == 0) out[b] = m;
        return;
    }
    const int g = b - n_opt, p0 = L.grp_pt[g], np = L.grp_pt[g + 1] - p0;
    for (int pl = tid; pl < np; pl += blockDim.x) {
        double d[3] = {0, 0, 0};
        for (int e = L.edge_start[p0 + pl]; e < L.edge_start[p0 + pl + 1]; ++e) {
            double JX[9], JP[18], w, om[3];
            vis_edge_jacobians(rig, kd, s0, E, e, eb.err, eb.err3, eb.chi2, JX, JP, w, om);
            for (int j = 0; j < 3; ++j) d[j] += w * rows3(JX, j, 3, JX, j, 3);
        }
        m = fmax(m, fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))));
    }
    mx[tid] = m;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < (int)blockDim.x; ++q) m = fmax(m, mx[q]);
        out[b] = m;
    }
}
// lambda = computeLambdaInit of the maximum of the blocks' maxima.
__global__ void __launch_bounds__(256) vis_lambda_kernel(const double *part, int n, LmCtl *c) {
    __shared__ double mx[256];
    if (!c->init_pending || c->lambda_init > 0) return;
    double m = 0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) m = fmax(m, part[q]);
    mx[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < (int)blockDim.x; ++q) m = fmax(m, mx[q]);
        c->lm.lambda = c->lambda_init = omv_lm::lm_lambda_init(c->lambda_init, m);
    }
}

}  // namespace

// =============================================================================================
// The single-rank epilogue's staging block, on the device and in pinned memory alike, in doubles:
// [state without points (head) | P points | E outlier flags, padded to 8 bytes | E chi2], edges and points in the
// caller's order.
struct StageLayout {
    size_t head, P, E;
    size_t pts() const { return head; }
    size_t flags() const { return head + 3 * P; }
    size_t chi2() const { return flags() + (E + 7) / 8; }
    size_t bytes(bool with_chi2) const { return (chi2() + (with_chi2 ? E : 0)) * sizeof(double); }
};

// What omv_lba_set_problem fills: the host plan, the counts and every pointer into the problem arena.  One value, so
// that a handle without a problem is this struct's default.
struct LbaDeviceProblem {
    Rig rig{};
    LbaPlan plan;   // the host plan (lba_plan.h): orders, pattern, schedule, groups, LDS mode
    int n_kf = 0, n_opt = 0, n_pts = 0, n_mono = 0, n_imu = 0;
    int n_mono_all = 0, n_stereo_all = 0;   // caller edge counts (perm_edge >= n_mono_all: EdgeStereo)
    bool imu_here = false;     // this rank evaluates the inertial edges (rank 0)
    State st[3]{};   // current / trial (push-pop double buffer) / the uploaded initial state
    int cur = 0;
    Edges E{};
    Land L{};
    Red R{};
    Imu I{};
    LdltSolver ldlt{};   // the uploaded block pattern (ldlt.pat) and the solver's launch on it
    Gather G{};
    SharedB sb{-1, -1, 0.0, 0.0, {nullptr, nullptr}, {nullptr, nullptr}};   // the shared bias pair (omv_fiba's bInit form)
    // omv_fiba: the caller's edges in the graph (a map point seen by fixed keyframes only is no vertex, its edges are
    // left out): graph edge -> caller edge
    std::vector<int> fiba_mono, fiba_stereo;
    int fiba_n_mono = 0, fiba_n_stereo = 0;   // the caller's edge counts
    double *d_imu_contrib = nullptr;   // [n_imu][30 x 30 + 30] per-edge inertial contributions
    const int16_t *d_e_lkf = nullptr;   // per edge: its keyframe's index in the group's list (-1: fixed)
    const int *d_lkf_kf = nullptr;      // per (group, local keyframe): the keyframe
    const int *d_big = nullptr;
    // device epilogue (single rank): the plan's perm_edge / order / track_depth on the device, one staging block
    int *d_perm_edge = nullptr, *d_perm_pt = nullptr;
    float *d_track_depth = nullptr;
    double *d_stage = nullptr, *h_stage = nullptr;
    StageLayout stage() const { return StageLayout{(size_t)(st[0].pts - st[0].Rwb), (size_t)n_pts, (size_t)n_mono}; }
    bool epi_ready = false;    // the staging block holds this optimize()'s final result
    bool epi_chi2 = false;     //   including the chi2
    int *d_offP = nullptr, *d_offV = nullptr, *d_offG = nullptr, *d_offA = nullptr;
    double *d_err = nullptr, *d_chi2 = nullptr, *d_err9 = nullptr, *d_err3 = nullptr;
    double *d_err_b = nullptr, *d_chi2_b = nullptr, *d_err9_b = nullptr, *d_err3_b = nullptr;   // the second error buffer
    ErrBufs eb(int i) const { return i ? ErrBufs{d_err_b, d_err3_b, d_chi2_b, d_err9_b} : ErrBufs{d_err, d_err3, d_chi2, d_err9}; }
    double *d_partial = nullptr, *d_imu_partial = nullptr, *d_scale_partial = nullptr, *d_out = nullptr;
    double *d_partial0 = nullptr, *d_imu_partial0 = nullptr;   // optimize()'s initial errors (device driver)
    double *d_S = nullptr, *d_coef = nullptr, *d_x = nullptr, *d_scratch = nullptr;
    int *d_fail = nullptr;
    double *d_bb = nullptr;    // the trial's copy of b (all-reduced with the packed system when sharded)
    // the visual kind (omv_vba): its constants, Huber deltas and level mask, and computeLambdaInit's work lists
    Kind<true> vis{};
    double *d_huber = nullptr, *d_diag = nullptr;   // [2]; [n_opt + n_lgrp] the blocks' diagonal maxima
    uint8_t *d_level = nullptr;                     // [E] device order
    int *d_kf_edge_start = nullptr, *d_kf_edge = nullptr;   // per optimisable keyframe its edges (device order, ascending)
    size_t state_doubles() const { return (size_t)n_kf * (24 + 12 * rig.n_cams) + 3 * (size_t)n_pts; }
};

struct omv_lba : LbaDeviceProblem {
    int max_kf, max_cams, max_pts, max_mono, max_imu;
    omv::DeviceArena mem;    // the handle's own blocks: h_out, h_ctl, d_ctl
    omv::DeviceArena prob;   // the current problem's device buffers and h_stage
    ~omv_lba();
    double *h_out = nullptr;   // pinned host copy of d_out: the per-trial 24-byte read-back
    LmCtl *d_ctl = nullptr;    // device-resident LM control (single-rank path)
    LmCtl *h_ctl = nullptr;    // pinned copy: the one read-back per optimize()
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;   // one LM step (trial, and buildSystem when an iteration starts)
    hipGraph_t step4_graph = nullptr;
    hipGraphExec_t step4_exec = nullptr;  // four LM steps in one launch (no launch gap between them)
    // four LM steps + the speculative epilogue + the staging and control read-backs (index: chi2 read-back or not):
    // the batch that usually ends the optimize() in one launch (a graph -> kernel -> copy transition on the stream
    // costs ~10 us each)
    hipGraph_t step4e_graph[2] = {nullptr, nullptr};
    hipGraphExec_t step4e_exec[2] = {nullptr, nullptr};
    bool timing = false;       // direct launches with per-stage events instead of the captured step
    bool host_lm = false;      // force the host-driven LM loop (parity checks of the device control)
    bool visual = false;       // an omv_vba handle: the visual kind of every kernel that depends on the parameterisation
    bool fiba = false;         // an omv_fiba handle: FullInertialBA's graph on the inertial kind's kernels
    int rank = 0, world = 1;   // landmark sharding (omv_lba_set_comm)
    omv_allreduce_fn allreduce = nullptr;
    void *ar_ctx = nullptr;
    bool lds_ok = false;
    // Huber deltas; thHuberMono / thHuberStereo are floats (:3028-3031)
    const double delta_mono = (double)(float)std::sqrt(5.991), dsqr_mono = delta_mono * delta_mono;
    const double delta_st = (double)(float)std::sqrt(7.815), dsqr_st = delta_st * delta_st;
    const double delta_imu = std::sqrt(16.92), dsqr_imu = delta_imu * delta_imu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    double stage_ms[4] = {0, 0, 0, 0};
    int last_trials = 0;
    int host_syncs = 0;        // host waits of the last optimize()'s LM loop (the device driver: one per batch)
};

// Has a problem: omv_lba_set_problem succeeded and nothing has freed it since.
static bool has_problem(const omv_lba *h) { return h->st[2].pts != nullptr; }

// The handle without a problem: the arena reset, the captured steps destroyed, the counts zero and every pointer into
// the arena null -- also where a failed upload ends.
static void free_problem(omv_lba *h) {
    h->prob.reset();
    static_cast<LbaDeviceProblem &>(*h) = LbaDeviceProblem{};
    hipGraphExec_t *execs[] = {&h->step_exec, &h->step4_exec, &h->step4e_exec[0], &h->step4e_exec[1]};
    hipGraph_t *graphs[] = {&h->step_graph, &h->step4_graph, &h->step4e_graph[0], &h->step4e_graph[1]};
    for (int q = 0; q < 4; ++q) {   // the captured steps hold the old problem's pointers
        if (*execs[q]) (void)hipGraphExecDestroy(*execs[q]);
        if (*graphs[q]) (void)hipGraphDestroy(*graphs[q]);
        *execs[q] = nullptr, *graphs[q] = nullptr;
    }
}

// Both state buffers hold the uploaded state (st[2]) again and the first is the current one; waits for the copies.
// omv_lba_reset, and the end of vba_upload, where `cur` is 0 already (free_problem) and setting it changes nothing.
static omv_status restore_uploaded_state(omv_lba *h) {
    for (int b = 0; b < 2; ++b)
        HIP_OK(hipMemcpyAsync(h->st[b].Rwb, h->st[2].Rwb, h->state_doubles() * sizeof(double), hipMemcpyDeviceToDevice,
                              h->stream));
    h->cur = 0;
    HIP_OK(hipStreamSynchronize(h->stream));
    return OMV_OK;
}

omv_lba::~omv_lba() {   // `mem` frees h_out, h_ctl and d_ctl after this body
    free_problem(this);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

// The device side of omv_lba_set_problem: h->plan (already checked) and the caller's state, rig and preintegrations
// into the problem arena, one allocation per array; the state blocks first, the pinned staging block last.  On
// OMV_ERR_HIP the caller frees the partial problem.
static omv_status upload_problem(omv_lba *h, const omv_lba_problem *p) {
    const LbaPlan &pl = h->plan;
    const int C = p->n_cams, K = p->n_kf, NI = p->n_imu, nb = pl.nb;   // nb: blocks of the reduced system
    const int P = (int)pl.order.size(), E = (int)pl.perm_edge.size(), nred = pl.n_red, n_slots = pl.n_slots;
    const size_t ni = (size_t)std::max(NI, 0);
    h->n_kf = K, h->n_opt = p->n_opt, h->n_imu = NI, h->n_pts = P, h->n_mono = E;
    h->n_mono_all = p->n_mono, h->n_stereo_all = std::max(p->n_stereo, 0);
    h->imu_here = NI > 0 && h->rank == 0;
    Rig &rig = h->rig;
    rig.n_cams = C, rig.bf = (double)p->bf;
    for (int c = 0; c < C; ++c) {
        for (int q = 0; q < 8; ++q) rig.cam[c][q] = p->cam[8 * c + q];
        rig.model[c] = p->cam_model ? p->cam_model[c] : OMV_CAM_KB8;
        for (int q = 0; q < 9; ++q) rig.Rcb[c][q] = p->Rcb[9 * c + q], rig.Rbc[c][q] = p->Rbc[9 * c + q];
        for (int q = 0; q < 3; ++q) rig.tcb[c][q] = p->tcb[3 * c + q], rig.tbc[c][q] = p->tbc[3 * c + q];
    }
    omv::Uploader up{h->prob};
    {   // one contiguous block per state: Rwb | twb | Rcw | tcw | vel | bg | ba | pts (device order): one copy to read back
        std::vector<double> init;
        auto add = [&](const double *src, size_t n) { init.insert(init.end(), src, src + n); };
        add(p->Rwb, 9 * (size_t)K), add(p->twb, 3 * (size_t)K), add(p->Rcw, 9 * (size_t)K * C), add(p->tcw, 3 * (size_t)K * C);
        add(p->vel, 3 * (size_t)K), add(p->bg, 3 * (size_t)K), add(p->ba, 3 * (size_t)K);
        for (int q : pl.order) add(p->pts + 3 * (size_t)q, 3);
        init.resize(h->state_doubles());
        for (State &s : h->st) {
            s.Rwb = up.copy(init);
            if (!up.ok) return OMV_ERR_HIP;
            s.twb = s.Rwb + 9 * K, s.Rcw = s.twb + 3 * K, s.tcw = s.Rcw + 9 * K * C;
            s.vel = s.tcw + 3 * K * C, s.bg = s.vel + 3 * K, s.ba = s.bg + 3 * K, s.pts = s.ba + 3 * K;
        }
    }
    h->E = Edges{up.copy(pl.e_pt),  up.copy(pl.e_kf), up.copy(pl.e_cam), up.copy(pl.e_slot),
                 up.copy(pl.e_obs), up.copy(pl.e_w),  up.copy(pl.e_ur),  E};
    {
        Land &L = h->L;
        L.edge_start = up.copy(pl.pt_edge), L.slot_start = up.copy(pl.pt_slot), L.slot_kf = up.copy(pl.slot_kf);
        L.slot_edge = up.copy(pl.slot_edge), L.slot_lkf = up.copy(pl.slot_lkf);
        up.buffer(&L.lnd, 12 * (size_t)P), up.buffer(&L.M, 18 * (size_t)pl.n_pt_slots);
        up.buffer(&L.rec, 36 * (size_t)pl.blk_start[n_slots]), up.buffer(&L.rec_rhs, 12 * (size_t)pl.rhs_start[nb]);
        L.n = P;
        L.grp_pt = up.copy(pl.grp_pt), L.grp_w = up.copy(pl.grp_w), L.grp_tp = up.copy(pl.grp_tp), L.tp = up.copy(pl.tp);
        L.grp_blk = up.copy(pl.grp_blk), L.blkoff = up.copy(pl.blkoff), L.grp_kf = up.copy(pl.grp_kf);
        L.rhsoff = up.copy(pl.rhsoff);
        h->d_big = up.copy(pl.big_grp), h->d_e_lkf = up.copy(pl.e_lkf), h->d_lkf_kf = up.copy(pl.lkf_kf);
    }
    h->d_offP = up.copy(pl.offP), h->d_offV = up.copy(pl.offV), h->d_offG = up.copy(pl.offG), h->d_offA = up.copy(pl.offA);
    h->R = Red{nred, h->d_offP, K};
    h->sb.blk = pl.shared_blk, h->sb.kf = pl.shared_kf;   // (the priors: omv_fiba_set_problem)
    // inertial edges, then the reduction work lists
    std::vector<uint8_t> rob(ni, 0);
    if (p->imu_robust) std::copy(p->imu_robust, p->imu_robust + ni, rob.begin());
    h->I = Imu{NI, up.copy(p->imu_kf1, ni), up.copy(p->imu_kf2, ni), up.copy(p->preint, ni * kPF), up.copy(pl.info9),
               up.copy(pl.infoG), up.copy(pl.infoA), up.copy(rob), h->d_offP, h->d_offV, h->d_offG, h->d_offA};
    up.buffer(&h->d_imu_contrib, ni * kImuContrib);
    h->G = Gather{up.copy(pl.blk_start), up.copy(pl.rhs_start), (const int4 *)up.copy(pl.imu_blk), up.copy(pl.ib_start),
                  (const int2 *)up.copy(pl.imu_vec), up.copy(pl.iv_start), h->d_imu_contrib};
    h->ldlt = LdltSolver::upload(pl, up);   // block pattern + level schedule
    if (!up.ok) return OMV_ERR_HIP;
    // work buffers
    // d_err9: [9n errors | n chi2 | 9n rotation errors eR]; the *_b set: the device driver's second (double-buffered) one
    // d_S: [packed blocks | b | coef], contiguous, the one buffer a sharded solve all-reduces per trial
    up.buffer(&h->d_err, 2 * (size_t)E), up.buffer(&h->d_chi2, E), up.buffer(&h->d_err3, E), up.buffer(&h->d_err9, 19 * ni);
    up.buffer(&h->d_err_b, 2 * (size_t)E), up.buffer(&h->d_chi2_b, E), up.buffer(&h->d_err3_b, E);
    up.buffer(&h->d_err9_b, 19 * ni), up.buffer(&h->d_partial, pl.n_lgrp), up.buffer(&h->d_imu_partial, 1);
    up.buffer(&h->d_partial0, pl.n_lgrp), up.buffer(&h->d_imu_partial0, 1), up.buffer(&h->d_scale_partial, pl.n_lgrp + 1);
    up.buffer(&h->d_out, 4), up.buffer(&h->d_S, pl.n_reduce), up.buffer(&h->d_x, nred);
    up.buffer(&h->d_scratch, LdltSolver::scratch_doubles(pl)), up.buffer(&h->d_fail, 1);
    if (!up.ok) return OMV_ERR_HIP;
    h->d_bb = h->d_S + (size_t)n_slots * 256;
    h->d_coef = h->d_bb + nred;
    HIP_OK(hipMemset(h->d_imu_partial, 0, sizeof(double)));
    HIP_OK(hipMemset(h->d_imu_partial0, 0, sizeof(double)));
    // device epilogue (single rank): caller-order permutations, trackDepth in device order, the staging block
    if (h->world == 1) {
        const size_t stage_doubles = h->stage().bytes(true) / sizeof(double);
        h->d_perm_edge = up.copy(pl.perm_edge), h->d_perm_pt = up.copy(pl.order), h->d_track_depth = up.copy(pl.track_depth);
        up.buffer(&h->d_stage, stage_doubles);
        if (!up.ok || !h->prob.alloc_pinned(&h->h_stage, stage_doubles)) return OMV_ERR_HIP;
    }
    return OMV_OK;
}

extern "C" {

omv_status omv_lba_create(int max_kf, int max_cams, int max_pts, int max_mono, int max_imu, omv_lba **out) {
    if (!out || max_kf <= 0 || max_cams <= 0 || max_cams > kMaxCams || max_pts < 0 || max_mono < 0 || max_imu < 0)
        return OMV_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OMV_ERR_NO_DEVICE;
    auto h = std::make_unique<omv_lba>();
    h->max_kf = max_kf, h->max_cams = max_cams, h->max_pts = max_pts, h->max_mono = max_mono, h->max_imu = max_imu;
    HIP_OK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (auto &e : h->ev) HIP_OK(hipEventCreate(&e));
    if (!h->mem.alloc_pinned(&h->h_out, 4) || !h->mem.alloc_pinned(&h->h_ctl, 1) || !h->mem.alloc(&h->d_ctl, 1))
        return OMV_ERR_HIP;
    // the reduced-system factorisation stages its nonzero blocks in up to 150 KB of LDS
    h->lds_ok = LdltSolver::opt_in_lds();
    // the landmark groups of the build take ~77 KB of LDS (two workgroups per CU)
    for (const void *k : {(const void *)build_all_kernel<false>, (const void *)build_big_kernel<false>,
                          (const void *)build_all_kernel<true>, (const void *)build_big_kernel<true>})
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBuildLds) != hipSuccess)
            return OMV_ERR_HIP;
    (void)hipGetLastError();
    *out = h.release();
    return OMV_OK;
}

omv_status omv_lba_destroy(omv_lba *h) {
    if (!h) return OMV_ERR_ARG;
    delete h;
    return OMV_OK;
}

omv_status omv_lba_set_problem(omv_lba *h, const omv_lba_problem *p) {
    if (!h || !p) return OMV_ERR_ARG;
    // validate and plan on the host first: a rejected problem leaves the handle and its current problem as they were
    LbaPlan plan;
    const LbaLimits lim{h->max_kf, h->max_cams, h->max_pts, h->max_mono, h->max_imu};
    const omv_status planned = plan_lba(*p, h->rank, h->world, lim, h->lds_ok, plan);
    if (planned != OMV_OK) return planned;
    free_problem(h);
    h->plan = std::move(plan);
    const omv_status rs = upload_problem(h, p);
    if (rs != OMV_OK) free_problem(h);   // a failed upload leaves no problem
    return rs;
}

}  // extern "C"

// ---- the LM driver ---------------------------------------------------------------------------------
// computeActiveErrors: the visual and inertial errors in one launch (err_kernel).
// lba_errors: the errors of state s into the first error buffer (host driver, optimize()'s start, evaluation);
// lba_trial_errors: the device driver's trial state and buffer (role 1 of the control block's `cur`).
// n_grp_err: the partial count of the visual errors (one per landmark group, in the group order).
// launch_errors: s0 / s1 and the error buffers by role (role_buf); `xp` (a trial): the landmarks' back-substitution
// first, from the role-0 state into the role's state.  The host driver keeps one error buffer (both ErrBufs eb(0)).
static omv_status launch_errors(omv_lba *h, const State &s0, const State &s1, const LmCtl *ctl, int gate, int role,
                                LmReset reset = LmReset{}, bool init_partials = false, const double *xp = nullptr,
                                double lambda = 0.0, bool one_buffer = false, int n_acc = 0) {
    const int ng = h->n_mono > 0 || xp ? h->plan.n_lgrp : 0;
    const int lead = xp || h->imu_here ? 1 : 0;
    const int blocks = (ng > 0 ? omv::xcd_grid(ng) : 0) + lead;
    const SharedB &sb = h->sb;
    const ErrTrial T{xp, n_acc % 3 == 2 ? 1 : 0, h->d_bb, lambda, h->d_offV, h->d_offG, h->d_offA, h->n_opt, h->d_e_lkf,
                     h->d_lkf_kf, sb.blk >= 0 ? sb.kf : -1, sb.blk >= 0 ? h->n_kf : h->n_opt, sb.prior_g, sb.prior_a};
    const size_t lds = (3 * (size_t)kGrpLand + 12 * (size_t)kGrpW * h->rig.n_cams) * sizeof(double);
    auto launch = [&](auto kernel, auto kd) {
        kernel<<<blocks, 256, lds, h->stream>>>(ng, lead, h->imu_here ? 1 : 0, h->rig, kd, s0, s1, h->E, h->L, h->R, T,
                                                h->delta_mono, h->dsqr_mono, h->delta_st, h->dsqr_st, h->eb(0),
                                                one_buffer ? h->eb(0) : h->eb(1),
                                                init_partials ? h->d_partial0 : h->d_partial, h->d_scale_partial, h->I,
                                                h->delta_imu, h->dsqr_imu,
                                                init_partials ? h->d_imu_partial0 : h->d_imu_partial, ctl, gate, role,
                                                reset);
    };
    if (blocks > 0) {
        if (h->visual) launch(err_kernel<true>, h->vis);
        else launch(err_kernel<false>, Kind<false>{});
    }
    if (h->imu_here && h->n_imu > kImuLead)   // a whole map: the edges past the lead block's one per thread
        imu_err_rest_kernel<<<1, 256, 0, h->stream>>>(s0, s1, h->I, h->delta_imu, h->dsqr_imu, h->eb(0),
                                                      one_buffer ? h->eb(0) : h->eb(1),
                                                      init_partials ? h->d_imu_partial0 : h->d_imu_partial, ctl, gate, role);
    return hipGetLastError() == hipSuccess ? OMV_OK : OMV_ERR_HIP;
}
static int n_grp_err(const omv_lba *h) { return h->n_mono > 0 ? h->plan.n_lgrp : 0; }
static omv_status lba_errors(omv_lba *h, const State &s) { return launch_errors(h, s, s, nullptr, kGateAlways, 0); }
// the device driver's trial: back-substitution + errors into the trial buffer (role 1)
static omv_status lba_trial_errors(omv_lba *h, const LmCtl *c) {
    return launch_errors(h, h->st[0], h->st[1], c, kGateTrial, 1, LmReset{}, false, h->d_x, 0.0);
}

// In-place SUM over the ranks of a sharded solve (no-op on one rank).
// The collective path runs whenever a communicator was given (omv_lba_set_comm), a single rank included: one RCCL
// rank exercises exactly the multi-rank call sequence (stream order, in-place buffers, host-sync count).
static bool lba_collective(const omv_lba *h) { return h->allreduce != nullptr; }
static omv_status lba_allreduce(omv_lba *h, double *buf, size_t n) {
    if (!lba_collective(h)) return OMV_OK;
    HIP_OK(hipGetLastError());
    return h->allreduce(h->ar_ctx, buf, n, (void *)h->stream) == 0 ? OMV_OK : OMV_ERR_HIP;
}

// n_scale counts the update's partials (pose part first); only rank 0 contributes the pose part.
static omv_status lba_read_scalars(omv_lba *h, int n_scale, double out[3], bool with_fail) {
    const int s0 = (h->rank > 0 && n_scale > 0) ? 1 : 0;
    finish_kernel<<<1, 256, 0, h->stream>>>(h->d_partial, n_grp_err(h), h->d_imu_partial,
                                           h->d_scale_partial + s0, n_scale - s0, with_fail ? h->d_fail : nullptr,
                                           h->d_out);
    omv_status rs = lba_allreduce(h, h->d_out, 2);
    if (rs != OMV_OK) return rs;
    HIP_OK(hipMemcpyAsync(h->h_out, h->d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    ++h->host_syncs;
    for (int q = 0; q < 3; ++q) out[q] = h->h_out[q];
    return OMV_OK;
}

// Residuals + Jacobians of the visual edges at the current state, in the caller's order; EdgeMono
// rows go to the mono_* arrays (2 rows), EdgeStereo rows to the stereo_* arrays (3 rows).
static omv_status lba_eval(omv_lba *h, double *mono_err, double *mono_jx, double *mono_jp, double *imu_err,
                           double *st_err, double *st_jx, double *st_jp) {
    if (!h || !has_problem(h)) return OMV_ERR_ARG;
    const State &s = h->st[h->cur];
    omv_status r = lba_errors(h, s);
    if (r != OMV_OK) return r;
    std::vector<double> jx, jp;
    omv::DeviceArena tmp;   // the Jacobians, for this call
    double *d_jx = nullptr, *d_jp = nullptr;
    const int E = h->n_mono;
    const bool jac = mono_jx || mono_jp || st_jx || st_jp;
    if (jac && E > 0) {
        if (!tmp.alloc(&d_jx, 9 * (size_t)E) || !tmp.alloc(&d_jp, 18 * (size_t)E)) return OMV_ERR_HIP;
        if (h->visual)
            vis_jac_kernel<<<(E + 255) / 256, 256, 0, h->stream>>>(h->rig, h->vis, s, h->E, h->d_err, h->d_err3, h->d_chi2,
                                                                   d_jx, d_jp);
        else
            mono_jac_kernel<<<(E + 255) / 256, 256, 0, h->stream>>>(h->rig, s, h->E, d_jx, d_jp);
    }
    HIP_OK(hipStreamSynchronize(h->stream));
    std::vector<double> err(2 * (size_t)E), err3(E), e9(10 * (size_t)h->n_imu);
    if (E > 0) {
        HIP_OK(hipMemcpy(err.data(), h->d_err, err.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(err3.data(), h->d_err3, err3.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (h->imu_here) HIP_OK(hipMemcpy(e9.data(), h->d_err9, e9.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (d_jx) {
        jx.resize(9 * (size_t)E), jp.resize(18 * (size_t)E);
        HIP_OK(hipMemcpy(jx.data(), d_jx, jx.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(jp.data(), d_jp, jp.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    const int EM = h->n_mono_all;
    for (int e = 0; e < E; ++e) {   // back to the caller's edge order
        const int o = h->plan.perm_edge[e];
        if (o < EM) {
            if (mono_err) mono_err[2 * o] = err[2 * e], mono_err[2 * o + 1] = err[2 * e + 1];
            if (mono_jx) std::memcpy(mono_jx + 6 * (size_t)o, &jx[9 * (size_t)e], 48);
            if (mono_jp) std::memcpy(mono_jp + 12 * (size_t)o, &jp[18 * (size_t)e], 96);
        } else {
            const size_t q = (size_t)(o - EM);
            if (st_err) st_err[3 * q] = err[2 * e], st_err[3 * q + 1] = err[2 * e + 1], st_err[3 * q + 2] = err3[e];
            if (st_jx) std::memcpy(st_jx + 9 * q, &jx[9 * (size_t)e], 72);
            if (st_jp) std::memcpy(st_jp + 18 * q, &jp[18 * (size_t)e], 144);
        }
    }
    if (imu_err && h->imu_here) std::memcpy(imu_err, e9.data(), 9 * sizeof(double) * h->n_imu);
    return OMV_OK;
}

extern "C" {

omv_status omv_lba_evaluate(omv_lba *h, double *mono_err, double *mono_jx, double *mono_jp, double *imu_err) {
    return lba_eval(h, mono_err, mono_jx, mono_jp, imu_err, nullptr, nullptr, nullptr);
}

omv_status omv_lba_evaluate_stereo(omv_lba *h, double *stereo_err, double *stereo_jx, double *stereo_jp) {
    return lba_eval(h, nullptr, nullptr, nullptr, nullptr, stereo_err, stereo_jx, stereo_jp);
}

static omv_status lba_finish_result(omv_lba *h, const omv_lba_opts *o, omv_lba_problem *p, omv_lba_result *res);
static bool lba_epilogue_ok(const omv_lba *h);
static omv_status lba_enqueue_epilogue(omv_lba *h, bool want_chi2);

// buildSystem + the landmark Schur complement at state A (the current state; B the other buffer, picked by the control
// block's `cur` on the device driver): the landmark groups and the inertial edges' quadratic forms in one launch, side
// by side (build_all_kernel), then the reduced system assembled per block (assemble_kernel).  Every sum is in a fixed
// order: the system is identical run to run.  lambda enters the landmark groups (R R^T = Hll + lambda I), so both run
// every trial; on a sharded solve lambda enters the pose diagonal once (rank 0), every rank damps its own landmarks.
static omv_status launch_build(omv_lba *h, const State &A, const State &B, const LmCtl *c, double lambda) {
    const int n_imu = h->imu_here ? h->n_imu : 0, n_imu_pad = (n_imu + 7) & ~7;
    const int grid = n_imu_pad + (h->plan.n_lgrp > 0 ? omv::xcd_grid(h->plan.n_lgrp) : 0);
    auto launch = [&](auto all_kernel, auto big_kernel, auto kd) {
        if (grid > 0)
            all_kernel<<<grid, kGrpEdges, kBuildLds, h->stream>>>(
                h->rig, kd, A, B, h->E, h->L, h->plan.n_lgrp, h->I, n_imu, n_imu_pad, lambda, h->delta_mono, h->dsqr_mono,
                h->delta_st, h->dsqr_st, h->delta_imu, h->dsqr_imu, h->eb(0), h->eb(1), h->d_imu_contrib, c);
        if (h->plan.n_big > 0)
            big_kernel<<<h->plan.n_big, kGrpEdges, kBuildLds, h->stream>>>(h->rig, kd, A, B, h->E, h->L, h->d_big,
                                                                      h->plan.n_big, lambda, h->delta_mono, h->dsqr_mono,
                                                                      h->delta_st, h->dsqr_st, h->eb(0), h->eb(1), c);
    };
    if (h->visual) launch(build_all_kernel<true>, build_big_kernel<true>, h->vis);
    else launch(build_all_kernel<false>, build_big_kernel<false>, Kind<false>{});
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

static omv_status launch_assemble(omv_lba *h, const State &A, const State &B, double lambda, const LmCtl *c) {
    SharedB sb = h->sb;   // the priors' gradient reads the current state's pair (A; by the control block's `cur`: A or B)
    sb.bg[0] = A.bg, sb.ba[0] = A.ba, sb.bg[1] = B.bg, sb.ba[1] = B.ba;
    assemble_kernel<<<h->ldlt.pat.n_slots, 256, 0, h->stream>>>(h->G, h->I, h->ldlt.pat, sb, h->L.rec, h->L.rec_rhs, lambda,
                                                          h->rank == 0 ? 1 : 0, h->d_S, h->d_bb, h->d_coef, c);
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

// One LM step of the device driver: the gated kernel sequence (see LmCtl).  The state and error buffers are
// double-buffered: the kernels take both (st[0], st[1]) and pick the current / trial one by the control block's
// `cur`, an accepted trial flips it -- no copy launch, and no recomputation of the current errors after a rejected
// trial.  With `ev`, events bracket the stages (build, Schur, solve, update + errors).
static omv_status lba_step(omv_lba *h, hipEvent_t *ev) {
    hipStream_t st = h->stream;
    LmCtl *c = h->d_ctl;
    const State &A = h->st[0], &B = h->st[1];
    omv_status rs;
    if (ev) HIP_OK(hipEventRecord(ev[0], st));
    if (h->visual) {   // computeLambdaInit at the first step of an optimize() without a user lambda (gated on the device)
        const int nd = h->n_opt + h->plan.n_lgrp;
        vis_diag_kernel<<<nd, 256, 0, st>>>(h->rig, h->vis, A, h->E, h->L, h->n_opt, h->d_kf_edge_start, h->d_kf_edge,
                                            h->eb(0), h->d_diag, c);
        vis_lambda_kernel<<<1, 256, 0, st>>>(h->d_diag, nd, c);
    }
    if ((rs = launch_build(h, A, B, c, 0.0)) != OMV_OK) return rs;
    if (ev) HIP_OK(hipEventRecord(ev[1], st));
    if ((rs = launch_assemble(h, A, B, 0.0, c)) != OMV_OK) return rs;
    // sharded: one in-place SUM of this rank's partial reduced system [blocks | b | Schur rhs], ordered on the stream
    if ((rs = lba_allreduce(h, h->d_S, h->plan.n_reduce)) != OMV_OK) return rs;
    if (ev) HIP_OK(hipEventRecord(ev[2], st));
    h->ldlt.launch(st, h->d_S, h->d_bb, h->d_coef, h->d_x, h->d_scratch, h->d_fail, c);
    if (ev) HIP_OK(hipEventRecord(ev[3], st));
    if ((rs = lba_trial_errors(h, c)) != OMV_OK) return rs;
    const int nmb = n_grp_err(h), nsc = 1 + h->plan.n_lgrp;
    const double *pre = nullptr;
    if (lba_collective(h)) {   // [chi(A), chi, computeScale] of this rank's edges / landmarks, summed over the ranks
        const int s0 = h->rank > 0 ? 1 : 0;   // the keyframe part of computeScale enters once (rank 0)
        trial_scalars_kernel<<<1, 256, 0, st>>>(c, h->d_partial, nmb, h->d_imu_partial, h->d_scale_partial + s0,
                                                nsc - s0, h->d_out, h->d_partial0, h->d_imu_partial0);
        if ((rs = lba_allreduce(h, h->d_out, 3)) != OMV_OK) return rs;
        pre = h->d_out;
    }
    finish_trial_kernel<<<1, 256, 0, st>>>(c, h->d_partial, nmb, h->d_imu_partial, h->d_scale_partial, nsc, h->d_fail,
                                           pre, h->d_partial0, h->d_imu_partial0);
    if (ev) HIP_OK(hipEventRecord(ev[4], st));
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

// optimize() with the LM control on the device: the initial errors, then LM steps in batches (opt_it first: every
// iteration takes at least one trial) until the device reports the end; one read-back per batch (host_syncs counts
// them); the last accepted trial's state copied into A.  Identical decisions to the host-driven loop below.  A
// sharded solve (world > 1) runs the same gated steps launched directly (its two all-reduces per step are calls into
// the caller's collective, ordered on the handle's stream): every rank reaches identical decisions from the
// all-reduced system and scalars, so every rank launches the same steps and collectives.
static omv_status lba_optimize_device(omv_lba *h, const omv_lba_opts *o, omv_lba_result *res) {
    const bool want_chi2 = res->mono_chi2 || res->stereo_chi2;
    h->epi_ready = false;
    hipStream_t st = h->stream;
    if (h->cur != 0) {   // the device path keeps the current state in st[0]
        HIP_OK(hipMemcpyAsync(h->st[0].Rwb, h->st[1].Rwb, h->state_doubles() * sizeof(double), hipMemcpyDeviceToDevice,
                              st));
        h->cur = 0;
    }
    omv_status rs;
    h->host_syncs = 0;
    const int nmb = n_grp_err(h);
    const bool sharded = lba_collective(h);
    if (o->opt_it > 0 && nmb + (h->imu_here ? 1 : 0) > 0) {
        // the initial errors into their own partials, the control block reset by the same launch; the first step's
        // bookkeeping sums the initial chi (through the first all-reduce on a sharded solve)
        if ((rs = launch_errors(h, h->st[0], h->st[0], nullptr, kGateAlways, 0,
                                LmReset{h->d_ctl, o->opt_it, o->max_trials, o->lambda_init}, true)) != OMV_OK)
            return rs;
    } else {
        if ((rs = lba_errors(h, h->st[0])) != OMV_OK) return rs;
        if (sharded) {
            trial_scalars_kernel<<<1, 256, 0, st>>>(nullptr, h->d_partial, nmb, h->d_imu_partial, nullptr, 0, h->d_out,
                                                    nullptr, nullptr);
            if ((rs = lba_allreduce(h, h->d_out, 3)) != OMV_OK) return rs;
        }
        ctl_init_kernel<<<1, 256, 0, st>>>(h->d_ctl, h->d_partial, nmb, h->d_imu_partial, o->opt_it, o->max_trials,
                                           o->lambda_init, sharded ? h->d_out : nullptr);
    }
    HIP_OK(hipGetLastError());
    const bool direct = h->timing || sharded;   // a collective call cannot be captured
    if (!direct && !h->step_exec) {   // capture one step and four steps (the problem's pointers are fixed
                                         // until set_problem); a batch is launched as 4-step graphs + single steps
        for (int n : {1, 4}) {
            HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            for (int q = 0; q < n && rs == OMV_OK; ++q) rs = lba_step(h, nullptr);
            hipGraph_t g = nullptr;
            const hipError_t ce = hipStreamEndCapture(st, &g);
            if (rs != OMV_OK) return rs;
            if (ce != hipSuccess) {
                fprintf(stderr, "omv: LM step capture failed: %s\n", hipGetErrorString(ce));
                return OMV_ERR_HIP;
            }
            (n == 1 ? h->step_graph : h->step4_graph) = g;
            HIP_OK(hipGraphInstantiate(n == 1 ? &h->step_exec : &h->step4_exec, g, nullptr, nullptr, 0));
        }
    }
    // the fused batch: four steps, the epilogue and the read-backs captured together (once per problem and chi2 mode)
    const bool fuse_epi = !direct && lba_epilogue_ok(h);
    const int wc = want_chi2 ? 1 : 0;
    if (fuse_epi && !h->step4e_exec[wc]) {
        HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        rs = OMV_OK;
        for (int q = 0; q < 4 && rs == OMV_OK; ++q) rs = lba_step(h, nullptr);
        if (rs == OMV_OK) rs = lba_enqueue_epilogue(h, want_chi2);
        const hipError_t me = hipMemcpyAsync(h->h_ctl, h->d_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, st);
        hipGraph_t g = nullptr;
        const hipError_t ce = hipStreamEndCapture(st, &g);
        if (rs != OMV_OK) return rs;
        if (ce != hipSuccess || me != hipSuccess) {
            fprintf(stderr, "omv: LM batch capture failed: %s\n", hipGetErrorString(ce != hipSuccess ? ce : me));
            return OMV_ERR_HIP;
        }
        h->step4e_graph[wc] = g;
        HIP_OK(hipGraphInstantiate(&h->step4e_exec[wc], g, nullptr, nullptr, 0));
        h->epi_ready = false;
    }
    const int max_steps = std::max(0, o->opt_it) * std::max(1, o->max_trials);
    std::vector<std::array<hipEvent_t, 5>> evs;
    int launched = 0, batch = std::min(std::max(0, o->opt_it), max_steps);
    while (true) {
        bool fused = false;   // this batch's last launch carried the epilogue and the control read-back
        for (int i = 0; i < batch;) {
            if (h->timing) {
                std::array<hipEvent_t, 5> e{};
                for (auto &x : e) HIP_OK(hipEventCreate(&x));
                evs.push_back(e);
                if ((rs = lba_step(h, evs.back().data())) != OMV_OK) return rs;
                ++i;
            } else if (direct) {
                if ((rs = lba_step(h, nullptr)) != OMV_OK) return rs;
                ++i;
            } else if (i + 4 <= batch) {
                fused = fuse_epi && i + 4 == batch;
                HIP_OK(hipGraphLaunch(fused ? h->step4e_exec[wc] : h->step4_exec, st));
                i += 4;
            } else {
                HIP_OK(hipGraphLaunch(h->step_exec, st));
                ++i;
            }
        }
        launched += batch;
        // the epilogue rides along with the control read-back (kept when the device reports the end)
        if (fused) {
            h->epi_ready = true, h->epi_chi2 = want_chi2;
        } else {
            const bool spec = lba_epilogue_ok(h);
            if (spec && (rs = lba_enqueue_epilogue(h, want_chi2)) != OMV_OK) return rs;
            HIP_OK(hipMemcpyAsync(h->h_ctl, h->d_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipStreamSynchronize(st));
        ++h->host_syncs;
        if (h->h_ctl->done || launched >= max_steps) break;
        h->epi_ready = false;
        batch = std::min(4, max_steps - launched);
    }
    if (!h->epi_ready) {   // the last accepted trial's state into A
        cur_copy_kernel<<<64, 256, 0, st>>>(h->d_ctl, h->st[1].Rwb, h->st[0].Rwb, h->state_doubles());
        HIP_OK(hipGetLastError());
    }
    const LmCtl &c = *h->h_ctl;
    for (double &m : h->stage_ms) m = 0;
    for (auto &e : evs) {
        float ms;
        for (int k = 0; k < 4; ++k) {
            HIP_OK(hipEventElapsedTime(&ms, e[k], e[k + 1]));
            h->stage_ms[k] += ms;
        }
        for (auto &x : e) (void)hipEventDestroy(x);
    }
    h->last_trials = c.trials;
    res->err = (float)c.err0;
    res->err_end = (float)c.errors_chi;
    res->iterations = c.its;
    res->trials = c.trials;
    res->lambda = c.lm.lambda;
    return OMV_OK;
}

omv_status omv_lba_optimize(omv_lba *h, const omv_lba_opts *o, omv_lba_problem *p, omv_lba_result *res) {
    if (!h || !o || !p || !res || !has_problem(h)) return OMV_ERR_ARG;
    hipStream_t st = h->stream;
    double sc[3];
    omv_status rs;
    for (double &m : h->stage_ms) m = 0;
    h->host_syncs = 0;
    if (!h->host_lm) {
        if ((rs = lba_optimize_device(h, o, res)) != OMV_OK) return rs;
        return lba_finish_result(h, o, p, res);
    }
    // err = activeRobustChi2 at the initial state (Optimizer.cc:3273-3274)
    if ((rs = lba_errors(h, h->st[h->cur])) != OMV_OK) return rs;
    if ((rs = lba_read_scalars(h, 0, sc, false)) != OMV_OK) return rs;
    res->err = (float)sc[0];
    double errors_chi = sc[0];
    bool errors_of_current = true;
    omv_lm::LmState lm{0.0, 2.0, 0.0, 0.0, 0, 0};
    int trials = 0, its = 0, n_acc = 0;   // n_acc: accepted updates (ImuCamPose::its, see LmCtl)
    for (int it = 0; it < o->opt_it; ++it) {
        ++its;
        State &A = h->st[h->cur];
        State &B = h->st[1 - h->cur];
        if (!errors_of_current) {
            if ((rs = lba_errors(h, A)) != OMV_OK) return rs;
            if ((rs = lba_read_scalars(h, 0, sc, false)) != OMV_OK) return rs;
            errors_chi = sc[0];
            errors_of_current = true;
        }
        omv_lm::lm_begin_iteration(lm, it, errors_chi, o->lambda_init);
        omv_lm::LmNext next;
        float ms;
        do {
            // buildSystem + the landmark Schur complement at this trial's lambda (a retry rebuilds at the same state; this
            // driver has one error buffer, which the rejected trial overwrote: the current state's errors first)
            if (lm.qmax > 0 && (rs = lba_errors(h, A)) != OMV_OK) return rs;
            HIP_OK(hipEventRecord(h->ev[0], st));
            if ((rs = launch_build(h, A, A, nullptr, lm.lambda)) != OMV_OK) return rs;
            HIP_OK(hipEventRecord(h->ev[1], st));
            HIP_OK(hipEventRecord(h->ev[2], st));
            if ((rs = launch_assemble(h, A, A, lm.lambda, nullptr)) != OMV_OK) return rs;
            // one exchange: sum the partial reduced systems [blocks | b | Schur rhs] of the landmark shards
            if ((rs = lba_allreduce(h, h->d_S, h->plan.n_reduce)) != OMV_OK) return rs;
            HIP_OK(hipEventRecord(h->ev[3], st));
            h->ldlt.launch(st, h->d_S, h->d_bb, h->d_coef, h->d_x, h->d_scratch, h->d_fail, nullptr);
            HIP_OK(hipEventRecord(h->ev[4], st));
            // the keyframe update and the landmarks' back-substitution A -> B, the trial's errors (one launch, this
            // driver's one error buffer)
            if ((rs = launch_errors(h, A, B, nullptr, kGateAlways, 1, LmReset{}, false, h->d_x, lm.lambda, true, n_acc)) !=
                OMV_OK)
                return rs;
            if ((rs = lba_read_scalars(h, 1 + h->plan.n_lgrp, sc, true)) != OMV_OK) return rs;
            const int fail = sc[2] != 0.0;
            HIP_OK(hipEventRecord(h->ev[5], st));
            HIP_OK(hipEventSynchronize(h->ev[5]));
            HIP_OK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
            h->stage_ms[0] += ms;
            HIP_OK(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
            h->stage_ms[1] += ms;
            HIP_OK(hipEventElapsedTime(&ms, h->ev[3], h->ev[4]));
            h->stage_ms[2] += ms;
            HIP_OK(hipEventElapsedTime(&ms, h->ev[4], h->ev[5]));
            h->stage_ms[3] += ms;
            const bool ok = fail == 0;
            errors_chi = sc[0];
            errors_of_current = false;   // the last computed errors belong to the trial state
            const omv_lm::LmTrial tr = omv_lm::lm_trial(lm, sc[0], ok, ok ? sc[1] : 0.0);   // a failed solve: no scale
            ++trials;
            if (tr.accepted) {
                ++n_acc;
                // fixed keyframes are identical in both buffers; make B the current state
                h->cur = 1 - h->cur;
                errors_of_current = true;
                // the next trial rewrites every optimisable keyframe and every point of the other buffer
            }
            next = omv_lm::lm_next(lm, tr.rho, o->max_trials);
        } while (next == omv_lm::kLmTrial);
        if (next == omv_lm::kLmStop) break;
    }
    h->last_trials = trials;
    res->err_end = (float)errors_chi;
    res->iterations = its;
    res->trials = trials;
    res->lambda = lm.lambda;
    return lba_finish_result(h, o, p, res);
}

// The epilogue shared by both LM drivers: state write-back in the caller's order, per-edge chi2 and the
// reference's outlier / FAIL tests (Optimizer.cc:3282-3321).
// The single-rank device epilogue: state of A (an accepted last trial copied in first), outlier flags, chi2 when
// asked for and the points in the caller's order into the staging block [head | points | flags | chi2], then
// its read-back into pinned memory (not synchronised here).
static bool lba_epilogue_ok(const omv_lba *h) {
    return h->world == 1 && h->d_stage && h->cur == 0 && h->n_mono_all + h->n_stereo_all == h->n_mono;
}
static omv_status lba_enqueue_epilogue(omv_lba *h, bool want_chi2) {
    hipStream_t st = h->stream;
    const State &s = h->st[0];
    const int P = h->n_pts, E = h->n_mono;
    const StageLayout L = h->stage();
    const size_t head = L.head;
    double *d_pts = h->d_stage + L.pts(), *d_chi2 = h->d_stage + L.chi2();
    uint8_t *d_flags = (uint8_t *)(h->d_stage + L.flags());
    const int n = std::max(std::max(E, P), (int)head);
    auto launch = [&](auto kernel) {
        kernel<<<(n + 255) / 256, 256, 0, st>>>(h->rig, s, h->st[1], h->state_doubles(), h->E, h->d_perm_edge,
                                                h->n_mono_all, h->d_track_depth, h->d_perm_pt, P, d_flags,
                                                want_chi2 ? d_chi2 : nullptr, d_pts, h->d_chi2, h->d_chi2_b,
                                                h->host_lm ? nullptr : h->d_ctl, h->d_stage, (int)head);
    };
    if (h->visual) launch(epilogue_kernel<true>);
    else launch(epilogue_kernel<false>);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h->h_stage, h->d_stage, L.bytes(want_chi2), hipMemcpyDeviceToHost, st));
    h->epi_ready = true, h->epi_chi2 = want_chi2;
    return OMV_OK;
}
// The pinned staging block holds this optimize()'s result, with the chi2 when wanted: already in flight with the LM
// control's last read-back when the device driver ran, else enqueued and waited for here.
static omv_status lba_await_epilogue(omv_lba *h, bool want_chi2) {
    if (!h->epi_ready || (want_chi2 && !h->epi_chi2)) {
        const omv_status rs = lba_enqueue_epilogue(h, want_chi2);
        if (rs != OMV_OK) return rs;
        HIP_OK(hipStreamSynchronize(h->stream));
    }
    h->epi_ready = false;
    return OMV_OK;
}
// The points and the per-edge results a caller asked for (null: not wanted) out of the pinned block.
static void take_staged(const omv_lba *h, double *pts, double *mono_chi2, double *stereo_chi2, uint8_t *mono_outlier,
                        uint8_t *stereo_outlier) {
    const StageLayout L = h->stage();
    const double *hs = h->h_stage, *hc = hs + L.chi2();
    const uint8_t *hf = (const uint8_t *)(hs + L.flags());
    const size_t EM = h->n_mono_all, ES = h->n_stereo_all;
    if (L.P > 0) std::memcpy(pts, hs + L.pts(), 3 * sizeof(double) * L.P);
    if (mono_chi2) std::memcpy(mono_chi2, hc, sizeof(double) * EM);
    if (stereo_chi2) std::memcpy(stereo_chi2, hc + EM, sizeof(double) * ES);
    if (mono_outlier) std::memcpy(mono_outlier, hf, EM);
    if (stereo_outlier) std::memcpy(stereo_outlier, hf + EM, ES);
}

static omv_status lba_finish_result(omv_lba *h, const omv_lba_opts *o, omv_lba_problem *p, omv_lba_result *res) {
    hipStream_t st = h->stream;
    const State &s = h->st[h->cur];
    const int K = h->n_kf, C = h->rig.n_cams, P = h->n_pts, E = h->n_mono;
    const bool fail = (2 * res->err < res->err_end || std::isnan(res->err) || std::isnan(res->err_end)) && !o->large;
    res->status = fail ? OMV_LBA_FAIL : OMV_LBA_OK;
    auto take_head = [&](const double *q) {
        auto take = [&](double *dst, size_t n) {
            std::memcpy(dst, q, n * sizeof(double));
            q += n;
        };
        take(p->Rwb, 9 * (size_t)K), take(p->twb, 3 * (size_t)K), take(p->Rcw, 9 * (size_t)K * C);
        take(p->tcw, 3 * (size_t)K * C), take(p->vel, 3 * (size_t)K), take(p->bg, 3 * (size_t)K), take(p->ba, 3 * (size_t)K);
    };
    if (lba_epilogue_ok(h)) {
        // device epilogue: outlier flags / chi2 / points in the caller's order, one staging read-back (already in
        // flight with the LM control's last read-back when the device driver ran)
        const omv_status rs = lba_await_epilogue(h, res->mono_chi2 || res->stereo_chi2);
        if (rs != OMV_OK) return rs;
        take_head(h->h_stage);
        take_staged(h, p->pts, res->mono_chi2, res->stereo_chi2, res->mono_outlier, res->stereo_outlier);
        return OMV_OK;
    }
    // sharded rank: this rank's landmarks and edges only, on the host
    std::vector<double> stg(h->state_doubles()), chi2(E);
    HIP_OK(hipMemcpyAsync(stg.data(), s.Rwb, stg.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    // the last computed errors: buffer `last` of the device driver's control block (the host driver uses the first)
    const double *d_last_chi2 = (!h->host_lm && h->h_ctl && h->h_ctl->last) ? h->d_chi2_b : h->d_chi2;
    if (E > 0) HIP_OK(hipMemcpyAsync(chi2.data(), d_last_chi2, sizeof(double) * E, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    take_head(stg.data());
    {
        const double *q = stg.data() + (s.pts - s.Rwb);
        for (int i = 0; i < P; ++i)
            for (int d = 0; d < 3; ++d) p->pts[3 * (size_t)h->plan.order[i] + d] = q[3 * (size_t)i + d];
    }
    for (int e = 0; e < E; ++e) {
        const int oe = h->plan.perm_edge[e];
        if (oe >= h->n_mono_all) {   // EdgeStereo: chi2 > chi2Stereo2 (:3299-3311)
            const int q = oe - h->n_mono_all;
            if (res->stereo_chi2) res->stereo_chi2[q] = chi2[e];
            if (res->stereo_outlier) res->stereo_outlier[q] = chi2[e] > 7.815f ? 1 : 0;
            continue;
        }
        if (res->mono_chi2) res->mono_chi2[oe] = chi2[e];
        if (res->mono_outlier) {
            const int k = p->mono_kf[oe], c = p->mono_cam[oe], pt = p->mono_pt[oe];
            const double *R = p->Rcw + ((size_t)k * C + c) * 9, *t = p->tcw + ((size_t)k * C + c) * 3;
            const double *X = p->pts + 3 * (size_t)pt;
            const bool depth_pos = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]) > 0.0;
            const bool close = p->pt_track_depth[pt] < 10.f;
            const double c2 = chi2[e];
            res->mono_outlier[oe] = ((c2 > 5.991f && !close) || (c2 > 1.5f * 5.991f && close) || !depth_pos) ? 1 : 0;
        }
    }
    return OMV_OK;
}

omv_status omv_lba_reset(omv_lba *h) {
    if (!h || !has_problem(h)) return OMV_ERR_ARG;
    return restore_uploaded_state(h);
}

omv_status omv_lba_set_comm(omv_lba *h, int rank, int world, omv_allreduce_fn allreduce, void *ctx) {
    if (!h || world < 1 || rank < 0 || rank >= world || (world > 1 && !allreduce)) return OMV_ERR_ARG;
    if (h->visual || h->fiba) return OMV_ERR_ARG;   // the visual and the full inertial kinds are single-rank
    h->rank = rank, h->world = world, h->allreduce = allreduce, h->ar_ctx = ctx;
    return OMV_OK;
}

omv_status omv_lba_shard(omv_lba *h, int32_t *n_pts, int32_t *n_mono, int32_t *pt_index) {
    if (!h) return OMV_ERR_ARG;
    if (n_pts) *n_pts = h->n_pts;
    if (n_mono) *n_mono = h->n_mono;
    if (pt_index) std::copy(h->plan.order.begin(), h->plan.order.end(), pt_index);
    return OMV_OK;
}

omv_status omv_lba_enable_timing(omv_lba *h, int on) {
    if (!h) return OMV_ERR_ARG;
    h->timing = on != 0;
    return OMV_OK;
}

omv_status omv_lba_set_driver(omv_lba *h, int host_driven) {
    if (!h) return OMV_ERR_ARG;
    h->host_lm = host_driven != 0;
    return OMV_OK;
}

omv_status omv_lba_host_syncs(omv_lba *h, int *host_syncs, int *trials) {
    if (!h) return OMV_ERR_ARG;
    if (host_syncs) *host_syncs = h->host_syncs;
    if (trials) *trials = h->last_trials;
    return OMV_OK;
}

omv_status omv_lba_stage_ms(omv_lba *h, double *ms4, int *trials) {
    if (!h || !ms4) return OMV_ERR_ARG;
    for (int k = 0; k < 4; ++k) ms4[k] = h->stage_ms[k];
    if (trials) *trials = h->last_trials;
    return OMV_OK;
}

}  // extern "C"

// ---- test hooks: the solver's 16x16 inverse alone, and one reduced-system solve read back ---------------------
__global__ void __launch_bounds__(64) selftest_inv16_kernel(const double *D, double *Dinv, int32_t *bad) {
    __shared__ double Ds[256];
    __shared__ int flag;
    const int p = blockIdx.x, lane = threadIdx.x;
    for (int q = lane; q < 256; q += 64) Ds[q] = D[(size_t)p * 256 + q];
    if (lane == 0) flag = 0;
    wave_sync<0>();
    inv16<0>(Ds, lane, &flag);
    for (int q = lane; q < 256; q += 64) Dinv[(size_t)p * 256 + q] = Ds[q];
    if (lane == 0) bad[p] = flag;
}

extern "C" {

omv_status omv_selftest_inv16(int batch, const double *D, double *Dinv, int32_t *bad, void *stream) {
    if (batch < 0 || (batch > 0 && (!D || !Dinv || !bad))) return OMV_ERR_ARG;
    if (batch == 0) return OMV_OK;
    selftest_inv16_kernel<<<batch, 64, 0, (hipStream_t)stream>>>(D, Dinv, bad);
    HIP_OK(hipGetLastError());
    return OMV_OK;
}

omv_status omv_lba_debug_solve(omv_lba *h, const omv_lba_opts *o, double lambda, double *S, double *rhs, double *x,
                               int32_t *fail, int32_t *plan, int plan_cap) {
    if (!h || !o || !S || !rhs || !x || !fail || !plan || !(lambda > 0.0) || !std::isfinite(lambda)) return OMV_ERR_ARG;
    const BlockPat &B = h->ldlt.pat;
    const int n = 16 * B.nb;
    if (!has_problem(h) || h->world != 1 || plan_cap < 4 + B.n_lev) return OMV_ERR_ARG;
    const State &A = h->st[h->cur];
    omv_status rs;
    if ((rs = lba_errors(h, A)) != OMV_OK) return rs;
    if ((rs = launch_build(h, A, A, nullptr, lambda)) != OMV_OK) return rs;
    if ((rs = launch_assemble(h, A, A, lambda, nullptr)) != OMV_OK) return rs;
    h->ldlt.launch(h->stream, h->d_S, h->d_bb, h->d_coef, h->d_x, h->d_scratch, h->d_fail, nullptr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(h->stream));
    std::vector<double> bb(n), coef(n);
    HIP_OK(hipMemcpy(bb.data(), h->d_bb, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(coef.data(), h->d_coef, n * sizeof(double), hipMemcpyDeviceToHost));
    for (int q = 0; q < n; ++q) rhs[q] = bb[q] - coef[q];
    return h->ldlt.read_solved(h->plan, h->d_S, h->d_x, h->d_fail, S, x, fail, plan);
}

}  // extern "C"

// ---- omv_vba: the visual kind's C ABI ------------------------------------------------------------------------------
// An omv_vba is an omv_lba created with `visual`: the plan, the arena, the LM driver, the captured steps and the
// epilogue are the inertial handle's; what follows translates the problem, uploads the kind's own few arrays and reads
// the result in its own layout.
static omv_lba *core(omv_vba *h) { return reinterpret_cast<omv_lba *>(h); }

// The visual problem as the planner's input: the same edges, no inertial edge, 6-row keyframe blocks only; q in the
// first four doubles of the keyframe's Rwb slot, t in twb, the per-camera poses left for vis_cams_kernel.
struct VbaTranslated {
    std::vector<double> Rcb, tcb, Rbc, tbc, Rwb, Rcw, tcw, zero3;
    std::vector<uint8_t> kf_imu;
    omv_lba_problem lp{};
};
static void vba_translate(const omv_vba_problem &p, VbaTranslated &t) {
    const size_t C = p.n_cams, K = p.n_kf;
    t.Rcb.assign(9 * C, 0.0), t.tcb.assign(p.t_c0, p.t_c0 + 3 * C), t.Rbc.assign(9 * C, 0.0), t.tbc.assign(3 * C, 0.0);
    for (size_t c = 0; c < C; ++c) {
        double *R = &t.Rcb[9 * c], *Rt = &t.Rbc[9 * c];
        q_to_mat(p.q_c0 + 4 * c, R);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = R[3 * j + i];
        for (int i = 0; i < 3; ++i)
            t.tbc[3 * c + i] = -(Rt[3 * i] * t.tcb[3 * c] + Rt[3 * i + 1] * t.tcb[3 * c + 1] + Rt[3 * i + 2] * t.tcb[3 * c + 2]);
    }
    t.Rwb.assign(9 * K, 0.0), t.Rcw.assign(9 * K * C, 0.0), t.tcw.assign(3 * K * C, 0.0), t.zero3.assign(3 * K, 0.0);
    for (size_t k = 0; k < K; ++k) std::copy(p.q_cw + 4 * k, p.q_cw + 4 * k + 4, &t.Rwb[9 * k]);
    t.kf_imu.assign(K, 0);
    omv_lba_problem &lp = t.lp;
    lp.n_cams = p.n_cams, lp.cam = p.cam, lp.cam_model = p.cam_model;
    lp.Rcb = t.Rcb.data(), lp.tcb = t.tcb.data(), lp.Rbc = t.Rbc.data(), lp.tbc = t.tbc.data();
    lp.n_kf = p.n_kf, lp.n_opt = p.n_opt, lp.kf_imu = t.kf_imu.data();
    lp.Rwb = t.Rwb.data(), lp.twb = p.t_cw, lp.Rcw = t.Rcw.data(), lp.tcw = t.tcw.data();
    lp.vel = lp.bg = lp.ba = t.zero3.data();
    lp.n_pts = p.n_pts, lp.pts = p.pts, lp.pt_track_depth = nullptr;
    lp.n_mono = p.n_mono, lp.mono_pt = p.mono_pt, lp.mono_kf = p.mono_kf, lp.mono_cam = p.mono_cam;
    lp.mono_obs = p.mono_obs, lp.mono_inv_sigma2 = p.mono_inv_sigma2;
    lp.n_imu = 0;
    lp.n_stereo = p.n_stereo, lp.stereo_pt = p.stereo_pt, lp.stereo_kf = p.stereo_kf, lp.stereo_obs = p.stereo_obs;
    lp.stereo_inv_sigma2 = p.stereo_inv_sigma2, lp.bf = (float)p.bf;
}

// The kind's own device arrays after upload_problem: Huber deltas, levels (all active), the keyframes' edge lists for
// computeLambdaInit, and every keyframe's per-camera pose derived on the device into all three state buffers.
static omv_status vba_upload(omv_lba *h, const omv_vba_problem *p) {
    const LbaPlan &pl = h->plan;
    const int E = h->n_mono, nb = h->n_opt;
    std::vector<int> start(nb + 1, 0), list;
    for (int e = 0; e < E; ++e)
        if (pl.e_kf[e] < nb) ++start[pl.e_kf[e] + 1];
    for (int k = 0; k < nb; ++k) start[k + 1] += start[k];
    list.resize(start[nb]);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int e = 0; e < E; ++e)
            if (pl.e_kf[e] < nb) list[at[pl.e_kf[e]]++] = e;
    }
    omv::DeviceArena &mem = h->prob;
    if (!mem.alloc(&h->d_huber, 2) || !mem.alloc(&h->d_level, (size_t)E) || !mem.alloc(&h->d_diag, (size_t)nb + pl.n_lgrp) ||
        !mem.alloc(&h->d_kf_edge_start, start.size()) || !mem.alloc(&h->d_kf_edge, list.size()))
        return OMV_ERR_HIP;
    HIP_OK(hipMemset(h->d_level, 0, std::max(E, 1)));
    HIP_OK(hipMemset(h->d_huber, 0, 2 * sizeof(double)));
    HIP_OK(hipMemcpy(h->d_kf_edge_start, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!list.empty()) HIP_OK(hipMemcpy(h->d_kf_edge, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice));
    Kind<true> &v = h->vis;
    for (int c = 0; c < p->n_cams; ++c)
        for (int q = 0; q < 4; ++q) v.qc0[c][q] = p->q_c0[4 * c + q];
    v.fx = p->fx, v.fy = p->fy, v.cx = p->cx, v.cy = p->cy, v.bf = p->bf;
    v.huber = h->d_huber, v.level = h->d_level;
    const int n = h->n_kf * p->n_cams;
    vis_cams_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(h->rig, v, h->st[2], h->n_kf);
    HIP_OK(hipGetLastError());
    return restore_uploaded_state(h);
}

static omv_status vba_set_huber(omv_lba *h, const omv_vba_opts *o) {
    if (!(o->huber_mono >= 0.0) || !(o->huber_stereo >= 0.0)) return OMV_ERR_ARG;
    const double d[2] = {o->huber_mono, o->huber_stereo};
    HIP_OK(hipMemcpyAsync(h->d_huber, d, sizeof d, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));   // `d` is this frame's
    return OMV_OK;
}

extern "C" {

omv_status omv_vba_create(int max_kf, int max_cams, int max_pts, int max_edges, omv_vba **out) {
    if (!out) return OMV_ERR_ARG;
    omv_lba *h = nullptr;
    const omv_status rs = omv_lba_create(max_kf, max_cams, max_pts, max_edges, 0, &h);
    if (rs != OMV_OK) return rs;
    h->visual = true;
    *out = reinterpret_cast<omv_vba *>(h);
    return OMV_OK;
}

omv_status omv_vba_destroy(omv_vba *h) { return omv_lba_destroy(core(h)); }

omv_status omv_vba_set_problem(omv_vba *hv, const omv_vba_problem *p) {
    omv_lba *h = core(hv);
    if (!h || !h->visual || !p || p->n_cams < 1 || p->n_kf < 1 || p->n_opt < 1 || p->n_opt > p->n_kf || p->n_pts < 0 ||
        p->n_mono < 0 || p->n_stereo < 0 || !p->cam || !p->q_c0 || !p->t_c0 || !p->q_cw || !p->t_cw ||
        (p->n_pts > 0 && !p->pts) ||
        (p->n_mono > 0 && (!p->mono_pt || !p->mono_kf || !p->mono_cam || !p->mono_obs || !p->mono_inv_sigma2)))
        return OMV_ERR_ARG;
    if (p->n_kf > h->max_kf || p->n_cams > h->max_cams || p->n_pts > h->max_pts ||
        (long long)p->n_mono + p->n_stereo > h->max_mono)
        return OMV_ERR_CAPACITY;
    VbaTranslated t;
    vba_translate(*p, t);
    LbaPlan plan;
    const LbaLimits lim{h->max_kf, h->max_cams, h->max_pts, h->max_mono, h->max_imu};
    const omv_status planned = plan_lba(t.lp, 0, 1, lim, h->lds_ok, plan);
    if (planned != OMV_OK) return planned;
    free_problem(h);
    h->plan = std::move(plan);
    omv_status rs = upload_problem(h, &t.lp);
    if (rs == OMV_OK) rs = vba_upload(h, p);
    if (rs != OMV_OK) free_problem(h);
    return rs;
}

omv_status omv_vba_set_levels(omv_vba *hv, const uint8_t *mono_level, const uint8_t *stereo_level) {
    omv_lba *h = core(hv);
    if (!h || !h->visual || !has_problem(h)) return OMV_ERR_ARG;
    const int E = h->n_mono, EM = h->n_mono_all;
    std::vector<uint8_t> lv(std::max(E, 1), 0);
    for (int e = 0; e < E; ++e) {
        const int o = h->plan.perm_edge[e];
        const uint8_t *src = o < EM ? mono_level : stereo_level;
        lv[e] = src && src[o < EM ? o : o - EM] ? 1 : 0;
    }
    HIP_OK(hipMemcpy(h->d_level, lv.data(), E, hipMemcpyHostToDevice));
    return OMV_OK;
}

omv_status omv_vba_optimize(omv_vba *hv, const omv_vba_opts *o, omv_vba_problem *p, omv_vba_result *r) {
    omv_lba *h = core(hv);
    if (!h || !h->visual || !o || !p || !r || !has_problem(h) || o->max_trials < 1 || !p->q_cw || !p->t_cw ||
        (h->n_pts > 0 && !p->pts) || p->n_kf != h->n_kf || p->n_pts != h->n_pts)
        return OMV_ERR_ARG;
    omv_status rs = vba_set_huber(h, o);
    if (rs != OMV_OK) return rs;
    const omv_lba_opts lo{o->iterations, o->lambda_init, o->max_trials, 1};
    omv_lba_result lr{};
    lr.mono_chi2 = r->mono_chi2, lr.stereo_chi2 = r->stereo_chi2;
    for (double &m : h->stage_ms) m = 0;
    if ((rs = lba_optimize_device(h, &lo, &lr)) != OMV_OK) return rs;
    const LmCtl &c = *h->h_ctl;
    r->err = c.err0, r->err_end = c.errors_chi, r->iterations = c.its, r->trials = c.trials, r->lambda = c.lm.lambda;
    r->lambda_init = c.lambda_init;
    // the epilogue's staging block: q in the keyframe's Rwb slot and t in twb (vba_translate), then the shared part
    if (!lba_epilogue_ok(h)) return OMV_ERR_HIP;
    if ((rs = lba_await_epilogue(h, r->mono_chi2 || r->stereo_chi2)) != OMV_OK) return rs;
    const int K = h->n_kf;
    const double *hs = h->h_stage;
    for (int k = 0; k < K; ++k) {
        std::memcpy(p->q_cw + 4 * (size_t)k, hs + 9 * (size_t)k, 4 * sizeof(double));
        std::memcpy(p->t_cw + 3 * (size_t)k, hs + 9 * (size_t)K + 3 * (size_t)k, 3 * sizeof(double));
    }
    take_staged(h, p->pts, r->mono_chi2, r->stereo_chi2, r->mono_outlier, r->stereo_outlier);
    return OMV_OK;
}

omv_status omv_vba_evaluate(omv_vba *hv, const omv_vba_opts *o, double *mono_err, double *mono_jxi, double *mono_jxj,
                            double *stereo_err, double *stereo_jxi, double *stereo_jxj) {
    omv_lba *h = core(hv);
    if (!h || !h->visual || !o || !has_problem(h)) return OMV_ERR_ARG;
    const omv_status rs = vba_set_huber(h, o);
    if (rs != OMV_OK) return rs;
    return lba_eval(h, mono_err, mono_jxi, mono_jxj, nullptr, stereo_err, stereo_jxi, stereo_jxj);
}

omv_status omv_vba_reset(omv_vba *hv) {
    omv_lba *h = core(hv);
    if (!h || !h->visual) return OMV_ERR_ARG;
    return omv_lba_reset(h);
}

omv_status omv_vba_debug_solve(omv_vba *hv, const omv_vba_opts *o, double lambda, double *S, double *rhs, double *x,
                               int32_t *fail, int32_t *plan, int plan_cap) {
    omv_lba *h = core(hv);
    if (!h || !h->visual || !o || !has_problem(h)) return OMV_ERR_ARG;
    const omv_status rs = vba_set_huber(h, o);
    if (rs != OMV_OK) return rs;
    const omv_lba_opts lo{o->iterations, o->lambda_init, o->max_trials, 1};
    return omv_lba_debug_solve(h, &lo, lambda, S, rhs, x, fail, plan, plan_cap);
}

omv_status omv_vba_enable_timing(omv_vba *hv, int on) { return omv_lba_enable_timing(core(hv), on); }
omv_status omv_vba_stage_ms(omv_vba *hv, double *ms4, int *trials) { return omv_lba_stage_ms(core(hv), ms4, trials); }

}  // extern "C"

// ---- omv_fiba: the full inertial kind's C ABI (Optimizer::FullInertialBA, src/Optimizer.cc:368-853) ---------------------
// An omv_fiba is an omv_lba created with `fiba`: the inertial kind's kernels, plan, LM driver and epilogue; what follows
// translates the problem (which edges are in the graph, the robust kernels, the shared pair's value), plans it with
// plan_fiba and reads the result in its own layout.  Single rank: there is no set_comm.
static omv_lba *core(omv_fiba *h) { return reinterpret_cast<omv_lba *>(h); }

struct FibaTranslated {
    std::vector<int32_t> mono_pt, mono_kf, mono_cam, stereo_pt, stereo_kf;
    std::vector<double> mono_obs, stereo_obs, bg, ba;
    std::vector<float> mono_w, stereo_w;
    std::vector<uint8_t> robust;
    std::vector<int> mono_map, stereo_map;   // graph edge -> caller edge
    omv_lba_problem lp{};
};
// OMV_ERR_ARG: what the planner cannot check for itself (it would read through the pointer).
static omv_status fiba_translate(const omv_fiba_problem &fp, FibaTranslated &t) {
    const omv_lba_problem &p = fp.base;
    const int K = p.n_kf, P = p.n_pts, EM = p.n_mono, ES = std::max(p.n_stereo, 0), NI = p.n_imu;
    if (K < 1 || P < 0 || EM < 0 || NI < 0 || p.n_opt < 1 || p.n_opt > K || !p.kf_imu || !p.Rwb || !p.twb || !p.Rcw ||
        !p.tcw || !p.vel || !p.bg || !p.ba || (P > 0 && !p.pts) || !p.cam || !p.Rcb || !p.tcb || !p.Rbc || !p.tbc ||
        (EM > 0 && (!p.mono_pt || !p.mono_kf || !p.mono_cam || !p.mono_obs || !p.mono_inv_sigma2)) ||
        (ES > 0 && (!p.stereo_pt || !p.stereo_kf || !p.stereo_obs || !p.stereo_inv_sigma2)) ||
        (NI > 0 && (!p.imu_kf1 || !p.imu_kf2 || !p.preint)))
        return OMV_ERR_ARG;
    // A map point all of whose observing keyframes are fixed is removed from the graph with its edges (bAllFixed,
    // :583, :771-774): it keeps its place in the point array (no edge: it does not move), its edges are left out.
    std::vector<uint8_t> free_pt((size_t)P, 0);
    for (int e = 0; e < EM; ++e) {
        if (p.mono_pt[e] < 0 || p.mono_pt[e] >= P || p.mono_kf[e] < 0 || p.mono_kf[e] >= K) return OMV_ERR_ARG;
        if (p.mono_kf[e] < p.n_opt) free_pt[p.mono_pt[e]] = 1;
    }
    for (int e = 0; e < ES; ++e) {
        if (p.stereo_pt[e] < 0 || p.stereo_pt[e] >= P || p.stereo_kf[e] < 0 || p.stereo_kf[e] >= K) return OMV_ERR_ARG;
        if (p.stereo_kf[e] < p.n_opt) free_pt[p.stereo_pt[e]] = 1;
    }
    for (int e = 0; e < EM; ++e) {
        if (!free_pt[p.mono_pt[e]]) continue;
        t.mono_map.push_back(e);
        t.mono_pt.push_back(p.mono_pt[e]), t.mono_kf.push_back(p.mono_kf[e]), t.mono_cam.push_back(p.mono_cam[e]);
        t.mono_obs.push_back(p.mono_obs[2 * (size_t)e]), t.mono_obs.push_back(p.mono_obs[2 * (size_t)e + 1]);
        t.mono_w.push_back(p.mono_inv_sigma2[e]);
    }
    for (int e = 0; e < ES; ++e) {
        if (!free_pt[p.stereo_pt[e]]) continue;
        t.stereo_map.push_back(e);
        t.stereo_pt.push_back(p.stereo_pt[e]), t.stereo_kf.push_back(p.stereo_kf[e]);
        for (int q = 0; q < 3; ++q) t.stereo_obs.push_back(p.stereo_obs[3 * (size_t)e + q]);
        t.stereo_w.push_back(p.stereo_inv_sigma2[e]);
    }
    omv_lba_problem &lp = t.lp = p;
    lp.pt_track_depth = nullptr;
    lp.n_mono = (int)t.mono_map.size();
    lp.mono_pt = t.mono_pt.data(), lp.mono_kf = t.mono_kf.data(), lp.mono_cam = t.mono_cam.data();
    lp.mono_obs = t.mono_obs.data(), lp.mono_inv_sigma2 = t.mono_w.data();
    lp.n_stereo = (int)t.stereo_map.size();
    lp.stereo_pt = t.stereo_pt.data(), lp.stereo_kf = t.stereo_kf.data(), lp.stereo_obs = t.stereo_obs.data();
    lp.stereo_inv_sigma2 = t.stereo_w.data();
    // every EdgeInertial: Huber sqrt(16.92), its information unscaled (:514-516; LocalInertialBA's 1e-2 is not here)
    t.robust.assign((size_t)std::max(NI, 1), 1);
    lp.imu_robust = t.robust.data(), lp.imu_info_scale = nullptr;
    if (fp.shared_bias) {   // the one pair's value in every bImu keyframe (VertexGyroBias(pIncKF), :442-446)
        t.bg.assign(p.bg, p.bg + 3 * (size_t)K), t.ba.assign(p.ba, p.ba + 3 * (size_t)K);
        for (int k = 0; k < K; ++k)
            if (p.kf_imu[k])
                for (int q = 0; q < 3; ++q) t.bg[3 * k + q] = fp.bg0[q], t.ba[3 * k + q] = fp.ba0[q];
        lp.bg = t.bg.data(), lp.ba = t.ba.data();
    }
    return OMV_OK;
}

extern "C" {

omv_status omv_fiba_create(int max_kf, int max_cams, int max_pts, int max_edges, int max_imu, omv_fiba **out) {
    if (!out) return OMV_ERR_ARG;
    omv_lba *h = nullptr;
    const omv_status rs = omv_lba_create(max_kf, max_cams, max_pts, max_edges, max_imu, &h);
    if (rs != OMV_OK) return rs;
    h->fiba = true;
    *out = reinterpret_cast<omv_fiba *>(h);
    return OMV_OK;
}

omv_status omv_fiba_destroy(omv_fiba *h) { return omv_lba_destroy(core(h)); }

omv_status omv_fiba_set_problem(omv_fiba *hf, const omv_fiba_problem *p) {
    omv_lba *h = core(hf);
    if (!h || !h->fiba || !p) return OMV_ERR_ARG;
    FibaTranslated t;
    omv_status rs = fiba_translate(*p, t);
    if (rs != OMV_OK) return rs;
    LbaPlan plan;
    const LbaLimits lim{h->max_kf, h->max_cams, h->max_pts, h->max_mono, h->max_imu};
    rs = plan_fiba(t.lp, p->shared_bias != 0, p->prior_g, p->prior_a, lim, h->lds_ok, plan);
    if (rs != OMV_OK) return rs;
    free_problem(h);
    h->plan = std::move(plan);
    rs = upload_problem(h, &t.lp);
    if (rs != OMV_OK) {
        free_problem(h);
        return rs;
    }
    h->sb.prior_g = p->shared_bias ? p->prior_g : 0.0, h->sb.prior_a = p->shared_bias ? p->prior_a : 0.0;
    h->fiba_mono = std::move(t.mono_map), h->fiba_stereo = std::move(t.stereo_map);
    h->fiba_n_mono = p->base.n_mono, h->fiba_n_stereo = std::max(p->base.n_stereo, 0);
    return OMV_OK;
}

omv_status omv_fiba_optimize(omv_fiba *hf, const omv_fiba_opts *o, omv_fiba_problem *p, omv_fiba_result *r) {
    omv_lba *h = core(hf);
    if (!h || !h->fiba || !o || !p || !r || !has_problem(h) || o->max_trials < 1 || !(o->lambda_init > 0.0) ||
        p->base.n_kf != h->n_kf || p->base.n_pts != h->n_pts || p->base.n_mono != h->fiba_n_mono ||
        std::max(p->base.n_stereo, 0) != h->fiba_n_stereo || !p->base.Rwb || !p->base.twb || !p->base.Rcw ||
        !p->base.tcw || !p->base.vel || !p->base.bg || !p->base.ba || (h->n_pts > 0 && !p->base.pts))
        return OMV_ERR_ARG;
    const omv_lba_opts lo{o->iterations, o->lambda_init, o->max_trials, 1};   // large: no FAIL guard here
    std::vector<double> mc(r->mono_chi2 ? h->fiba_mono.size() + 1 : 0), sc(r->stereo_chi2 ? h->fiba_stereo.size() + 1 : 0);
    omv_lba_result lr{};
    lr.mono_chi2 = r->mono_chi2 ? mc.data() : nullptr, lr.stereo_chi2 = r->stereo_chi2 ? sc.data() : nullptr;
    for (double &m : h->stage_ms) m = 0;
    omv_status rs = lba_optimize_device(h, &lo, &lr);
    if (rs != OMV_OK) return rs;
    const LmCtl &c = *h->h_ctl;
    r->err = c.err0, r->err_end = c.errors_chi, r->iterations = c.its, r->trials = c.trials, r->lambda = c.lm.lambda;
    // the state in the caller's order (every bImu keyframe holds the shared pair: the update wrote it to each) and the
    // chi2 of the graph's edges; no outlier test, no FAIL status: the reference has neither in this function
    if ((rs = lba_finish_result(h, &lo, &p->base, &lr)) != OMV_OK) return rs;
    if (r->mono_chi2) {
        std::fill(r->mono_chi2, r->mono_chi2 + h->fiba_n_mono, 0.0);
        for (size_t e = 0; e < h->fiba_mono.size(); ++e) r->mono_chi2[h->fiba_mono[e]] = mc[e];
    }
    if (r->stereo_chi2) {
        std::fill(r->stereo_chi2, r->stereo_chi2 + h->fiba_n_stereo, 0.0);
        for (size_t e = 0; e < h->fiba_stereo.size(); ++e) r->stereo_chi2[h->fiba_stereo[e]] = sc[e];
    }
    return OMV_OK;
}

omv_status omv_fiba_evaluate(omv_fiba *hf, double *mono_err, double *mono_jx, double *mono_jp, double *imu_err,
                             double *stereo_err, double *stereo_jx, double *stereo_jp, double *prior_err) {
    omv_lba *h = core(hf);
    if (!h || !h->fiba || !has_problem(h)) return OMV_ERR_ARG;
    const size_t EM = h->fiba_mono.size(), ES = h->fiba_stereo.size();
    // the graph's edges, then scattered into the caller's order
    std::vector<double> me(2 * EM + 1), mx(6 * EM + 1), mp(12 * EM + 1), se(3 * ES + 1), sx(9 * ES + 1), sp(18 * ES + 1);
    const omv_status rs = lba_eval(h, me.data(), mx.data(), mp.data(), imu_err, se.data(), sx.data(), sp.data());
    if (rs != OMV_OK) return rs;
    auto scatter = [](double *dst, const std::vector<double> &src, const std::vector<int> &map, int n_all, int w) {
        if (!dst) return;
        std::fill(dst, dst + (size_t)n_all * w, 0.0);
        for (size_t e = 0; e < map.size(); ++e) std::copy(&src[e * w], &src[e * w] + w, dst + (size_t)map[e] * w);
    };
    scatter(mono_err, me, h->fiba_mono, h->fiba_n_mono, 2), scatter(mono_jx, mx, h->fiba_mono, h->fiba_n_mono, 6);
    scatter(mono_jp, mp, h->fiba_mono, h->fiba_n_mono, 12);
    scatter(stereo_err, se, h->fiba_stereo, h->fiba_n_stereo, 3), scatter(stereo_jx, sx, h->fiba_stereo, h->fiba_n_stereo, 9);
    scatter(stereo_jp, sp, h->fiba_stereo, h->fiba_n_stereo, 18);
    if (prior_err) {
        std::fill(prior_err, prior_err + 6, 0.0);
        if (h->sb.blk >= 0) {   // EdgePriorGyro / EdgePriorAcc::computeError: bprior (zero) - the vertex's estimate
            const State &s = h->st[h->cur];
            double b[6];
            HIP_OK(hipMemcpy(b, s.bg + 3 * h->sb.kf, 3 * sizeof(double), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(b + 3, s.ba + 3 * h->sb.kf, 3 * sizeof(double), hipMemcpyDeviceToHost));
            for (int q = 0; q < 6; ++q) prior_err[q] = 0.0 - b[q];
        }
    }
    return OMV_OK;
}

omv_status omv_fiba_reset(omv_fiba *hf) {
    omv_lba *h = core(hf);
    if (!h || !h->fiba) return OMV_ERR_ARG;
    return omv_lba_reset(h);
}

omv_status omv_fiba_debug_solve(omv_fiba *hf, double lambda, double *S, double *rhs, double *x, int32_t *fail,
                                int32_t *plan, int plan_cap) {
    omv_lba *h = core(hf);
    if (!h || !h->fiba || !has_problem(h)) return OMV_ERR_ARG;
    const omv_lba_opts lo{1, 1e-5, 10, 1};   // validated only
    return omv_lba_debug_solve(h, &lo, lambda, S, rhs, x, fail, plan, plan_cap);
}

omv_status omv_fiba_enable_timing(omv_fiba *hf, int on) { return omv_lba_enable_timing(core(hf), on); }
omv_status omv_fiba_stage_ms(omv_fiba *hf, double *ms4, int *trials) { return omv_lba_stage_ms(core(hf), ms4, trials); }

}  // extern "C"
