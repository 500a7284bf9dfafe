// The host-side plan of one LocalInertialBA problem (lba.hip): everything omv_lba_set_problem decides about how the LM
// trial sums and factors, as one value of std::vectors.  plan_lba makes every argument check and reads no handle.
// Nothing here needs the HIP runtime: hipcc compiles this text into the product, the host compiler into the oracle
// library (oracle/lba_plan_host.cpp), where tests/test_lba_plan_cpu.py asserts what the kernels rely on.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <set>
#include <vector>

#include "../../include/omv.h"
#include "omv_inv3.h"

namespace omv_lba_plan {

// the kernels' int2 / int4 records (lba.hip asserts the layouts agree)
struct alignas(8) Int2 { int x, y; };
struct alignas(16) Int4 { int x, y, z, w; };

// ---- the limits the kernels and the plan share --------------------------------------------------------
constexpr int kGrpEdges = 256;   // edges per buildSystem landmark group / pose chunk (one per thread)
constexpr int kGrpLand = 128;    // landmarks per group (one thread each, threads 0..127)
constexpr int kGrpSlots = 128;   // slots per group (one thread each, threads 128..255)
constexpr int kGrpW = 32;        // optimisable keyframes per group (rows of the Schur product: 8 each)
constexpr int kSE = 22;                   // LDS doubles per edge of a group: JP (3 x 6) | w | -W e (3)
constexpr int kLdsE = kSE * kGrpEdges;    // edges; then per slot its 27 diagonal terms; then the MFMA operand panels
constexpr int kPanel = kLdsE / 16;        // operand panels: ceil(w / 2) * kpad <= kPanel (a group-planning bound)
constexpr size_t kLdltLds = 160 * 1024 - 512;   // dynamic LDS of the solver (the static part is one int)
constexpr int kPreintCov = 67;   // offset of the 15 x 15 covariance C in a preintegration record (PreView::C)

// ---- host-side analysis ------------------------------------------------------------------------------
inline void host_inv(std::vector<double> &A, int n) {   // Gauss-Jordan with partial pivoting
    std::vector<double> I(n * n, 0.0);
    for (int i = 0; i < n; ++i) I[i * n + i] = 1;
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[r * n + c]) > std::fabs(A[p * n + c])) p = r;
        if (p != c)
            for (int k = 0; k < n; ++k) std::swap(A[p * n + k], A[c * n + k]), std::swap(I[p * n + k], I[c * n + k]);
        const double d = A[c * n + c];
        for (int k = 0; k < n; ++k) A[c * n + k] /= d, I[c * n + k] /= d;
        for (int r = 0; r < n; ++r)
            if (r != c && A[r * n + c] != 0) {
                const double f = A[r * n + c];
                for (int k = 0; k < n; ++k) A[r * n + k] -= f * A[c * n + k], I[r * n + k] -= f * I[c * n + k];
            }
    }
    A = I;
}
inline void host_sym_eig(std::vector<double> A, int n, std::vector<double> &w, std::vector<double> &V) {
    V.assign(n * n, 0.0);
    for (int i = 0; i < n; ++i) V[i * n + i] = 1;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0, dg = 0;   // converged: off-diagonal mass below 1e-32 of the diagonal's
        for (int p = 0; p < n; ++p) {
            dg += A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        }
        if (off <= 1e-32 * dg || off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0) continue;
                const double th = (A[q * n + q] - A[p * n + p]) / (2 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1));
                const double c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq, A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk, A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq, V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    w.resize(n);
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

// Symbolic block LDL^T of the keyframe adjacency `adj` (nb x nb, symmetric) in the elimination order `perm`
// (position -> keyframe): the filled lower pattern in positions and each position's elimination-tree level
// (leaves 0, a parent above all its children).  Returns the number of levels (the factorisation's critical
// path in diagonal-block steps) and the number of stored blocks.
inline int symbolic_ldlt(int nb, const std::vector<uint8_t> &adj, const std::vector<int> &perm, std::vector<uint8_t> &pat,
                         std::vector<int> &level, int &n_slots) {
    pat.assign((size_t)nb * nb, 0);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j <= i; ++j) pat[(size_t)i * nb + j] = i == j || adj[(size_t)perm[i] * nb + perm[j]];
    for (int k = 0; k < nb; ++k)
        for (int i = k + 1; i < nb; ++i)
            if (pat[(size_t)i * nb + k])
                for (int j = k + 1; j <= i; ++j)
                    if (pat[(size_t)j * nb + k]) pat[(size_t)i * nb + j] = 1;
    level.assign(nb, 0);
    n_slots = 0;
    int top = 0;
    for (int k = 0; k < nb; ++k) {
        for (int i = k; i < nb; ++i) n_slots += pat[(size_t)i * nb + k];
        for (int i = k + 1; i < nb; ++i)
            if (pat[(size_t)i * nb + k]) {   // the parent: the first block below the diagonal
                level[i] = std::max(level[i], level[k] + 1);
                break;
            }
        top = std::max(top, level[k]);
    }
    return nb > 0 ? top + 1 : 0;
}

// The elimination order of the reduced system's keyframe blocks.  Candidates: the keyframe order, and every
// two-way dissection of it -- a cut c, the separator S = the keyframes before c adjacent to one at or after c,
// then [before c minus S, in order] [from c, reversed] [S]: the two sides share no block, so their columns
// factor concurrently, and each side is eliminated away from the separator (no fill beyond it).  The one with
// the fewest elimination-tree levels whose blocks fit `max_slots` wins (ties: fewer blocks, then earlier).
// The solution of the damped system does not depend on the order beyond rounding (SimplicialLDLT's own AMD
// ordering is a different one again, linear_solver_eigen.h:60).
// max_cuts > 0: at most that many cuts are tried, evenly spaced over 1 .. nb - 1 (a whole map's planning time: every
// cut costs one symbolic factorisation); 0 tries every cut.
inline std::vector<int> plan_order(int nb, const std::vector<uint8_t> &adj, int max_slots, int max_cuts = 0) {
    std::vector<int> best(nb);
    std::iota(best.begin(), best.end(), 0);
    std::vector<uint8_t> pat;
    std::vector<int> lev;
    int best_slots = 0;
    int best_h = symbolic_ldlt(nb, adj, best, pat, lev, best_slots);
    const int n_cuts = max_cuts > 0 ? std::min(max_cuts, nb - 1) : nb - 1;
    for (int ci = 0; ci < n_cuts; ++ci) {
        const int cut = n_cuts == nb - 1 ? 1 + ci : 1 + (int)((long long)ci * (nb - 2) / std::max(n_cuts - 1, 1));
        std::vector<int> order, sep;
        for (int v = 0; v < cut; ++v) {
            bool s = false;
            for (int w = cut; w < nb && !s; ++w) s = adj[(size_t)v * nb + w] != 0;
            (s ? sep : order).push_back(v);
        }
        if (sep.size() * 2 > (size_t)nb) continue;
        for (int w = nb - 1; w >= cut; --w) order.push_back(w);
        order.insert(order.end(), sep.begin(), sep.end());
        int ns = 0;
        const int h = symbolic_ldlt(nb, adj, order, pat, lev, ns);
        if (ns > max_slots) continue;
        if (h < best_h || (h == best_h && ns < best_slots)) best = order, best_h = h, best_slots = ns;
    }
    return best;
}

// ---- the plan ----------------------------------------------------------------------------------------
struct LbaLimits { int max_kf, max_cams, max_pts, max_mono, max_imu; };   // the handle's capacities (omv_lba_create)

struct LbaPlan {
    // order: device point -> caller point (this rank's share of the landmark order); perm_edge: device edge -> caller
    // edge (>= the caller's n_mono: EdgeStereo); edges landmark-major, a landmark's by keyframe; slot: (landmark, keyframe)
    std::vector<int> order, perm_edge, e_pt, e_kf, e_cam, e_slot, pt_edge, pt_slot, slot_kf, slot_edge;
    std::vector<double> e_obs, info9, infoG, infoA;   // info*: the inertial / random-walk information per inertial edge
    std::vector<float> e_w, e_ur, track_depth;
    // reduced-system layout: keyframe block k at 16k: pose 0-5, v 6-8, bg 9-11, ba 12-14, pad 15 (-1: none)
    std::vector<int> offP, offV, offG, offA;
    int n_pt_slots = 0, n_red = 0;   // (landmark, keyframe) slots; rows of the reduced system
    // blocks of the reduced system: the optimisable keyframes, then (FullInertialBA's bInit form, plan_fiba) the one
    // VertexGyroBias / VertexAccBias pair every keyframe shares as block `shared_blk` = n_opt (-1: none): rows 9..14 of
    // its 16, the rest padding; `shared_kf`: the first bImu keyframe, where the kernels read the pair's value
    int nb = 0, shared_blk = -1, shared_kf = -1;
    // block pattern (slot_kr / slot_kc: the keyframes of each stored block, column-major in positions) and the level
    // schedule of its LDL^T, also packed into `blob` (16-byte aligned sub-arrays at `off`) for the solver
    int n_slots = 0, n_lev = 0;      // stored blocks; elimination-tree levels
    std::vector<int> perm, slot_kr, slot_kc, dslot, lev_start, lev_col, ug_start, ug_split, ug_task_start, crit_grp;
    std::vector<Int4> ug, inv_rec, imu_blk;
    std::vector<Int2> rs, cs, imu_vec;
    std::vector<int> rs_start, cs_start, blob;
    struct BlobOff {
        size_t perm, dslot, lev_start, lev_col, ug_start, ug_split, crit_grp, ug_task_start, ug, rs_start, rs, cs_start, cs,
            inv_rec;
    } off{};
    // landmark groups of the build (grp_w < 0: a one-landmark group of the scalar path, listed in big_grp)
    int n_lgrp = 0, n_big = 0;
    std::vector<int> grp_pt, grp_w, grp_tp, grp_blk, blkoff, grp_kf, rhsoff, lkf_kf, big_grp, blk_start, rhs_start;
    std::vector<uint8_t> tp;
    std::vector<int16_t> slot_lkf, e_lkf;
    std::vector<int> ib_start, iv_start;   // with imu_blk / imu_vec: the inertial work lists (the evaluating rank's)
    // the solver's storage: 1 every block in LDS; 2 (the pattern does not fit) the vectors, the schedule and the first
    // n_lds blocks in LDS, the rest in global scratch; 0 (no LDS attribute, or a test build) every block in global scratch
    int use_lds = 0, n_lds = 0, blob_ints = 0;   // blob_ints > 0: the schedule is staged in LDS too
    size_t ldlt_lds = 0, n_reduce = 0;   // the solver's dynamic LDS bytes; doubles of [packed blocks | b | coef]
};

struct PlanWork {   // what one step of plan_lba hands to the next and the device never sees
    std::vector<std::vector<int>> pe;   // per caller point: its caller edges
    std::vector<uint8_t> adj, pat;      // keyframe adjacency (symmetric); filled lower pattern in positions
    std::vector<int> ipos, slot, level; // keyframe -> position; (row, column) position -> block slot; position -> level
};

// Step 1: the problem's sizes checked, the reduced layout, this rank's landmarks and their edges in device order, and
// the keyframe adjacency from ALL landmarks (every rank of a sharded solve lays out the identical packed system).
inline omv_status plan_edge_order(const omv_lba_problem &p, int rank, int world, const LbaLimits &lim, bool shared,
                                  LbaPlan &P, PlanWork &W) {
    if (p.n_cams <= 0 || p.n_cams > lim.max_cams || p.n_kf > lim.max_kf || p.n_pts < 0 || p.n_mono < 0 ||
        p.n_imu > lim.max_imu || p.n_opt > p.n_kf || p.n_opt < 1)
        return OMV_ERR_ARG;
    P.nb = p.n_opt + (shared ? 1 : 0);
    if (shared) {   // the pair's value lives in every bImu keyframe's bg / ba; without one there is no pair
        for (int k = 0; k < p.n_kf && P.shared_kf < 0; ++k)
            if (p.kf_imu[k]) P.shared_kf = k;
        if (P.shared_kf < 0) return OMV_ERR_ARG;
        P.shared_blk = p.n_opt;
    }
    const int C = p.n_cams, K = p.n_kf, P_all = p.n_pts;
    const int EM = p.n_mono, ES = p.n_stereo > 0 ? p.n_stereo : 0, E_all = EM + ES;
    if (ES > 0 && (!p.stereo_pt || !p.stereo_kf || !p.stereo_obs || !p.stereo_inv_sigma2)) return OMV_ERR_ARG;
    for (int e = 0; e < ES; ++e)   // an EdgeStereo exists only where mvuRight >= 0 (Optimizer.cc:3075, :3108)
        if (!(p.stereo_obs[3 * (size_t)e + 2] >= 0.0)) return OMV_ERR_ARG;
    for (int c = 0; c < C; ++c)
        if (p.cam_model && p.cam_model[c] != OMV_CAM_KB8 && p.cam_model[c] != OMV_CAM_PINHOLE) return OMV_ERR_ARG;
    // visual edge e < EM: EdgeMono e; e >= EM: EdgeStereo e - EM (camera 0, EdgeStereo(0) at :3118)
    auto e_pt_of = [&](int e) { return e < EM ? p.mono_pt[e] : p.stereo_pt[e - EM]; };
    auto e_kf_of = [&](int e) { return e < EM ? p.mono_kf[e] : p.stereo_kf[e - EM]; };
    auto e_cam_of = [&](int e) { return e < EM ? p.mono_cam[e] : 0; };
    // reduced-system layout: per optimisable keyframe pose (6) [+ v bg ba (9)]
    P.offP.assign(K, -1), P.offV.assign(K, -1), P.offG.assign(K, -1), P.offA.assign(K, -1);
    P.n_red = 16 * P.nb;
    for (int k = 0; k < p.n_opt; ++k) {
        P.offP[k] = 16 * k;
        if (p.kf_imu[k]) P.offV[k] = 16 * k + 6, P.offG[k] = 16 * k + 9, P.offA[k] = 16 * k + 12;
    }
    if (shared)   // every bImu keyframe, fixed ones too, takes the pair's step: all hold its value (Optimizer.cc:818-829)
        for (int k = 0; k < K; ++k)
            if (p.kf_imu[k]) P.offG[k] = 16 * P.shared_blk + 9, P.offA[k] = 16 * P.shared_blk + 12;
    // landmark order: by the first optimisable keyframe observing them (workgroup keyframe spans stay small)
    std::vector<std::vector<int>> &pe = W.pe = std::vector<std::vector<int>>(P_all);
    for (int e = 0; e < E_all; ++e) {
        if (e_pt_of(e) < 0 || e_pt_of(e) >= P_all || e_kf_of(e) < 0 || e_kf_of(e) >= K || e_cam_of(e) < 0 || e_cam_of(e) >= C)
            return OMV_ERR_ARG;
        pe[e_pt_of(e)].push_back(e);
    }
    std::vector<int> key(P_all, 1 << 30);
    for (int q = 0; q < P_all; ++q)
        for (int e : pe[q]) key[q] = std::min(key[q], e_kf_of(e) < p.n_opt ? e_kf_of(e) : (1 << 29) + e_kf_of(e));
    std::vector<int> &order = P.order = std::vector<int>(P_all);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
    // block pattern of the reduced system (keyframe blocks) from ALL landmarks
    const int nb = P.nb, n_opt = p.n_opt;
    W.adj.assign((size_t)nb * nb, 0);
    for (int q = 0; q < P_all; ++q)
        for (int a : pe[q])
            for (int b : pe[q]) {
                const int i = e_kf_of(a), j = e_kf_of(b);
                if (i < n_opt && j < n_opt && i != j) W.adj[(size_t)i * nb + j] = 1;
            }
    // this rank's landmarks: a contiguous share of the landmark order
    if (world > 1) {
        const size_t lo = (size_t)P_all * rank / world, hi = (size_t)P_all * (rank + 1) / world;
        order = std::vector<int>(order.begin() + lo, order.begin() + hi);
    }
    const int np = (int)order.size();
    int E = 0;
    for (int q : order) E += (int)pe[q].size();
    if (np > lim.max_pts || E > lim.max_mono) return OMV_ERR_ARG;
    P.pt_edge.assign(np + 1, 0), P.pt_slot.assign(np + 1, 0);
    for (int q = 0; q < np; ++q) {
        std::vector<int> es = pe[order[q]];
        std::stable_sort(es.begin(), es.end(), [&](int a, int b) { return e_kf_of(a) < e_kf_of(b); });
        P.pt_edge[q] = (int)P.e_pt.size();
        P.pt_slot[q] = (int)P.slot_kf.size();
        int last_kf = -1;
        for (int e : es) {
            const int kf = e_kf_of(e);
            if (kf != last_kf) P.slot_kf.push_back(kf), last_kf = kf;
            P.e_pt.push_back(q), P.e_kf.push_back(kf), P.e_cam.push_back(e_cam_of(e));
            P.e_slot.push_back((int)P.slot_kf.size() - 1);
            if (e < EM) {
                P.e_obs.push_back(p.mono_obs[2 * e]), P.e_obs.push_back(p.mono_obs[2 * e + 1]);
                P.e_w.push_back(p.mono_inv_sigma2[e]), P.e_ur.push_back(-1.f);
            } else {   // the reference stores mvuRight (a float >= 0) in the double measurement
                const double *o = p.stereo_obs + 3 * (size_t)(e - EM);
                P.e_obs.push_back(o[0]), P.e_obs.push_back(o[1]);
                P.e_w.push_back(p.stereo_inv_sigma2[e - EM]), P.e_ur.push_back((float)o[2]);
            }
            P.perm_edge.push_back(e);
        }
    }
    P.pt_edge[np] = E, P.pt_slot[np] = P.n_pt_slots = (int)P.slot_kf.size();
    P.slot_edge.assign(P.n_pt_slots + 1, 0);
    for (int e = E - 1; e >= 0; --e) P.slot_edge[P.e_slot[e]] = e;
    P.slot_edge[P.n_pt_slots] = E;
    P.track_depth.assign(np, 1e30f);   // MapPoint::mTrackDepth in device order (the device epilogue's bClose)
    if (p.pt_track_depth)
        for (int q = 0; q < np; ++q) P.track_depth[q] = p.pt_track_depth[order[q]];
    return OMV_OK;
}

// plan_order's block budget for a whole map (plan_fiba, either bias form, and the pose graph).  A whole map's blocks
// rarely fit the LDS: when the keyframe order itself is past the budget the hybrid storage holds whichever order wins,
// so the budget no longer picks among them (fewest levels, then fewest blocks).
inline int whole_map_slot_budget(int n, const std::vector<uint8_t> &adj, int budget) {
    int ns0 = 0;
    std::vector<uint8_t> pat;
    std::vector<int> id(n), lev;
    std::iota(id.begin(), id.end(), 0);
    symbolic_ldlt(n, adj, id, pat, lev, ns0);
    return ns0 > budget ? std::numeric_limits<int>::max() : budget;
}
// The blocks the solver's LDS holds beside its two vectors of n_red rows (0 without the LDS attribute).
inline int lds_slot_budget(bool lds_ok, int n_red) {
    const size_t vec_bytes = 2 * (size_t)n_red * sizeof(double);
    return lds_ok && kLdltLds > vec_bytes ? (int)((kLdltLds - vec_bytes) / (256 * sizeof(double))) : 0;
}

// The stored blocks and the level schedule of the block LDL^T of `nb` blocks with adjacency `adj` in the elimination
// order P.perm (position -> block): the filled pattern, the slots column-major in positions, each level's columns, its
// trailing updates grouped by target block, the inverse records and the row / column structures of the substitutions.
// What the solver (omv_ldlt.h) reads; plan_pattern and the pose graph's plan (essgraph_plan.h) both end here.
inline void plan_schedule(int nb, const std::vector<uint8_t> &adj, LbaPlan &P, PlanWork &W) {
    std::vector<uint8_t> &pat = W.pat;
    const std::vector<int> &perm = P.perm;
    W.ipos.resize(nb);
    for (int q = 0; q < nb; ++q) W.ipos[perm[q]] = q;
    std::vector<int> &level = W.level, &slot = W.slot, &dslot = P.dslot;
    const int n_lev = P.n_lev = symbolic_ldlt(nb, adj, perm, pat, level, P.n_slots);
    slot.assign((size_t)nb * nb, -1), dslot.resize(nb);
    std::vector<int> slot_kr_pos, slot_kc_pos;   // block positions of each slot
    for (int j = 0; j < nb; ++j)   // column-major in positions: a column's panel blocks sit together
        for (int i = j; i < nb; ++i)
            if (pat[(size_t)i * nb + j]) {
                slot[(size_t)i * nb + j] = (int)P.slot_kr.size();
                P.slot_kr.push_back(perm[i]), P.slot_kc.push_back(perm[j]);
                slot_kr_pos.push_back(i), slot_kc_pos.push_back(j);
            }
    for (int k = 0; k < nb; ++k) dslot[k] = slot[(size_t)k * nb + k];
    // level schedule: columns per level; trailing updates grouped by target block (ascending k)
    std::vector<int> &lev_start = P.lev_start, &lev_col = P.lev_col, &ug_start = P.ug_start, &ug_split = P.ug_split,
                     &ug_task_start = P.ug_task_start, &crit_grp = P.crit_grp;
    lev_start.assign(n_lev + 1, 0), ug_start.assign(n_lev + 1, 0), ug_split.assign(std::max(n_lev, 1), 0);
    ug_task_start.assign(1, 0), crit_grp.assign(nb, -1);
    std::vector<Int4> &ug = P.ug;
    for (int l = 0; l < n_lev; ++l) {
        lev_start[l] = (int)lev_col.size(), ug_start[l] = (int)ug_task_start.size() - 1;
        std::map<int, std::vector<Int4>> by_target;   // target slot -> updates in ascending k
        for (int k = 0; k < nb; ++k) {
            if (level[k] != l) continue;
            lev_col.push_back(k);
            std::vector<int> col;
            for (int i = k + 1; i < nb; ++i)
                if (pat[(size_t)i * nb + k]) col.push_back(i);
            for (size_t a = 0; a < col.size(); ++a)
                for (size_t c = 0; c <= a; ++c) {
                    const int i = col[a], j = col[c];
                    by_target[slot[(size_t)i * nb + j]].push_back(
                        Int4{slot[(size_t)i * nb + j], slot[(size_t)i * nb + k], slot[(size_t)j * nb + k], dslot[k]});
                }
        }
        // the diagonal blocks of level l + 1 first: their inverses wait only for these groups, the rest of the level's
        // updates run beside those inverses
        for (int pass = 0; pass < 2; ++pass) {
            for (auto &kv : by_target) {
                const int kr = slot_kr_pos[kv.first], kc = slot_kc_pos[kv.first];
                const bool crit = kr == kc && level[kr] == l + 1;
                if (crit != (pass == 0)) continue;
                if (crit) crit_grp[kr] = (int)ug_task_start.size() - 1;
                ug.insert(ug.end(), kv.second.begin(), kv.second.end());
                ug_task_start.push_back((int)ug.size());
            }
            if (pass == 0) ug_split[l] = (int)ug_task_start.size() - 1;
        }
    }
    lev_start[n_lev] = (int)lev_col.size(), ug_start[n_lev] = (int)ug_task_start.size() - 1;
    P.inv_rec.assign(2 * (size_t)std::max(nb, 1), Int4{0, 0, 0, 0});
    for (size_t c = 0; c < lev_col.size(); ++c) {
        const int col = lev_col[c], g = crit_grp[col];
        const int u0 = g >= 0 ? ug_task_start[g] : 0, u1 = g >= 0 ? ug_task_start[g + 1] : 0;
        P.inv_rec[2 * c] = Int4{dslot[col], u0, u1, 0};
        if (u0 < u1) P.inv_rec[2 * c + 1] = ug[u0];
    }
    P.rs_start.assign(nb + 1, 0), P.cs_start.assign(nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
        for (int k = 0; k < i; ++k)
            if (pat[(size_t)i * nb + k]) P.rs.push_back(Int2{slot[(size_t)i * nb + k], k});
        P.rs_start[i + 1] = (int)P.rs.size();
    }
    for (int k = 0; k < nb; ++k) {
        for (int i = k + 1; i < nb; ++i)
            if (pat[(size_t)i * nb + k]) P.cs.push_back(Int2{slot[(size_t)i * nb + k], i});
        P.cs_start[k + 1] = (int)P.cs.size();
    }
}

// Step 2: the inertial pairs checked and added to the adjacency, the elimination order (every rank of a sharded solve
// plans from the same full pattern), its symbolic LDL^T, the stored blocks and the level schedule.
inline omv_status plan_pattern(const omv_lba_problem &p, bool lds_ok, bool whole_map, int max_cuts, LbaPlan &P,
                               PlanWork &W) {
    const int nb = P.nb, n_opt = p.n_opt, K = p.n_kf, S = P.shared_blk;
    std::vector<uint8_t> &adj = W.adj;
    for (int i = 0; i < p.n_imu; ++i) {
        const int a = p.imu_kf1[i], b = p.imu_kf2[i];
        if (a < 0 || a >= K || b < 0 || b >= K || a == b) return OMV_ERR_ARG;
        if (a < n_opt && b < n_opt) adj[(size_t)a * nb + b] = adj[(size_t)b * nb + a] = 1;
        if (S < 0) continue;
        // the shared pair: vertices G and A of every EdgeInertial, which exists between two bImu keyframes only
        // (Optimizer.cc:469, :485-486)
        if (!p.kf_imu[a] || !p.kf_imu[b]) return OMV_ERR_ARG;
        for (int k : {a, b})
            if (k < n_opt) adj[(size_t)k * nb + S] = adj[(size_t)S * nb + k] = 1;
    }
    const int lds_slots = lds_slot_budget(lds_ok, P.n_red);
    auto whole_map_budget = [&](int n, const std::vector<uint8_t> &a, int budget) {
        return whole_map ? whole_map_slot_budget(n, a, budget) : budget;   // plan_lba keeps its budget
    };
    if (S < 0) {
        P.perm = plan_order(nb, adj, whole_map_budget(nb, adj, std::max(lds_slots, 1)), max_cuts);
    } else {
        // The pair's block borders every keyframe with an inertial edge: counted into a dissection it would sit in every
        // separator and plan_order would reject every cut.  The keyframes are dissected without it (its row of at most
        // nb blocks taken off the LDS budget) and it is eliminated last.
        std::vector<uint8_t> sub((size_t)n_opt * n_opt);
        for (int i = 0; i < n_opt; ++i)
            for (int j = 0; j < n_opt; ++j) sub[(size_t)i * n_opt + j] = adj[(size_t)i * nb + j];
        P.perm = plan_order(n_opt, sub, whole_map_budget(n_opt, sub, std::max(lds_slots - nb, 1)), max_cuts);
        P.perm.push_back(S);
    }
    plan_schedule(nb, adj, P, W);
    return OMV_OK;
}

// Step 3: buildSystem landmark groups (land_group): whole landmarks in landmark order, at most kGrpEdges edges, kGrpLand
// landmarks, kGrpSlots slots and kGrpW optimisable keyframes; a landmark past one of those alone forms a group of
// its own built by the scalar path (land_group_big).  Per group: its keyframes in elimination order (local index a),
// its record (w(w+1)/2 blocks a >= b of 36, then w rows of [gradient 6 | Schur rhs 6]), the 16x16 output tiles that
// hold a co-observed keyframe pair, and per diagonal tile the residual rows of its keyframes' edges.
inline void plan_groups(int n_opt, LbaPlan &P, const PlanWork &W) {
    const int nb = P.nb;   // blocks (n_opt keyframes, then the shared pair if any: it observes no landmark)
    const int np = (int)P.order.size(), n_slots = P.n_slots;
    const std::vector<int> &pt_edge = P.pt_edge, &pt_slot = P.pt_slot, &slot_kf = P.slot_kf, &ipos = W.ipos, &slot = W.slot;
    std::vector<int> &grp_blk = P.grp_blk, &grp_kf = P.grp_kf, &blkoff = P.blkoff, &rhsoff = P.rhsoff;
    P.slot_lkf.assign(P.n_pt_slots, -1), P.grp_pt.assign(1, 0), P.grp_tp.assign(1, 0);
    P.blk_start.assign(n_slots + 1, 0), P.rhs_start.assign(nb + 1, 0);
    // per reduced-system block / keyframe: the (blkoff / rhsoff index) of each contributing group, in group order
    std::vector<std::vector<int>> by_blk(n_slots), by_kf(nb);
    auto opt_kfs = [&](int q0, int q1) {   // distinct optimisable keyframes of landmarks [q0, q1)
        std::set<int> k;
        for (int q = q0; q < q1; ++q)
            for (int a = pt_slot[q]; a < pt_slot[q + 1]; ++a)
                if (slot_kf[a] < n_opt) k.insert(slot_kf[a]);
        return k;
    };
    // the MFMA operand panels fit their LDS region
    auto panel_ok = [&](int n_land, int n_kf) { return (n_kf + 1) / 2 * ((3 * n_land + 3) & ~3) <= kPanel; };
    auto fits = [&](int q0, int q1) {
        const int nk = (int)opt_kfs(q0, q1).size();
        return pt_edge[q1] - pt_edge[q0] <= kGrpEdges && q1 - q0 <= kGrpLand && pt_slot[q1] - pt_slot[q0] <= kGrpSlots &&
               nk <= kGrpW && panel_ok(q1 - q0, nk);
    };
    for (int q = 0; q < np;) {
        int r = q + 1;
        const bool big = !fits(q, r);
        if (!big) {
            std::set<int> k = opt_kfs(q, r);
            while (r < np && r - q < kGrpLand && pt_edge[r + 1] - pt_edge[q] <= kGrpEdges &&
                   pt_slot[r + 1] - pt_slot[q] <= kGrpSlots) {
                std::set<int> k2 = k;
                for (int a = pt_slot[r]; a < pt_slot[r + 1]; ++a)
                    if (slot_kf[a] < n_opt) k2.insert(slot_kf[a]);
                if ((int)k2.size() > kGrpW || !panel_ok(r + 1 - q, (int)k2.size())) break;
                k.swap(k2);
                ++r;
            }
        }
        // the group's keyframes in elimination order
        std::set<int> ks = opt_kfs(q, r);
        std::vector<int> kl(ks.begin(), ks.end());
        std::sort(kl.begin(), kl.end(), [&](int x, int y) { return ipos[x] < ipos[y]; });
        const int w = (int)kl.size(), nblk = w * (w + 1) / 2;
        std::vector<int> lk(n_opt, -1);
        for (int a = 0; a < w; ++a) lk[kl[a]] = a;
        for (int a = pt_slot[q]; a < pt_slot[r]; ++a) P.slot_lkf[a] = (int16_t)(slot_kf[a] < n_opt ? lk[slot_kf[a]] : -1);
        const int g = (int)P.grp_w.size();
        P.grp_w.push_back(big ? -w - 1 : w);
        grp_blk.push_back((int)blkoff.size());
        grp_kf.push_back((int)rhsoff.size());
        blkoff.resize(blkoff.size() + nblk, -1);
        rhsoff.resize(rhsoff.size() + w, -1);
        P.lkf_kf.insert(P.lkf_kf.end(), kl.begin(), kl.end());
        // co-observed keyframe pairs (a >= b): the group's blocks
        std::vector<uint8_t> co((size_t)std::max(w, 1) * std::max(w, 1), 0);
        for (int x = q; x < r; ++x) {
            std::vector<int> loc;
            for (int a = pt_slot[x]; a < pt_slot[x + 1]; ++a)
                if (slot_kf[a] < n_opt) loc.push_back(lk[slot_kf[a]]);
            for (int u : loc)
                for (int v : loc)
                    if (u >= v) co[(size_t)u * w + v] = 1;
        }
        for (int u = 0; u < w; ++u) {
            by_kf[kl[u]].push_back(grp_kf[g] + u);
            for (int v = 0; v <= u; ++v)
                if (co[(size_t)u * w + v])
                    by_blk[slot[(size_t)ipos[kl[u]] * nb + ipos[kl[v]]]].push_back(grp_blk[g] + u * (u + 1) / 2 + v);
        }
        if (!big) {
            const int nt = (w + 1) / 2;
            for (int ti = 0; ti < nt; ++ti)
                for (int tj = 0; tj <= ti; ++tj) {
                    bool any = false;
                    for (int u = 2 * ti; u < std::min(w, 2 * ti + 2) && !any; ++u)
                        for (int v = 2 * tj; v < std::min(w, 2 * tj + 2) && !any; ++v) any = u >= v && co[(size_t)u * w + v];
                    if (any) P.tp.push_back((uint8_t)ti), P.tp.push_back((uint8_t)tj);
                }
        }
        P.grp_tp.push_back((int)P.tp.size() / 2);
        P.grp_pt.push_back(r);
        q = r;
    }
    // records contiguous per block (per keyframe), in group order: assemble_kernel reads them as one run
    for (int t = 0; t < n_slots; ++t) {
        P.blk_start[t + 1] = P.blk_start[t] + (int)by_blk[t].size();
        for (size_t i = 0; i < by_blk[t].size(); ++i) blkoff[by_blk[t][i]] = P.blk_start[t] + (int)i;
    }
    for (int k = 0; k < nb; ++k) {
        P.rhs_start[k + 1] = P.rhs_start[k] + (int)by_kf[k].size();
        for (size_t i = 0; i < by_kf[k].size(); ++i) rhsoff[by_kf[k][i]] = P.rhs_start[k] + (int)i;
    }
    P.n_lgrp = (int)P.grp_w.size();
    for (int g = 0; g < P.n_lgrp; ++g)
        if (P.grp_w[g] < 0) P.big_grp.push_back(g);
    P.n_big = (int)P.big_grp.size();
    P.e_lkf.resize(P.e_slot.size());
    for (size_t e = 0; e < P.e_slot.size(); ++e) P.e_lkf[e] = P.slot_lkf[P.e_slot[e]];
}

// Step 4: inertial edges per block (edge, side of the row keyframe, side of the column keyframe; side 0 = kf1) and per
// keyframe (edge, side), in edge order, only on the rank that evaluates them; the inertial information (EdgeInertial
// ctor :486-495) and random-walk information of every edge.
// With the shared pair an edge has a third side, 2 = the pair's block: its G / A columns (local variables 9..14 of the
// edge's form, kf1's in the per-keyframe form) belong there, the keyframe sides keep P and V, and there is no
// random-walk edge (Optimizer.cc:484-487, :520): infoG / infoA stay zero.
inline void plan_inertial(const omv_lba_problem &p, bool imu_here, LbaPlan &P, const PlanWork &W) {
    const int nb = P.nb, n_opt = p.n_opt, NI = p.n_imu, n_slots = P.n_slots, S = P.shared_blk;
    const int n_sides = S >= 0 ? 3 : 2;
    const std::vector<int> &ipos = W.ipos, &slot = W.slot;
    P.ib_start.assign(n_slots + 1, 0), P.iv_start.assign(nb + 1, 0);
    std::vector<std::vector<Int4>> bl(n_slots);
    std::vector<std::vector<Int2>> vl(nb);
    if (imu_here)
        for (int i = 0; i < NI; ++i) {
            // the block of each side; a fixed keyframe has none
            int kk[3] = {p.imu_kf1[i], p.imu_kf2[i], S};
            for (int sd = 0; sd < 2; ++sd)
                if (kk[sd] >= n_opt) kk[sd] = -1;
            for (int sr = 0; sr < n_sides; ++sr) {
                if (kk[sr] < 0) continue;
                vl[kk[sr]].push_back(Int2{i, sr});
                for (int sc = 0; sc < n_sides; ++sc) {
                    if (kk[sc] < 0 || ipos[kk[sr]] < ipos[kk[sc]]) continue;
                    bl[slot[(size_t)ipos[kk[sr]] * nb + ipos[kk[sc]]]].push_back(Int4{i, sr, sc, 0});
                }
            }
        }
    for (int t = 0; t < n_slots; ++t)
        P.imu_blk.insert(P.imu_blk.end(), bl[t].begin(), bl[t].end()), P.ib_start[t + 1] = (int)P.imu_blk.size();
    for (int k = 0; k < nb; ++k)
        P.imu_vec.insert(P.imu_vec.end(), vl[k].begin(), vl[k].end()), P.iv_start[k + 1] = (int)P.imu_vec.size();
    const size_t ni = (size_t)std::max(NI, 0);
    P.info9.assign(ni * 81, 0.0), P.infoG.assign(ni * 9, 0.0), P.infoA.assign(ni * 9, 0.0);
    for (int i = 0; i < NI; ++i) {
        const float *pr = p.preint + (size_t)i * OMV_PREINT_FLOATS + kPreintCov;
        std::vector<double> A(81);
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) A[r * 9 + c] = (double)pr[r * 15 + c];
        host_inv(A, 9);
        for (int r = 0; r < 9; ++r)
            for (int c = r + 1; c < 9; ++c) A[r * 9 + c] = A[c * 9 + r] = (A[r * 9 + c] + A[c * 9 + r]) / 2;
        std::vector<double> w, V;
        host_sym_eig(A, 9, w, V);
        for (double &x : w)
            if (x < 1e-12) x = 0;
        const double sc = p.imu_info_scale ? (double)p.imu_info_scale[i] : 1.0;
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) {
                double s = 0;
                for (int k = 0; k < 9; ++k) s += V[r * 9 + k] * w[k] * V[c * 9 + k];
                P.info9[(size_t)i * 81 + r * 9 + c] = s * sc;
            }
        double g[9], a[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) g[3 * r + c] = pr[(9 + r) * 15 + 9 + c], a[3 * r + c] = pr[(12 + r) * 15 + 12 + c];
        if (S >= 0) continue;   // no EdgeGyroRW / EdgeAccRW beside a shared pair
        omv_g2o::inv3(g, &P.infoG[(size_t)9 * i]);
        omv_g2o::inv3(a, &P.infoA[(size_t)9 * i]);
    }
}

// Step 5: the schedule packed for the solver and its LDS mode (LbaPlan::use_lds).
inline void plan_lds(bool lds_ok, LbaPlan &P) {
    const size_t nred = (size_t)P.n_red;
    const size_t ldlt_bytes = ((size_t)P.n_slots * 256 + 2 * nred) * sizeof(double);
    P.use_lds = !lds_ok ? 0 : ldlt_bytes <= kLdltLds ? 1 : kLdltLds > 2 * nred * sizeof(double) + 8 * 256 * sizeof(double) ? 2 : 0;
#ifdef OMV_LBA_FORCE_G
    P.use_lds = 0;
#endif
    P.ldlt_lds = P.use_lds == 1 ? ldlt_bytes : 0;
    std::vector<int> &blob = P.blob;
    auto put = [&](const auto &v) {   // 16-byte aligned sub-array
        const size_t off = blob.size(), n = v.size() * sizeof(v[0]) / sizeof(int);
        blob.resize(off + ((n + 3) & ~(size_t)3));
        if (n) std::memcpy(blob.data() + off, v.data(), n * sizeof(int));
        return off;
    };
    LbaPlan::BlobOff &o = P.off;
    o.perm = put(P.perm), o.dslot = put(P.dslot), o.lev_start = put(P.lev_start), o.lev_col = put(P.lev_col);
    o.ug_start = put(P.ug_start), o.ug_split = put(P.ug_split), o.crit_grp = put(P.crit_grp);
    o.ug_task_start = put(P.ug_task_start), o.ug = put(P.ug), o.rs_start = put(P.rs_start), o.rs = put(P.rs);
    o.cs_start = put(P.cs_start), o.cs = put(P.cs), o.inv_rec = put(P.inv_rec);
    // stage the schedule in LDS when it fits beside the blocks and vectors
    const size_t sched_bytes = blob.size() * sizeof(int);
    P.blob_ints = 0;
    P.n_lds = P.n_slots;
    if (P.use_lds == 2) {   // hybrid: the vectors and the schedule in LDS, then as many blocks as fit
        const size_t vb = 2 * nred * sizeof(double);
        const bool sch = vb + sched_bytes + 8 * 256 * sizeof(double) <= kLdltLds;
        P.n_lds = std::min(P.n_slots, (int)((kLdltLds - vb - (sch ? sched_bytes : 0)) / (256 * sizeof(double))));
        P.ldlt_lds = (size_t)P.n_lds * 256 * sizeof(double) + vb + (sch ? sched_bytes : 0);
        P.blob_ints = sch ? (int)blob.size() : 0;
    } else if (P.use_lds && P.ldlt_lds + sched_bytes <= kLdltLds) {
        P.ldlt_lds += sched_bytes;
        P.blob_ints = (int)blob.size();
    }
    // [packed blocks | b | coef], contiguous: the one buffer a sharded solve all-reduces per trial
    P.n_reduce = (size_t)P.n_slots * 256 + 2 * nred;
}

// The plan of problem `p` for rank `rank` of `world` on a handle of capacities `lim`; lds_ok: the solver kernels may
// take kLdltLds of dynamic LDS.  OMV_ERR_ARG for every problem omv_lba_set_problem rejects (`out` is then unspecified).
// shared: the keyframes share one gyro / acc bias pair (LbaPlan::shared_blk; one rank); max_cuts: plan_order's.
// whole_map: the LDS budget stops choosing among orders once the keyframe order itself is past it (plan_pattern).
inline omv_status plan_problem(const omv_lba_problem &p, int rank, int world, const LbaLimits &lim, bool lds_ok, bool shared,
                               bool whole_map, int max_cuts, LbaPlan &out) {
    out = LbaPlan{};
    PlanWork W;
    if (plan_edge_order(p, rank, world, lim, shared, out, W) != OMV_OK ||
        plan_pattern(p, lds_ok, whole_map, max_cuts, out, W) != OMV_OK)
        return OMV_ERR_ARG;
    plan_groups(p.n_opt, out, W);
    plan_inertial(p, p.n_imu > 0 && rank == 0, out, W);
    plan_lds(lds_ok, out);
    return OMV_OK;
}
inline omv_status plan_lba(const omv_lba_problem &p, int rank, int world, const LbaLimits &lim, bool lds_ok, LbaPlan &out) {
    return plan_problem(p, rank, world, lim, lds_ok, false, false, 0, out);
}

// The plan of a FullInertialBA problem (omv_fiba): the whole map on one rank.  shared_bias: the bInit form (one
// VertexGyroBias / VertexAccBias for every keyframe, Optimizer.cc:441-450), which needs an inertial edge -- with none
// the pair would hang on its two priors alone -- and non-negative prior informations.  plan_order tries every cut at an
// O(nb^3) symbolic factorisation each, which a local window of 25 keyframes does not feel and a map of hundreds does
// (DESIGN has the measured times): here at most kFibaCuts evenly spaced cuts are tried.
constexpr int kFibaCuts = 32;
inline omv_status plan_fiba(const omv_lba_problem &p, bool shared_bias, double prior_g, double prior_a,
                            const LbaLimits &lim, bool lds_ok, LbaPlan &out) {
    if (shared_bias && (p.n_imu < 1 || !(prior_g >= 0.0) || !(prior_a >= 0.0) || !std::isfinite(prior_g) ||
                        !std::isfinite(prior_a)))
        return OMV_ERR_ARG;
    return plan_problem(p, 0, 1, lim, lds_ok, shared_bias, true, kFibaCuts, out);
}

}  // namespace omv_lba_plan
