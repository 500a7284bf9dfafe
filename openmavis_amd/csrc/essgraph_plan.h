// The host-side plan of one pose graph (essgraph.hip): which vertices are variables and where their rows sit in the
// solver's 16x16 blocks, the block adjacency, the elimination order, stored blocks and level schedule (lba_plan.h's
// plan_order / plan_schedule / plan_lds: the pose graph is a third client of that solver), and per stored block the
// fixed-order list of edge contributions it gathers.  plan_essgraph makes every argument check and reads no handle.
// Nothing here needs the HIP runtime: hipcc compiles this text into the product, the host compiler into
// tests/cpp/essgraph_plan_host.cpp.
#pragma once
#include "lba_plan.h"

namespace omv_essgraph_plan {

using omv_lba_plan::Int2;
using omv_lba_plan::Int4;
using omv_lba_plan::LbaPlan;
using omv_lba_plan::PlanWork;

struct EssLimits { int max_vertices, max_edges; };   // the handle's capacities (omv_essgraph_create)

// Variables per vertex: g2o::VertexSim3Expmap 7, VertexPose4DoF 4; rows of the edge's error: EdgeSim3 7, Edge4DoF 6.
inline int ess_dim(int kind) { return kind == OMV_ESSGRAPH_SIM3 ? 7 : 4; }
inline int ess_err_dim(int kind) { return kind == OMV_ESSGRAPH_SIM3 ? 7 : 6; }

struct EssPlan {
    int kind = 0, dim = 0, per_blk = 0;   // variables per vertex; vertices per 16-row block (2 Sim3, 4 4DoF)
    int n_v = 0, n_e = 0, n_opt = 0;
    std::vector<int> opt_v;    // [n_opt] optimisable vertices in caller order
    std::vector<int> row_of;   // [n_v] first row of the vertex in the system (16 block + dim local), -1: fixed
    std::vector<uint8_t> real_row;   // [16 nb] 1: a variable's row; 0: padding (diagonal 1, zero right-hand side)
    // the solver's side: nb, n_red, perm, stored blocks (slot_kr / slot_kc), level schedule, blob, LDS mode
    LbaPlan L;
    // Per stored block its contributions in edge order: (edge, side of the rows, side of the columns, 16 row0 + col0)
    // -- the dim x dim block J_sr^T Omega J_sc of the edge lands at (row0, col0) of the 16x16 block.  Side 0 is the
    // edge's vertex i (g2o's vertex 0).  Parallel edges are separate entries of one list: they sum.
    std::vector<int> cb_start;
    std::vector<Int4> cb;
    // Per block the right-hand-side contributions in edge order: (edge, side, row0, 0).
    std::vector<int> cv_start;
    std::vector<Int4> cv;
};

// The plan of a pose graph of `kind` on a handle of capacities `lim`; lds_ok: the solver may take kLdltLds of dynamic
// LDS.  OMV_ERR_ARG: a null array, a size beyond the capacities, an edge naming a vertex that is not there, i == j, a
// table other than 0 / 1, no optimisable vertex.  An edge between two fixed vertices is in no list (chi2 only).
inline omv_status plan_essgraph(int kind, int n_v, const uint8_t *fixed, int n_e, const int32_t *ei, const int32_t *ej,
                                const int32_t *et, const EssLimits &lim, bool lds_ok, EssPlan &out) {
    out = EssPlan{};
    if ((kind != OMV_ESSGRAPH_SIM3 && kind != OMV_ESSGRAPH_4DOF) || n_v < 1 || n_v > lim.max_vertices || n_e < 0 ||
        n_e > lim.max_edges || !fixed || (n_e > 0 && (!ei || !ej || !et)))
        return OMV_ERR_ARG;
    for (int e = 0; e < n_e; ++e)
        if (ei[e] < 0 || ei[e] >= n_v || ej[e] < 0 || ej[e] >= n_v || ei[e] == ej[e] || et[e] < 0 || et[e] > 1)
            return OMV_ERR_ARG;
    EssPlan &P = out;
    P.kind = kind, P.dim = ess_dim(kind), P.per_blk = 16 / P.dim, P.n_v = n_v, P.n_e = n_e;
    P.row_of.assign(n_v, -1);
    for (int v = 0; v < n_v; ++v)
        if (!fixed[v]) {
            const int o = (int)P.opt_v.size();
            P.row_of[v] = 16 * (o / P.per_blk) + P.dim * (o % P.per_blk);
            P.opt_v.push_back(v);
        }
    P.n_opt = (int)P.opt_v.size();
    if (P.n_opt < 1) return OMV_ERR_ARG;
    LbaPlan &L = P.L;
    const int nb = L.nb = (P.n_opt + P.per_blk - 1) / P.per_blk;
    L.n_red = 16 * nb;
    P.real_row.assign((size_t)16 * nb, 0);
    for (int v : P.opt_v)
        for (int r = 0; r < P.dim; ++r) P.real_row[P.row_of[v] + r] = 1;
    PlanWork W;
    W.adj.assign((size_t)nb * nb, 0);
    for (int e = 0; e < n_e; ++e) {
        const int ri = P.row_of[ei[e]], rj = P.row_of[ej[e]];
        if (ri < 0 || rj < 0 || ri / 16 == rj / 16) continue;
        W.adj[(size_t)(ri / 16) * nb + rj / 16] = W.adj[(size_t)(rj / 16) * nb + ri / 16] = 1;
    }
    // the whole map's order: at most kFibaCuts dissections, the LDS budget as for FullInertialBA
    const int budget = std::max(omv_lba_plan::lds_slot_budget(lds_ok, L.n_red), 1);
    L.perm = omv_lba_plan::plan_order(nb, W.adj, omv_lba_plan::whole_map_slot_budget(nb, W.adj, budget),
                                      omv_lba_plan::kFibaCuts);
    omv_lba_plan::plan_schedule(nb, W.adj, L, W);
    omv_lba_plan::plan_lds(lds_ok, L);
    // contributions: every ordered pair of optimisable sides whose block is stored (row position >= column position)
    std::vector<std::vector<Int4>> bl(L.n_slots), vl(nb);
    for (int e = 0; e < n_e; ++e) {
        const int row[2] = {P.row_of[ei[e]], P.row_of[ej[e]]};
        for (int sr = 0; sr < 2; ++sr) {
            if (row[sr] < 0) continue;
            const int br = row[sr] / 16;
            vl[br].push_back(Int4{e, sr, row[sr] % 16, 0});
            for (int sc = 0; sc < 2; ++sc) {
                if (row[sc] < 0) continue;
                const int bc = row[sc] / 16;
                if (W.ipos[br] < W.ipos[bc]) continue;   // the transposed pair fills the stored block
                bl[W.slot[(size_t)W.ipos[br] * nb + W.ipos[bc]]].push_back(
                    Int4{e, sr, sc, 16 * (row[sr] % 16) + row[sc] % 16});
            }
        }
    }
    P.cb_start.assign(L.n_slots + 1, 0), P.cv_start.assign(nb + 1, 0);
    for (int t = 0; t < L.n_slots; ++t) P.cb.insert(P.cb.end(), bl[t].begin(), bl[t].end()), P.cb_start[t + 1] = (int)P.cb.size();
    for (int k = 0; k < nb; ++k) P.cv.insert(P.cv.end(), vl[k].begin(), vl[k].end()), P.cv_start[k + 1] = (int)P.cv.size();
    return OMV_OK;
}

}  // namespace omv_essgraph_plan
