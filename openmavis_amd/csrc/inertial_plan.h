// Host-side planning of one InertialOptimization job (inertial.hip), apart from the device upload and testable without
// a GPU (tests/test_inertial_plan_cpu.py: through the host-only hook omv_inertial_opt_plan, and as the stand-alone program
// tests/cpp/inertial_plan_host.cpp under the host sanitizers).
//
// KeyFrame::mPrevKF is a single link, so the EdgeInertialGS edges of a map (Optimizer.cc:3571-3610) form a forest of
// simple paths over its keyframes: a keyframe is kf1 (the previous one) of at most one edge and kf2 of at most one.  The
// planner orders the keyframes along their paths -- heads (no incoming edge) in ascending keyframe index, each followed
// to its tail -- so that the velocity part of the normal equations is block-tridiagonal in position order: position p
// couples with p + 1 exactly when an edge leaves the keyframe at p.  A keyframe without an edge is a path of its own.
// Rejected (false): an index out of range, an edge from a keyframe to itself, a keyframe with two successors or two
// predecessors, a cycle.
#pragma once
#include <cstdint>
#include <vector>

namespace omv_inertial {

struct Plan {
    std::vector<int32_t> order;      // [K] position -> keyframe
    std::vector<int32_t> pos_of;     // [K] keyframe -> position
    std::vector<int32_t> edge_in;    // [K] per position: the edge whose kf2 sits there, or -1
    std::vector<int32_t> edge_out;   // [K] per position: the edge whose kf1 sits there, or -1 (then its kf2 is at p + 1)
    int n_paths = 0;
};

inline bool plan_paths(int K, int E, const int32_t *kf1, const int32_t *kf2, Plan *out) {
    if (K < 0 || E < 0 || (E > 0 && (!kf1 || !kf2))) return false;
    std::vector<int32_t> in(K, -1), outgoing(K, -1);
    for (int e = 0; e < E; ++e) {
        const int a = kf1[e], b = kf2[e];
        if (a < 0 || a >= K || b < 0 || b >= K || a == b) return false;
        if (outgoing[a] >= 0 || in[b] >= 0) return false;   // two successors / two predecessors
        outgoing[a] = e, in[b] = e;
    }
    Plan &P = *out;
    P.order.clear(), P.order.reserve(K);
    P.pos_of.assign(K, -1), P.edge_in.assign(K, -1), P.edge_out.assign(K, -1);
    P.n_paths = 0;
    for (int k = 0; k < K; ++k) {
        if (in[k] >= 0) continue;
        ++P.n_paths;
        for (int c = k;;) {
            const int p = (int)P.order.size();
            P.pos_of[c] = p, P.edge_in[p] = in[c], P.edge_out[p] = outgoing[c];
            P.order.push_back(c);
            if (outgoing[c] < 0) break;
            c = kf2[outgoing[c]];
        }
    }
    return (int)P.order.size() == K;   // a cycle has no head: its keyframes were never reached
}

}  // namespace omv_inertial
