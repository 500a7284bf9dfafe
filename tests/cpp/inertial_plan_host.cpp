// Stand-alone host program over openmavis_amd/csrc/inertial_plan.h (no HIP, no device): plans a set of edge lists and
// prints one line per case, "ok <n_paths> | order | edge_in | edge_out" or "reject".  Built with
// -fsanitize=address,undefined by tests/test_inertial_plan_cpu.py, which compares the lines with its own expectations.
#include <cstdio>
#include <random>
#include <vector>

#include "../../openmavis_amd/csrc/inertial_plan.h"

namespace {

void run(int K, const std::vector<int32_t> &a, const std::vector<int32_t> &b) {
    omv_inertial::Plan P;
    if (!omv_inertial::plan_paths(K, (int)a.size(), a.data(), b.data(), &P)) {
        std::printf("reject\n");
        return;
    }
    std::printf("ok %d |", P.n_paths);
    for (int v : P.order) std::printf(" %d", v);
    std::printf(" |");
    for (int v : P.edge_in) std::printf(" %d", v);
    std::printf(" |");
    for (int v : P.edge_out) std::printf(" %d", v);
    std::printf("\n");
}

}  // namespace

int main() {
    run(0, {}, {});
    run(1, {}, {});
    run(4, {0, 1, 2}, {1, 2, 3});                 // a chain
    run(6, {0, 1, 3, 4}, {1, 2, 4, 5});           // split by a bad keyframe (no edge into 3)
    run(5, {0, 3}, {1, 4});                       // 2 isolated
    run(5, {3, 0, 2, 4}, {0, 2, 4, 1});           // shuffled: 3 -> 0 -> 2 -> 4 -> 1
    run(3, {0, 0}, {1, 2});                       // two successors
    run(3, {0, 1}, {2, 2});                       // two predecessors
    run(3, {0, 1, 2}, {1, 2, 0});                 // a cycle
    run(3, {0}, {3});                             // out of range
    run(3, {1}, {1});                             // an edge to itself
    // a long shuffled chain with breaks, checked for consistency here
    const int K = 300;
    std::mt19937 rng(7);
    std::vector<int32_t> perm(K), a, b;
    for (int i = 0; i < K; ++i) perm[i] = i;
    for (int i = K - 1; i > 0; --i) std::swap(perm[i], perm[rng() % (i + 1)]);
    for (int i = 0; i + 1 < K; ++i)
        if (i % 37 != 36) a.push_back(perm[i]), b.push_back(perm[i + 1]);
    omv_inertial::Plan P;
    bool ok = omv_inertial::plan_paths(K, (int)a.size(), a.data(), b.data(), &P) && (int)P.order.size() == K;
    for (int p = 0; ok && p < K; ++p) {
        ok = P.pos_of[P.order[p]] == p;
        if (P.edge_out[p] >= 0) ok = ok && p + 1 < K && a[P.edge_out[p]] == P.order[p] && b[P.edge_out[p]] == P.order[p + 1] && P.edge_in[p + 1] == P.edge_out[p];
        else ok = ok && (p + 1 == K || P.edge_in[p + 1] < 0);
    }
    std::printf("long %s %d\n", ok ? "ok" : "bad", P.n_paths);
    return ok ? 0 : 1;
}
