// Stand-alone host program over openmavis_amd/csrc/omv_ldlt_host.h for tests/test_ldlt_host_cpu.py: plans a block pattern
// with the planners the handles use, fills every stored 16x16 block with values that name their place, expands them as
// debug_solve does (expand_solved) and prints the dense matrix and plan[].  Host code only; built plain and with
// -fsanitize=address,undefined.
//   ldlt_host sim3 <n_v> <fixed vertex> <loop from> <loop to>   a Sim3 pose graph: the chain k -- k-1 and one loop edge
//   ldlt_host band <n_kf> <width>                                keyframe blocks adjacent up to <width> apart
// Entry (r, c) of stored block t holds 1 + 256 t + 16 r + c; the upper triangle of a diagonal block, which the solver
// never reads, holds the poison value -1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../openmavis_amd/csrc/essgraph_plan.h"
#include "../../openmavis_amd/csrc/omv_ldlt_host.h"

using omv_lba_plan::LbaPlan;

static void line(const char *name, const std::vector<int> &v) {
    printf("%s", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

static int expand_and_print(const LbaPlan &L) {
    std::vector<double> blocks((size_t)L.n_slots * 256);
    for (int t = 0; t < L.n_slots; ++t)
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c < 16; ++c) {
                const bool unread = L.slot_kr[t] == L.slot_kc[t] && c > r;
                // the kernels' layout written out here, not through the header's sw16
                blocks[(size_t)t * 256 + 16 * r + (c ^ r)] = unread ? -1.0 : 1.0 + 256 * t + 16 * r + c;
            }
    const size_t n = 16 * (size_t)L.nb;
    std::vector<double> S(n * n, -7.0);   // expand_solved writes every entry
    std::vector<int32_t> plan(4 + L.n_lev, -1);
    omv_ldlt_host::expand_solved(blocks.data(), L.slot_kr.data(), L.slot_kc.data(), L.lev_start.data(), L.nb, L.n_slots,
                                 L.n_lds, L.n_lev, L.use_lds, S.data(), plan.data());
    printf("scalars %d %d %d %d %d\n", L.nb, L.n_slots, L.n_lds, L.n_lev, L.use_lds);
    line("slot_kr", L.slot_kr), line("slot_kc", L.slot_kc), line("plan", std::vector<int>(plan.begin(), plan.end()));
    printf("S");
    for (double v : S) printf(" %.0f", v);
    printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "sim3")) {
        const int n = atoi(argv[2]), fix = atoi(argv[3]), la = atoi(argv[4]), lb = atoi(argv[5]);
        std::vector<uint8_t> fixed(n, 0);
        fixed[fix] = 1;
        std::vector<int32_t> ei, ej, et;
        for (int k = 1; k < n; ++k) ei.push_back(k), ej.push_back(k - 1), et.push_back(1);
        ei.push_back(la), ej.push_back(lb), et.push_back(0);
        omv_essgraph_plan::EssPlan P;
        if (omv_essgraph_plan::plan_essgraph(OMV_ESSGRAPH_SIM3, n, fixed.data(), (int)ei.size(), ei.data(), ej.data(), et.data(),
                                             omv_essgraph_plan::EssLimits{n, (int)ei.size()}, true, P) != OMV_OK)
            return 3;
        // the blocks an edge joins (its two vertices' blocks, -1 for the fixed one): a stored block without one is fill
        std::vector<int> eb;
        for (size_t e = 0; e < ei.size(); ++e)
            for (int v : {ei[e], ej[e]}) eb.push_back(P.row_of[v] < 0 ? -1 : P.row_of[v] / 16);
        line("edge_blocks", eb);
        return expand_and_print(P.L);
    }
    if (argc == 4 && !strcmp(argv[1], "band")) {
        const int nb = atoi(argv[2]), width = atoi(argv[3]);
        std::vector<uint8_t> adj((size_t)nb * nb, 0);
        std::vector<int> eb;
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j < i; ++j)
                if (i - j <= width) adj[(size_t)i * nb + j] = adj[(size_t)j * nb + i] = 1, eb.push_back(i), eb.push_back(j);
        line("edge_blocks", eb);
        LbaPlan L;
        omv_lba_plan::PlanWork W;
        L.nb = nb, L.n_red = 16 * nb;
        L.perm = omv_lba_plan::plan_order(nb, adj, std::max(omv_lba_plan::lds_slot_budget(true, L.n_red), 1));
        omv_lba_plan::plan_schedule(nb, adj, L, W);
        omv_lba_plan::plan_lds(true, L);
        return expand_and_print(L);
    }
    return 2;
}
