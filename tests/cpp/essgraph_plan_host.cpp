// Stand-alone host program over openmavis_amd/csrc/essgraph_plan.h (and lba_plan.h beneath it) for
// tests/test_essgraph_plan_cpu.py: plans a synthetic pose graph and prints the plan, the rejected problems' statuses, or
// the planning time of a large graph.  Host code only; built plain and with -fsanitize=address,undefined.
//   essgraph_plan_host plan <kind> <n_v> <lds_ok> <n_fixed> [offset ...]
//   essgraph_plan_host reject
//   essgraph_plan_host time <kind> <n_v>
// The graph: vertex k has an edge to k - 1 and to k - offset for every offset, the last vertex one to vertex 0, and the
// pair (1, 0) a second, parallel edge; the first n_fixed vertices are fixed, and so is vertex n_v / 2 when n_fixed > 1
// (a second fixed set) -- with an edge between vertices 0 and 1 then fixed-fixed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../openmavis_amd/csrc/essgraph_plan.h"

using namespace omv_essgraph_plan;

struct Graph {
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ei, ej, et;
};

static Graph make(int n, int n_fixed, const std::vector<int> &offs) {
    Graph g;
    g.fixed.assign(n, 0);
    for (int k = 0; k < n_fixed && k < n; ++k) g.fixed[k] = 1;
    if (n_fixed > 1 && n > 4) g.fixed[n / 2] = 1;
    auto add = [&](int i, int j, int t) { g.ei.push_back(i), g.ej.push_back(j), g.et.push_back(t); };
    if (n > 2) add(n - 1, 0, 0);
    for (int k = 1; k < n; ++k) {
        add(k, k - 1, 1);
        if (k == 1) add(1, 0, 1);   // the parallel pair
        for (int o : offs)
            if (k - o >= 0) add(k, k - o, 1);
    }
    return g;
}

template <class T>
static void line(const char *name, const std::vector<T> &v) {
    printf("%s", name);
    for (const auto &x : v) printf(" %d", (int)x);
    printf("\n");
}
static void line4(const char *name, const std::vector<Int4> &v) {
    printf("%s", name);
    for (const Int4 &x : v) printf(" %d %d %d %d", x.x, x.y, x.z, x.w);
    printf("\n");
}

static omv_status plan_of(int kind, const Graph &g, int max_v, int max_e, bool lds_ok, EssPlan &P) {
    return plan_essgraph(kind, (int)g.fixed.size(), g.fixed.data(), (int)g.ei.size(), g.ei.data(), g.ej.data(), g.et.data(),
                         EssLimits{max_v, max_e}, lds_ok, P);
}

int main(int argc, char **argv) {
    if (argc >= 6 && !strcmp(argv[1], "plan")) {
        const int kind = atoi(argv[2]), n = atoi(argv[3]), lds_ok = atoi(argv[4]), n_fixed = atoi(argv[5]);
        std::vector<int> offs;
        for (int a = 6; a < argc; ++a) offs.push_back(atoi(argv[a]));
        const Graph g = make(n, n_fixed, offs);
        EssPlan P;
        const omv_status rs = plan_of(kind, g, n, (int)g.ei.size(), lds_ok != 0, P);
        printf("status %d\n", (int)rs);
        if (rs != OMV_OK) return 0;
        const LbaPlan &L = P.L;
        printf("scalars %d %d %d %d %d %d %d %d %d %d\n", P.dim, P.per_blk, P.n_opt, L.nb, L.n_red, L.n_slots, L.n_lev,
               L.use_lds, L.n_lds, L.blob_ints);
        line("edge_i", g.ei), line("edge_j", g.ej), line("fixed", g.fixed);
        line("opt_v", P.opt_v), line("row_of", P.row_of), line("real_row", P.real_row), line("perm", L.perm);
        line("slot_kr", L.slot_kr), line("slot_kc", L.slot_kc), line("lev_start", L.lev_start), line("lev_col", L.lev_col);
        line("cb_start", P.cb_start), line4("cb", P.cb), line("cv_start", P.cv_start), line4("cv", P.cv);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "reject")) {
        EssPlan P;
        const Graph ok = make(6, 1, {});
        auto with = [&](auto &&change, int max_v = 6, int max_e = 64) {
            Graph g = ok;
            change(g);
            return (int)plan_of(OMV_ESSGRAPH_SIM3, g, max_v, max_e, true, P);
        };
        printf("ok %d\n", with([](Graph &) {}));
        printf("vertex_out_of_range %d\n", with([](Graph &g) { g.ej[2] = 6; }));
        printf("negative_vertex %d\n", with([](Graph &g) { g.ei[1] = -1; }));
        printf("self_edge %d\n", with([](Graph &g) { g.ej[3] = g.ei[3]; }));
        printf("bad_table %d\n", with([](Graph &g) { g.et[0] = 2; }));
        printf("all_fixed %d\n", with([](Graph &g) { g.fixed.assign(g.fixed.size(), 1); }));
        printf("over_max_vertices %d\n", with([](Graph &) {}, 5));
        printf("over_max_edges %d\n", with([](Graph &) {}, 6, 3));
        printf("no_edges %d\n", with([](Graph &g) { g.ei.clear(), g.ej.clear(), g.et.clear(); }));
        printf("bad_kind %d\n", (int)plan_of(7, ok, 6, 64, true, P));
        printf("null_fixed %d\n", (int)plan_essgraph(OMV_ESSGRAPH_SIM3, 6, nullptr, 0, nullptr, nullptr, nullptr, EssLimits{6, 64},
                                                   true, P));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "time")) {
        const int kind = atoi(argv[2]), n = atoi(argv[3]);
        const Graph g = make(n, 1, {2, 3, 9});
        EssPlan P;
        const auto t0 = std::chrono::steady_clock::now();
        const omv_status rs = plan_of(kind, g, n, (int)g.ei.size(), true, P);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("status %d\nplan_ms %.3f\nscalars %d %d %d %d\n", (int)rs, ms, P.L.nb, P.L.n_slots, P.L.n_lev, P.L.use_lds);
        return 0;
    }
    return 2;
}
