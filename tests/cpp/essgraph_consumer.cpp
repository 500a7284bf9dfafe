// A plain C++ (g++) consumer of omv_adapt::OptimizeEssentialGraph / OptimizeEssentialGraph4DoF (include/omv_adapters.hpp):
// reads a flattened pose graph, runs the adapter and prints the result at full precision, for
// tests/test_essgraph_consumer_gpu.py to compare with the Python call bit for bit.
//   essgraph_consumer graph.bin
// graph.bin: int32 [kind, n, E, m, fix_scale], then vScw [n][8], vSnc [n][8] (f64), fixed [n] (u8), edge_i, edge_j,
// edge_table [E] (i32), pose4 [n][24], Rcb [9], tcb [3] (f64; 4DoF only), points [m][3] (f32), point_ref [m] (i32).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "omv_adapters.hpp"

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (fread(hd, sizeof(int32_t), 5, f) != 5) return 2;
    const int kind = hd[0];
    const size_t n = hd[1], E = hd[2], m = hd[3];
    omv_adapt::EssentialGraphInput g;
    bool ok = rd(f, g.vScw, 8 * n) && rd(f, g.vSnc, 8 * n) && rd(f, g.fixed, n) && rd(f, g.edge_i, E) && rd(f, g.edge_j, E) &&
              rd(f, g.edge_table, E);
    if (ok && kind == OMV_ESSGRAPH_4DOF) {
        std::vector<double> rig;
        ok = rd(f, g.pose4, 24 * n) && rd(f, rig, 12);
        for (int q = 0; ok && q < 9; ++q) g.Rcb[q] = rig[q];
        for (int q = 0; ok && q < 3; ++q) g.tcb[q] = rig[9 + q];
    }
    ok = ok && rd(f, g.points, 3 * m) && rd(f, g.point_ref, m);
    fclose(f);
    if (!ok) return 2;
    try {
        if (kind == OMV_ESSGRAPH_SIM3) omv_adapt::OptimizeEssentialGraph(g, hd[4] != 0);
        else omv_adapt::OptimizeEssentialGraph4DoF(g);
    } catch (const omv_adapt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("it %d tr %d fail %d err %.17g %.17g\n", g.iterations, g.trials, g.solver_failed, g.err, g.err_end);
    printf("vertices");
    for (double v : g.vertices) printf(" %.17g", v);
    printf("\nposes");
    for (float v : g.poses) printf(" %.9g", v);
    printf("\npoints");
    for (float v : g.points) printf(" %.9g", v);
    printf("\n");
    return 0;
}
