// A plain C++ consumer of omv_adapt::LocalBundleAdjustment (include/omv_adapters.hpp) with the call shape of
// LocalMapping::Run (src/LocalMapping.cc:171-177).  The window comes from a file the test writes (little-endian):
//   int32 C, K, n_opt, P, E, S, inertial_map; double fx, fy, cx, cy, bf;
//   float cam[8C]; int32 cam_model[C]; double q_c0[4C], t_c0[3C], q_cw[4K], t_cw[3K], pts[3P];
//   int32 mono_pt[E], mono_kf[E], mono_cam[E]; double mono_obs[2E]; float mono_inv_sigma2[E];
//   int32 stereo_pt[S], stereo_kf[S]; double stereo_obs[3S]; float stereo_inv_sigma2[S]
// Prints one line (the doubles as %.17g)
//   fixed <n> opt <n> mps <n> edges <n> it <n> tr <n> err <2> q <4K> t <3K> pts <3P> erase <2 per pair>
// and exits 0 when the call succeeded.
#include <cstdio>
#include <cstdlib>

#include "omv_adapters.hpp"

namespace {
template <typename T>
bool rd(std::FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: vba_consumer WINDOW_FILE\n");
        return 2;
    }
    try {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) throw omv_adapt::Error("cannot open the window file");
        int32_t hd[7];
        double pin[5];
        if (std::fread(hd, sizeof(int32_t), 7, f) != 7 || std::fread(pin, sizeof(double), 5, f) != 5)
            throw omv_adapt::Error("bad window file header");
        for (int32_t v : hd)
            if (v < 0) throw omv_adapt::Error("bad window file header");
        const size_t C = hd[0], K = hd[1], P = hd[3], E = hd[4], S = hd[5];
        omv_adapt::LocalBAView w;
        w.n_cams = hd[0], w.n_opt = hd[2], w.n_local = hd[2];
        w.fx = pin[0], w.fy = pin[1], w.cx = pin[2], w.cy = pin[3], w.bf = pin[4];
        const bool ok = rd(f, w.cam, 8 * C) && rd(f, w.cam_model, C) && rd(f, w.q_c0, 4 * C) && rd(f, w.t_c0, 3 * C) &&
                        rd(f, w.q_cw, 4 * K) && rd(f, w.t_cw, 3 * K) && rd(f, w.pts, 3 * P) && rd(f, w.mono_pt, E) &&
                        rd(f, w.mono_kf, E) && rd(f, w.mono_cam, E) && rd(f, w.mono_obs, 2 * E) &&
                        rd(f, w.mono_inv_sigma2, E) && rd(f, w.stereo_pt, S) && rd(f, w.stereo_kf, S) &&
                        rd(f, w.stereo_obs, 3 * S) && rd(f, w.stereo_inv_sigma2, S);
        std::fclose(f);
        if (!ok) throw omv_adapt::Error("short window file");
        bool stop = false;
        int num_fixedKF = 0, num_OptKF = 0, num_MPs = 0, num_edges = 0;
        omv_adapt::LocalBundleAdjustment(w, &stop, hd[6] != 0, num_fixedKF, num_OptKF, num_MPs, num_edges);
        std::printf("fixed %d opt %d mps %d edges %d it %d tr %d err %.17g %.17g q", num_fixedKF, num_OptKF, num_MPs,
                    num_edges, w.iterations, w.trials, w.err, w.err_end);
        for (double v : w.q_cw) std::printf(" %.17g", v);
        std::printf(" t");
        for (double v : w.t_cw) std::printf(" %.17g", v);
        std::printf(" pts");
        for (double v : w.pts) std::printf(" %.17g", v);
        std::printf(" erase");
        for (const auto &e : w.vToErase) std::printf(" %d %d", e.first, e.second);
        std::printf("\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "vba_consumer: %s\n", e.what());
        return 2;
    }
}
