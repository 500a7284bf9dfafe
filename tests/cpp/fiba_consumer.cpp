// A plain C++ consumer of omv_adapt::FullInertialBA (include/omv_adapters.hpp) with the call shape of
// LocalMapping::InitializeIMU (src/LocalMapping.cc:1398-1406).  The map comes from a file the test writes (little-endian):
//   int32 C, K, P, E, S, NI, its, bFixLocal, bInit; float bf, priorG, priorA; double bg0[3], ba0[3];
//   float cam[8C]; int32 cam_model[C]; double Rcb[9C], tcb[3C], Rbc[9C], tbc[3C]; uint8 kf_imu[K];
//   double Rwb[9K], twb[3K], Rcw[9KC], tcw[3KC], vel[3K], bg[3K], ba[3K], pts[3P];
//   int32 mono_pt[E], mono_kf[E], mono_cam[E]; double mono_obs[2E]; float mono_inv_sigma2[E];
//   int32 stereo_pt[S], stereo_kf[S]; double stereo_obs[3S]; float stereo_inv_sigma2[S];
//   int32 imu_kf1[NI], imu_kf2[NI]; float preint[292 NI]
// Prints one line (the doubles as %.17g)
//   ran <0|1> it <n> tr <n> err <2> not_included <n> Rwb <9K> twb <3K> vel <3K> bg <3K> ba <3K> pts <3P>
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
void put(const char *name, const std::vector<double> &v) {
    std::printf(" %s", name);
    for (double x : v) std::printf(" %.17g", x);
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: fiba_consumer MAP_FILE\n");
        return 2;
    }
    try {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) throw omv_adapt::Error("cannot open the map file");
        int32_t hd[9];
        float fl[3];
        double b0[6];
        if (std::fread(hd, sizeof(int32_t), 9, f) != 9 || std::fread(fl, sizeof(float), 3, f) != 3 ||
            std::fread(b0, sizeof(double), 6, f) != 6)
            throw omv_adapt::Error("bad map file header");
        for (int32_t v : hd)
            if (v < 0) throw omv_adapt::Error("bad map file header");
        const size_t C = hd[0], K = hd[1], P = hd[2], E = hd[3], S = hd[4], NI = hd[5];
        omv_adapt::FullInertialMap m;
        m.n_cams = hd[0], m.bf = fl[0];
        for (int q = 0; q < 3; ++q) m.bg0[q] = b0[q], m.ba0[q] = b0[3 + q];
        const bool ok = rd(f, m.cam, 8 * C) && rd(f, m.cam_model, C) && rd(f, m.Rcb, 9 * C) && rd(f, m.tcb, 3 * C) &&
                        rd(f, m.Rbc, 9 * C) && rd(f, m.tbc, 3 * C) && rd(f, m.kf_imu, K) && rd(f, m.Rwb, 9 * K) &&
                        rd(f, m.twb, 3 * K) && rd(f, m.Rcw, 9 * K * C) && rd(f, m.tcw, 3 * K * C) && rd(f, m.vel, 3 * K) &&
                        rd(f, m.bg, 3 * K) && rd(f, m.ba, 3 * K) && rd(f, m.pts, 3 * P) && rd(f, m.mono_pt, E) &&
                        rd(f, m.mono_kf, E) && rd(f, m.mono_cam, E) && rd(f, m.mono_obs, 2 * E) &&
                        rd(f, m.mono_inv_sigma2, E) && rd(f, m.stereo_pt, S) && rd(f, m.stereo_kf, S) &&
                        rd(f, m.stereo_obs, 3 * S) && rd(f, m.stereo_inv_sigma2, S) && rd(f, m.imu_kf1, NI) &&
                        rd(f, m.imu_kf2, NI) && rd(f, m.preint, (size_t)OMV_PREINT_FLOATS * NI);
        std::fclose(f);
        if (!ok) throw omv_adapt::Error("short map file");
        bool stop = false;
        const bool ran = omv_adapt::FullInertialBA(m, hd[6], hd[7] != 0, &stop, hd[8] != 0, fl[1], fl[2]);
        int not_included = 0;
        for (uint8_t v : m.pt_not_included) not_included += v;
        std::printf("ran %d it %d tr %d err %.17g %.17g not_included %d", ran ? 1 : 0, m.iterations, m.trials, m.err, m.err_end,
                    not_included);
        put("Rwb", m.Rwb), put("twb", m.twb), put("vel", m.vel), put("bg", m.bg), put("ba", m.ba), put("pts", m.pts);
        std::printf("\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "fiba_consumer: %s\n", e.what());
        return 2;
    }
}
