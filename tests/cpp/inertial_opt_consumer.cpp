// A plain C++ consumer of omv_adapt::InertialOptimization (include/omv_adapters.hpp) with the call shapes of the
// reference's three overloads (src/LocalMapping.cc:1255-1517, :1548, src/LoopClosing.cc:2037).  The job comes from a file
// the test writes (little-endian, in this order):
//   int32 K, E, mode, mono; float priorG, priorA; double bg0[3], ba0[3], Rwg[9], scale;
//   double Rwb[9K], twb[3K], vel[3K]; float gyro_bias[3K]; int32 kf1[E], kf2[E]; float preint[292 E]
// Prints one line (the doubles as %.17g, the floats as %.9g)
//   it <n> tr <n> Rwg <9> scale <1> bg <3> ba <3> vel <3K> velf <3K> re <one digit per keyframe>
// and exits 0 when the call succeeded.
#include <cstdio>
#include <cstdlib>

#include "omv_adapters.hpp"

namespace {
template <typename T>
bool rd(std::FILE *f, T *p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: inertial_opt_consumer JOB_FILE\n");
        return 2;
    }
    try {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) throw omv_adapt::Error("cannot open the job file");
        int32_t hd[4];
        float prior[2];
        double Rwg[9], scale = 1.0, bg[3] = {0, 0, 0}, ba[3] = {0, 0, 0};
        omv_adapt::InertialMap m;
        bool ok = rd(f, hd, 4) && rd(f, prior, 2) && rd(f, m.bg0, 3) && rd(f, m.ba0, 3) && rd(f, Rwg, 9) && rd(f, &scale, 1);
        if (!ok || hd[0] < 0 || hd[1] < 0) throw omv_adapt::Error("bad job file header");
        const size_t K = (size_t)hd[0], E = (size_t)hd[1];
        m.Rwb.resize(9 * K), m.twb.resize(3 * K), m.vel.resize(3 * K), m.gyro_bias.resize(3 * K);
        m.kf1.resize(E), m.kf2.resize(E), m.preint.resize(E * OMV_PREINT_FLOATS);
        ok = rd(f, m.Rwb.data(), 9 * K) && rd(f, m.twb.data(), 3 * K) && rd(f, m.vel.data(), 3 * K) &&
             rd(f, m.gyro_bias.data(), 3 * K) && rd(f, m.kf1.data(), E) && rd(f, m.kf2.data(), E) &&
             rd(f, m.preint.data(), E * OMV_PREINT_FLOATS);
        std::fclose(f);
        if (!ok) throw omv_adapt::Error("short job file");
        if (hd[2] == OMV_INERTIAL_FULL) omv_adapt::InertialOptimization(m, Rwg, scale, bg, ba, hd[3] != 0, prior[0], prior[1]);
        else if (hd[2] == OMV_INERTIAL_BIAS) omv_adapt::InertialOptimization(m, bg, ba, prior[0], prior[1]);
        else omv_adapt::InertialOptimization(m, Rwg, scale);
        std::printf("it %d tr %d Rwg", m.iterations, m.trials);
        for (double v : Rwg) std::printf(" %.17g", v);
        std::printf(" scale %.17g bg %.17g %.17g %.17g ba %.17g %.17g %.17g vel", scale, bg[0], bg[1], bg[2], ba[0], ba[1],
                    ba[2]);
        for (double v : m.vel) std::printf(" %.17g", v);
        std::printf(" velf");
        for (float v : m.vel_f32) std::printf(" %.9g", (double)v);
        std::printf(" re ");
        for (uint8_t r : m.reintegrate) std::printf("%d", (int)r);
        std::printf("\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "inertial_opt_consumer: %s\n", e.what());
        return 2;
    }
}
