// A plain C++ consumer of omv_adapt::OptimizeSim3 (include/omv_adapters.hpp) with the call shape of LoopClosing's three
// call sites (src/LoopClosing.cc:658, :899, :935): vpMatches1-style vector in / out, g2oS12 in / out, th2, bFixScale and
// the mAcumHessian the reference leaves zero.  The job comes from a file the test writes (little-endian, in this order):
//   int32 N, mN1, model1, model2, fix_scale; float th2, pose1[12], pose2[12], cam1[8], cam2[8]; double q[4], t[3], s;
//   int32 index1[N]; float Xw1[3N], Xw2[3N], obs1[2N], obs2[2N], inv_sigma2_1[N], inv_sigma2_2[N]; uint8 has_kp2[N]
// Prints one line
//   nIn <n> status <one digit per entry> matches <vpMatches1 as 0/1> q <4> t <3> s <1> (the doubles as %.17g)
// and exits 0 when the call succeeded and mAcumHessian is zero.
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
        std::fprintf(stderr, "usage: optimize_sim3_consumer JOB_FILE\n");
        return 2;
    }
    try {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) throw omv_adapt::Error("cannot open the job file");
        int32_t hd[5];
        float th2 = 0.f;
        omv_adapt::OptimizeSim3Input in;
        omv_adapt::Sim3 S;
        bool ok = rd(f, hd, 5) && rd(f, &th2, 1) && rd(f, in.pose1, 12) && rd(f, in.pose2, 12) && rd(f, in.cam1, 8) &&
                  rd(f, in.cam2, 8) && rd(f, S.q, 4) && rd(f, S.t, 3) && rd(f, &S.s, 1);
        if (!ok || hd[0] < 0 || hd[1] < 0) throw omv_adapt::Error("bad job file header");
        const size_t N = (size_t)hd[0];
        in.model1 = hd[2], in.model2 = hd[3];
        in.index1.resize(N), in.Xw1.resize(3 * N), in.Xw2.resize(3 * N), in.obs1.resize(2 * N), in.obs2.resize(2 * N);
        in.inv_sigma2_1.resize(N), in.inv_sigma2_2.resize(N), in.has_kp2.resize(N);
        ok = rd(f, in.index1.data(), N) && rd(f, in.Xw1.data(), 3 * N) && rd(f, in.Xw2.data(), 3 * N) &&
             rd(f, in.obs1.data(), 2 * N) && rd(f, in.obs2.data(), 2 * N) && rd(f, in.inv_sigma2_1.data(), N) &&
             rd(f, in.inv_sigma2_2.data(), N) && rd(f, in.has_kp2.data(), N);
        std::fclose(f);
        if (!ok) throw omv_adapt::Error("short job file");
        std::vector<bool> vpMatches1((size_t)hd[1], false);
        for (size_t i = 0; i < N; i++) vpMatches1.at((size_t)in.index1[i]) = true;
        std::array<double, 49> mAcumHessian;
        mAcumHessian.fill(1.0);
        std::vector<uint8_t> status;
        const int nIn = omv_adapt::OptimizeSim3(in, vpMatches1, S, th2, hd[4] != 0, mAcumHessian, nullptr, nullptr, &status);
        std::printf("nIn %d status ", nIn);
        for (uint8_t s : status) std::printf("%d", (int)s);
        std::printf(" matches ");
        for (bool b : vpMatches1) std::printf("%d", (int)b);
        std::printf(" q %.17g %.17g %.17g %.17g t %.17g %.17g %.17g s %.17g\n", S.q[0], S.q[1], S.q[2], S.q[3], S.t[0],
                    S.t[1], S.t[2], S.s);
        for (double v : mAcumHessian)
            if (v != 0.0) return 1;
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "optimize_sim3_consumer: %s\n", e.what());
        return 2;
    }
}
