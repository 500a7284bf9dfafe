// A plain C++ consumer of omv_adapt::Sim3Solver (include/omv_adapters.hpp) with the call shape of
// LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:812-832): constructor, SetRansacParameters(0.99, n, 300),
// iterate(20, ...) until bConverge or bNoMore, then the GetEstimated* accessors; and find() on a fresh solver.
// The job is made here: a planted similarity between two pinhole cameras, 60 % inliers.  Prints one line
//   converged <0|1> inliers <n> iterations_calls <k> rot_err <rad> scale_err <rel> trans_err <m> find_inliers <n>
// and exits 0 when the planted similarity is recovered.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "omv_adapters.hpp"

int main() {
    try {
        std::mt19937 rng(7);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        std::normal_distribution<float> G(0.f, 1.f);
        const int N = 100, mN1 = 140;
        const float fx = 380.f, cx = 360.f, cy = 270.f;
        const float a = 0.2f, s12 = 1.15f, t12[3] = {0.3f, -0.2f, 0.1f};   // rotation about y
        const float R12[9] = {std::cos(a), 0.f, std::sin(a), 0.f, 1.f, 0.f, -std::sin(a), 0.f, std::cos(a)};
        omv_adapt::Sim3SolverInput in;
        in.mN1 = mN1, in.model1 = in.model2 = OMV_CAM_PINHOLE, in.fix_scale = false;
        const float cam[8] = {fx, fx, cx, cy, 0, 0, 0, 0};
        const float eye[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        for (int k = 0; k < 8; k++) in.cam1[k] = in.cam2[k] = cam[k];
        for (int k = 0; k < 12; k++) in.pose1[k] = in.pose2[k] = eye[k];   // world = camera frame on both sides
        in.pose2[9] = 0.5f;   // except a translation of camera 2, undone in the world points below
        for (int i = 0; i < N; i++) {
            const float z = 2.f + 13.f * U(rng);
            const float X2[3] = {(40.f + 640.f * U(rng) - cx) / fx * z, (40.f + 460.f * U(rng) - cy) / fx * z, z};
            float X1[3];
            for (int r = 0; r < 3; r++)
                X1[r] = s12 * (R12[3 * r] * X2[0] + R12[3 * r + 1] * X2[1] + R12[3 * r + 2] * X2[2]) + t12[r] +
                        G(rng) * z * 0.3f / fx;
            if (U(rng) > 0.6f) {   // a gross outlier
                const float zo = 2.f + 13.f * U(rng);
                X1[0] = (640.f * U(rng) - cx) / fx * zo, X1[1] = (460.f * U(rng) - cy) / fx * zo, X1[2] = zo;
            }
            for (int r = 0; r < 3; r++) in.Xw1.push_back(X1[r]), in.Xw2.push_back(X2[r] - (r == 0 ? 0.5f : 0.f));
            in.sigma2_1.push_back(1.44f), in.sigma2_2.push_back(1.f);
            in.index1.push_back(i + i / 3);   // holes in vpMatched12
        }
        std::srand(1);
        omv_adapt::Sim3Solver solver(in);
        solver.SetRansacParameters(0.99, 20, 300);
        bool bNoMore = false, bConverge = false;
        std::vector<bool> vbInliers;
        int nInliers = 0, calls = 0;
        std::array<float, 16> T{};
        while (!bConverge && !bNoMore) {
            T = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
            calls++;
        }
        const std::array<float, 9> R = solver.GetEstimatedRotation();
        const std::array<float, 3> t = solver.GetEstimatedTranslation();
        const float s = solver.GetEstimatedScale();
        const float tr = R[0] * R12[0] + R[1] * R12[1] + R[2] * R12[2] + R[3] * R12[3] + R[4] * R12[4] + R[5] * R12[5] +
                         R[6] * R12[6] + R[7] * R12[7] + R[8] * R12[8];
        const float rot_err = std::acos(std::fmin(1.f, std::fmax(-1.f, (tr - 1.f) / 2.f)));
        const float scale_err = std::fabs(s - s12) / s12;
        const float trans_err = std::sqrt((t[0] - t12[0]) * (t[0] - t12[0]) + (t[1] - t12[1]) * (t[1] - t12[1]) +
                                          (t[2] - t12[2]) * (t[2] - t12[2]));
        int n_true = 0;
        for (bool b : vbInliers) n_true += b;
        omv_adapt::Sim3Solver again(in);
        again.SetRansacParameters(0.99, 20, 300);
        std::vector<bool> vb2;
        int n2 = 0;
        const std::array<float, 16> T2 = again.find(vb2, n2);
        std::printf("converged %d inliers %d iterations_calls %d rot_err %g scale_err %g trans_err %g find_inliers %d\n",
                    (int)bConverge, nInliers, calls, rot_err, scale_err, trans_err, n2);
        const bool ok = bConverge && nInliers > 20 && n_true == nInliers && (int)vbInliers.size() == mN1 &&
                        rot_err < 0.02f && scale_err < 0.02f && trans_err < 0.3f && T[15] == 1.f && n2 > 20 && T2[15] == 1.f;
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "sim3_solver_consumer: %s\n", e.what());
        return 2;
    }
}
