// A plain C++ consumer of omv_adapt::MLPnPsolver (include/omv_adapters.hpp) with the call shape of
// Tracking::Relocalization (src/Tracking.cc:3543-3730): MLPnPsolver(F, vpMapPointMatches),
// SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991), then iterate(5, bNoMore, vbInliers, nInliers, Tcw).
// The frame is made here: a planted pose seen by a pinhole camera, 0.3 px noise, 20 % gross outliers (the 35 hypotheses
// of these parameters then hold a sample of six inliers whatever rand() returns: the HIP runtime's start-up may call it
// too), and entries of vpMapPointMatches without a map point or with a bad one.  Prints one line
//   found <0|1> no_more <0|1> inliers <n> kept <N> max_its <k> rot_err <rad> trans_err <m> outliers_accepted <n>
// and exits 0 when the planted pose is recovered and no planted outlier is accepted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "omv_adapters.hpp"

int main() {
    try {
        std::mt19937 rng(11);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        std::normal_distribution<float> G(0.f, 1.f);
        const int mN = 260, n_keys = 250;
        const float fx = 380.f, cx = 360.f, cy = 270.f;
        const float a = 0.25f, tcw[3] = {0.2f, -0.1f, 0.3f};   // rotation about y
        const float Rcw[9] = {std::cos(a), 0.f, std::sin(a), 0.f, 1.f, 0.f, -std::sin(a), 0.f, std::cos(a)};
        omv_adapt::MLPnPInput in;
        in.n_keys = n_keys, in.model = OMV_CAM_PINHOLE;
        const float cam[8] = {fx, fx, cx, cy, 0, 0, 0, 0};
        for (int k = 0; k < 8; k++) in.cam[k] = cam[k];
        std::vector<uint8_t> outlier(mN, 0);
        for (int i = 0; i < mN; i++) {
            const float z = 2.f + 6.f * U(rng);
            const float u = 40.f + 640.f * U(rng), v = 40.f + 460.f * U(rng);
            const float Xc[3] = {(u - cx) / fx * z - tcw[0], (v - cy) / fx * z - tcw[1], z - tcw[2]};
            for (int r = 0; r < 3; r++)   // Xw = Rcw^T (Xc - tcw)
                in.Xw.push_back(Rcw[r] * Xc[0] + Rcw[3 + r] * Xc[1] + Rcw[6 + r] * Xc[2]);
            outlier[i] = U(rng) < 0.2f;
            in.P2D.push_back(outlier[i] ? 20.f + 680.f * U(rng) : u + 0.3f * G(rng));
            in.P2D.push_back(outlier[i] ? 20.f + 500.f * U(rng) : v + 0.3f * G(rng));
            in.sigma2.push_back(i % 2 ? 1.44f : 1.f);
            in.has_mp.push_back(i % 5 != 4);
            in.is_bad.push_back(i % 17 == 3);
        }
        std::srand(1);
        omv_adapt::MLPnPsolver solver(in);
        solver.SetRansacParameters(0.99, 10, 300, 6, 0.5f, 5.991f);
        bool bNoMore = false;
        std::vector<bool> vbInliers;
        int nInliers = 0;
        std::array<float, 16> Tcw{};
        const bool found = solver.iterate(5, bNoMore, vbInliers, nInliers, Tcw);
        const float tr = Tcw[0] * Rcw[0] + Tcw[1] * Rcw[1] + Tcw[2] * Rcw[2] + Tcw[4] * Rcw[3] + Tcw[5] * Rcw[4] +
                         Tcw[6] * Rcw[5] + Tcw[8] * Rcw[6] + Tcw[9] * Rcw[7] + Tcw[10] * Rcw[8];
        const float rot_err = std::acos(std::fmin(1.f, std::fmax(-1.f, (tr - 1.f) / 2.f)));
        const float trans_err = std::sqrt((Tcw[3] - tcw[0]) * (Tcw[3] - tcw[0]) + (Tcw[7] - tcw[1]) * (Tcw[7] - tcw[1]) +
                                          (Tcw[11] - tcw[2]) * (Tcw[11] - tcw[2]));
        int n_true = 0, n_out = 0, n_unkept = 0;
        for (int i = 0; i < (int)vbInliers.size(); i++) {
            n_true += vbInliers[i], n_out += vbInliers[i] && outlier[i];
            n_unkept += vbInliers[i] && (i >= n_keys || !in.has_mp[i] || in.is_bad[i]);
        }
        const int kept = (int)solver.key_point_indices().size();
        std::printf("found %d no_more %d inliers %d kept %d max_its %d rot_err %g trans_err %g outliers_accepted %d\n",
                    (int)found, (int)bNoMore, nInliers, kept, solver.ransac_max_its(), rot_err, trans_err, n_out);
        const bool ok = found && nInliers > solver.ransac_min_inliers() && n_true == nInliers &&
                        (int)vbInliers.size() == mN && n_out == 0 && n_unkept == 0 && rot_err < 0.01f &&
                        trans_err < 0.05f && Tcw[15] == 1.f && solver.ransac_min_inliers() == (int)(kept * 0.5f);
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mlpnp_consumer: %s\n", e.what());
        return 2;
    }
}
