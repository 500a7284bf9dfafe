// The host plan of a FullInertialBA problem (openmavis_amd/csrc/lba_plan.h: plan_fiba) as a stand-alone program, built by
// tests/test_fiba_plan_cpu.py with -fsanitize=address,undefined.  The problems are made here: K keyframes in mnId order,
// an inertial chain, and landmarks seen by three consecutive keyframes (a three-keyframe covisibility band).
//   fiba_plan_host plan K fix_last shared no_imu_first break_at [lds_ok]   the plan's arrays as text, one per line
//   fiba_plan_host big K                                          n_big with one more landmark seen by all K keyframes
//   fiba_plan_host reject                                         the status of each problem the planner must reject
//   fiba_plan_host time K                                         planning milliseconds: every cut / the bounded cuts
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../openmavis_amd/csrc/lba_plan.h"

using namespace omv_lba_plan;

struct Problem {
    std::vector<float> cam, preint, w;
    std::vector<double> R, t3, Rc, tc, pts, obs;
    std::vector<uint8_t> imu;
    std::vector<int32_t> pt, kf, camid, k1, k2;
    omv_lba_problem p{};
};

// pts_per_kf landmarks start at every keyframe k and are seen by k, k + 1, k + 2 (where they exist)
static void make(Problem &q, int K, bool fix_last, bool no_imu_first, int break_at, int pts_per_kf = 2) {
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    q.cam.assign(8, 0.f), q.cam[0] = q.cam[1] = 300.f, q.cam[2] = q.cam[3] = 200.f;
    q.R.clear(), q.t3.assign(3 * (size_t)K, 0.0), q.Rc.clear(), q.tc.assign(3 * (size_t)K, 0.0);
    for (int k = 0; k < K; ++k) q.R.insert(q.R.end(), I3, I3 + 9), q.Rc.insert(q.Rc.end(), I3, I3 + 9);
    q.imu.assign(K, 1);
    if (no_imu_first && K > 0) q.imu[0] = 0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < pts_per_kf; ++j) {
            const int p = (int)q.pts.size() / 3;
            q.pts.insert(q.pts.end(), {0.1 * k, 0.2 * j, 5.0});
            for (int d = 0; d < 3 && k + d < K; ++d) {
                q.pt.push_back(p), q.kf.push_back(k + d), q.camid.push_back(0);
                q.obs.insert(q.obs.end(), {200.0, 200.0});
                q.w.push_back(1.f);
            }
        }
    for (int k = 1; k < K; ++k) {
        if (k == break_at || !q.imu[k - 1] || !q.imu[k]) continue;   // no mPrevKF / not between two bImu keyframes
        q.k1.push_back(k - 1), q.k2.push_back(k);
        std::vector<float> pre(OMV_PREINT_FLOATS, 0.f);
        for (int d = 0; d < 15; ++d) pre[kPreintCov + 16 * d] = 1e-4f * (1 + d);
        q.preint.insert(q.preint.end(), pre.begin(), pre.end());
    }
    omv_lba_problem &p = q.p;
    p.n_cams = 1, p.cam = q.cam.data(), p.Rcb = p.Rbc = q.R.data(), p.tcb = p.tbc = q.t3.data();   // one camera: identity
    p.n_kf = K, p.n_opt = fix_last ? K - 1 : K, p.kf_imu = q.imu.data();
    p.Rwb = q.R.data(), p.twb = q.t3.data(), p.Rcw = q.Rc.data(), p.tcw = q.tc.data();
    p.vel = p.bg = p.ba = q.t3.data();
    p.n_pts = (int)q.pts.size() / 3, p.pts = q.pts.data();
    p.n_mono = (int)q.pt.size(), p.mono_pt = q.pt.data(), p.mono_kf = q.kf.data(), p.mono_cam = q.camid.data();
    p.mono_obs = q.obs.data(), p.mono_inv_sigma2 = q.w.data();
    p.n_imu = (int)q.k1.size(), p.imu_kf1 = q.k1.data(), p.imu_kf2 = q.k2.data(), p.preint = q.preint.data();
}

static LbaLimits limits_of(const omv_lba_problem &p) {
    return LbaLimits{p.n_kf, p.n_cams, p.n_pts, p.n_mono + (p.n_stereo > 0 ? p.n_stereo : 0), p.n_imu > 0 ? p.n_imu : 1};
}

template <typename T>
static void line(const char *name, const std::vector<T> &v) {
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %d", (int)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan" && (argc == 7 || argc == 8)) {
        Problem q;
        const bool shared = std::atoi(argv[4]) != 0;
        make(q, std::atoi(argv[2]), std::atoi(argv[3]) != 0, std::atoi(argv[5]) != 0, std::atoi(argv[6]));
        LbaPlan P;
        const bool lds_ok = argc < 8 || std::atoi(argv[7]) != 0;
        const omv_status st = plan_fiba(q.p, shared, 1e2, 1e5, limits_of(q.p), lds_ok, P);
        std::printf("status %d\n", (int)st);
        if (st != OMV_OK) return 0;
        std::printf("scalars %d %d %d %d %d %d %d\n", P.nb, P.shared_blk, P.shared_kf, P.n_red, P.n_slots, P.n_lev, P.use_lds);
        line("perm", P.perm), line("slot_kr", P.slot_kr), line("slot_kc", P.slot_kc);
        line("offV", P.offV), line("offG", P.offG), line("offA", P.offA);
        line("ib_start", P.ib_start), line("iv_start", P.iv_start);
        std::vector<int> ib, iv;
        for (const Int4 &e : P.imu_blk) ib.insert(ib.end(), {e.x, e.y, e.z});
        for (const Int2 &e : P.imu_vec) iv.insert(iv.end(), {e.x, e.y});
        line("imu_blk", ib), line("imu_vec", iv);
        line("imu_kf1", q.k1), line("imu_kf2", q.k2), line("rhs_start", P.rhs_start), line("lev_start", P.lev_start);
        std::printf("storage %d %d %d\n", P.n_lds, P.blob_ints, (int)P.ldlt_lds);
        double rw = 0;
        for (double x : P.infoG) rw += x * x;
        for (double x : P.infoA) rw += x * x;
        std::printf("rw_info_zero %d\n", rw == 0.0 ? 1 : 0);
        return 0;
    }
    if (mode == "big" && argc == 3) {   // a landmark on every keyframe: past kGrpW optimisable keyframes it is a group of its own
        Problem q;
        const int K = std::atoi(argv[2]);
        make(q, K, false, false, -1);
        const int p = (int)q.pts.size() / 3;
        q.pts.insert(q.pts.end(), {1.0, 1.0, 6.0});
        for (int k = 0; k < K; ++k) {
            q.pt.push_back(p), q.kf.push_back(k), q.camid.push_back(0);
            q.obs.insert(q.obs.end(), {210.0, 190.0});
            q.w.push_back(1.f);
        }
        q.p.n_pts = p + 1, q.p.pts = q.pts.data(), q.p.n_mono = (int)q.pt.size(), q.p.mono_pt = q.pt.data();
        q.p.mono_kf = q.kf.data(), q.p.mono_cam = q.camid.data(), q.p.mono_obs = q.obs.data(), q.p.mono_inv_sigma2 = q.w.data();
        LbaPlan P;
        const omv_status st = plan_fiba(q.p, true, 1e2, 1e5, limits_of(q.p), true, P);
        std::printf("status %d\nn_big %d\nkGrpW %d\n", (int)st, P.n_big, kGrpW);
        return 0;
    }
    if (mode == "reject") {
        LbaPlan P;
        {   // shared_bias with no bImu keyframe (and so no inertial edge)
            Problem q;
            make(q, 6, false, false, -1);
            q.imu.assign(6, 0), q.p.n_imu = 0;
            std::printf("no_imu_kf %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, limits_of(q.p), true, P));
            std::printf("no_imu_kf_per_kf_form %d\n", (int)plan_fiba(q.p, false, 0, 0, limits_of(q.p), true, P));
        }
        {   // bImu keyframes, but no inertial edge: the pair would hang on its priors alone
            Problem q;
            make(q, 6, false, false, -1);
            q.p.n_imu = 0;
            std::printf("no_imu_edge %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, limits_of(q.p), true, P));
        }
        {   // an inertial edge on a keyframe that is not bImu
            Problem q;
            make(q, 6, false, false, -1);
            q.imu[2] = 0;
            std::printf("edge_on_non_imu %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, limits_of(q.p), true, P));
        }
        {   // a negative prior, a NaN prior
            Problem q;
            make(q, 6, false, false, -1);
            std::printf("negative_prior_g %d\n", (int)plan_fiba(q.p, true, -1.0, 1e5, limits_of(q.p), true, P));
            std::printf("negative_prior_a %d\n", (int)plan_fiba(q.p, true, 1e2, -1e-3, limits_of(q.p), true, P));
            std::printf("nan_prior %d\n", (int)plan_fiba(q.p, true, std::nan(""), 1e5, limits_of(q.p), true, P));
            std::printf("negative_prior_unread %d\n", (int)plan_fiba(q.p, false, -1.0, -1.0, limits_of(q.p), true, P));
        }
        {   // (not rejected: more inertial edges than one block has threads, and more than the handle was made for)
            Problem q;
            make(q, 300, false, false, -1, 1);
            std::printf("many_imu_edges %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, limits_of(q.p), true, P));
            LbaLimits lim = limits_of(q.p);
            lim.max_imu = 298;
            std::printf("over_max_imu %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, lim, true, P));
        }
        {   // n_kf > max_kf
            Problem q;
            make(q, 6, false, false, -1);
            LbaLimits lim = limits_of(q.p);
            lim.max_kf = 5;
            std::printf("over_capacity %d\n", (int)plan_fiba(q.p, true, 1e2, 1e5, lim, true, P));
        }
        return 0;
    }
    if (mode == "time" && argc == 3) {
        Problem q;
        make(q, std::atoi(argv[2]), false, false, -1, 8);
        for (int bounded = 0; bounded < 2; ++bounded) {
            LbaPlan P;
            const auto t0 = std::chrono::steady_clock::now();
            const omv_status st = plan_problem(q.p, 0, 1, limits_of(q.p), true, true, true, bounded ? kFibaCuts : 0, P);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::printf("%s status %d ms %.2f n_slots %d n_lev %d use_lds %d\n", bounded ? "bounded" : "every_cut", (int)st, ms,
                        P.n_slots, P.n_lev, P.use_lds);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: fiba_plan_host plan K fix_last shared no_imu_first break_at | reject | time K\n");
    return 2;
}
