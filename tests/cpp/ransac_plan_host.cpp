// Stand-alone host program over openmavis_amd/csrc/ransac_plan.h (no HIP, no device): reads one case per line from
// standard input and prints one line per case.  Built with -fsanitize=address,undefined by
// tests/test_ransac_plan_cpu.py, which writes the cases and compares the lines with its own expectations.
//   its prob min_inliers n max_its                      -> "its <mRansacMaxIts>" as omv_sim3_solver_set computes it
//   pnp n prob min_inliers max_its min_set epsilon      -> "pnp <mRansacMaxIts> <mRansacMinInliers>"
//   layout max_jobs max_corr words_cap bad_job nulls n_jobs corr_start[n_jobs + 1] mN[n_jobs] index[n_corr]
//       words_cap < 0: words_cap(max_corr, max_jobs); bad_job: the job whose camera model is unknown, or -1; nulls:
//       1 corr_start, 2 mN, 4 the per-correspondence arrays.
//       -> "status <s>", then on OMV_OK " | inl_start | word_start | words_total | corr_job"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../openmavis_amd/csrc/ransac_plan.h"

namespace {

void layout(std::istringstream &in) {
    int max_jobs, max_corr, cap, bad_job, nulls, n_jobs;
    in >> max_jobs >> max_corr >> cap >> bad_job >> nulls >> n_jobs;
    std::vector<int32_t> corr_start(n_jobs > 0 ? n_jobs + 1 : 0), mN(n_jobs > 0 ? n_jobs : 0), index;
    for (int32_t &v : corr_start) in >> v;
    for (int32_t &v : mN) in >> v;
    for (int32_t v; in >> v;) index.push_back(v);
    if (cap < 0) cap = omv_ransac::words_cap(max_corr, max_jobs);
    std::vector<omv_ransac::JobLayout> lay;
    std::vector<int32_t> corr_job;
    int words = -1;
    const omv_status s = omv_ransac::plan_layout(
        n_jobs, (nulls & 1) ? nullptr : corr_start.data(), (nulls & 2) ? nullptr : mN.data(),
        (nulls & 4) ? nullptr : index.data(), !(nulls & 4), max_jobs, max_corr, cap, [&](int j) { return j != bad_job; },
        &lay, &corr_job, &words);
    std::printf("status %d", s);
    if (s == OMV_OK) {
        std::printf(" |");
        for (const auto &l : lay) std::printf(" %d", l.inl_start);
        std::printf(" |");
        for (const auto &l : lay) std::printf(" %d", l.word_start);
        std::printf(" | %d |", words);
        for (int v : corr_job) std::printf(" %d", v);
        bool same = true;   // the slices restate the input
        for (int j = 0; j < n_jobs; j++)
            same = same && lay[j].corr_start == corr_start[j] && lay[j].n == corr_start[j + 1] - corr_start[j] &&
                   lay[j].mn == mN[j];
        if (!same) std::printf(" | slices differ");
    }
    std::printf("\n");
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "its") {
            double prob;
            int mi, n, max_its;
            in >> prob >> mi >> n >> max_its;
            std::printf("its %d\n", n > 0 ? omv_ransac::ransac_its(prob, (float)mi / n, mi == n, max_its) : 1);
        } else if (what == "pnp") {
            double prob;
            int n, mi, max_its, min_set, its = 0, n_min = 0;
            float eps;
            in >> n >> prob >> mi >> max_its >> min_set >> eps;
            omv_ransac::mlpnp_parameters(n, prob, mi, max_its, min_set, eps, &its, &n_min);
            std::printf("pnp %d %d\n", its, n_min);
        } else if (what == "layout") {
            layout(in);
        } else {
            std::printf("unknown\n");
            return 1;
        }
    }
    return 0;
}
