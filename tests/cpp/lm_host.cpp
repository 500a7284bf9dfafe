// openmavis_amd/csrc/omv_lm.h on the host, driven by scripted traces (tests/test_lm_header_cpu.py).  One command per
// input line, one output line per `it` and `tr`; doubles are read with strtod (hex floats, inf, nan) and printed as
// their 64 bits.
//   new                                   a fresh state (a new optimizer)
//   opt <max_trials> <user_lambda> <max_diagonal>    an optimize() on the current state: the next `it` is iteration 0
//   it <chi2>                             the start of an iteration     -> it <lambda> <ni> <currentChi> <iniChi> <qmax> <nBad>
//   tr <chi2> <solved> <scale>            one trial and what follows it -> tr <lambda> <ni> <currentChi> <rho> <accepted> <next> <qmax> <nBad>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../openmavis_amd/csrc/omv_lm.h"

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main() {
    omv_lm::LmState s{};
    int max_trials = 0, iteration = 0;
    double user = 0, max_diagonal = 0;
    char line[512], a[3][128];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "new", 3)) {
            s = omv_lm::LmState{};
        } else if (sscanf(line, "opt %d %127s %127s", &max_trials, a[0], a[1]) == 3) {
            user = strtod(a[0], nullptr), max_diagonal = strtod(a[1], nullptr);
            iteration = 0;
        } else if (sscanf(line, "it %127s", a[0]) == 1) {
            omv_lm::lm_begin_iteration(s, iteration++, strtod(a[0], nullptr), omv_lm::lm_lambda_init(user, max_diagonal));
            printf("it %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d\n", bits(s.lambda), bits(s.ni),
                   bits(s.currentChi), bits(s.iniChi), s.qmax, s.nBad);
        } else if (sscanf(line, "tr %127s %127s %127s", a[0], a[1], a[2]) == 3) {
            const omv_lm::LmTrial t = omv_lm::lm_trial(s, strtod(a[0], nullptr), atoi(a[1]) != 0, strtod(a[2], nullptr));
            const omv_lm::LmNext next = omv_lm::lm_next(s, t.rho, max_trials);
            printf("tr %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %s %d %d\n", bits(s.lambda), bits(s.ni),
                   bits(s.currentChi), bits(t.rho), t.accepted ? 1 : 0,
                   next == omv_lm::kLmTrial ? "trial" : next == omv_lm::kLmIteration ? "iteration" : "stop", s.qmax, s.nBad);
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
