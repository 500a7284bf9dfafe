// g2o's Levenberg-Marquardt step control (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-185), stated
// once for the solvers that run it: optimize_sim3_kernel (optsim3.hip), both Local BA drivers (lba.hip) and the pose
// graphs' device control (essgraph.hip);
// pose_only_kernel (pose.hip) and inertial_opt_kernel (inertial.hip) follow it written out.  Only the arithmetic and
// the decisions are here; a site keeps its loops, its build / solve / oplus / chi2 / computeScale reductions and where
// the state lives.  One text for hipcc (both sides) and a plain C++ compiler (tests/cpp/lm_host.cpp); tests/lm_ref.py
// is the same rules in Python.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define OMV_LM_FN __host__ __device__ inline
#else
#define OMV_LM_FN inline
#endif

namespace omv_lm {

// _currentLambda, _ni, _nBad (kept between solve() calls) and currentChi, iniChi, qmax = _levenbergIterations.
struct LmState {
    double lambda, ni, currentChi, iniChi;
    int qmax, nBad;
};

// computeLambdaInit (:171-185): a positive _userLambdaInit, otherwise _tau times the site's maximum of |H(j,j)|.
OMV_LM_FN double lm_lambda_init(double user_lambda, double max_diagonal) {
    return user_lambda > 0 ? user_lambda : 1e-5 * max_diagonal;
}

// The start of solve(iteration) (:82-101), after computeActiveErrors: chi = activeRobustChi2 of the current estimate.
// lambda_init is read on iteration 0 only.
OMV_LM_FN void lm_begin_iteration(LmState &s, int iteration, double chi, double lambda_init) {
    s.currentChi = s.iniChi = chi;
    if (iteration == 0) s.lambda = lambda_init, s.ni = 2, s.nBad = 0;
    s.qmax = 0;
}

struct LmTrial {
    double rho;
    bool accepted;   // discardTop(): the trial becomes the estimate; otherwise pop()
};

// One pass of the do-while body after the trial's errors (:124-148).  chi = activeRobustChi2 of the trial estimate,
// solved = _solver->solve() succeeded, scale = computeScale() = sum x_j (lambda x_j + b_j) at the lambda of this trial.
// A failed solve makes tempChi DBL_MAX, which is finite: with a scale below -1e-3 the reference accepts it.  The cube
// is the product, not pow(): under -ffp-contract=off the same bits on host and device without a math library, and
// the clamped factor within 2^-51 relative of the one pow() gives.
OMV_LM_FN LmTrial lm_trial(LmState &s, double chi, bool solved, double scale) {
    const double tempChi = solved ? chi : DBL_MAX;
    const double rho = (s.currentChi - tempChi) / (scale + 1e-3);
    const bool accepted = rho > 0 && std::isfinite(tempChi);
    if (accepted) {
        const double a = 2 * rho - 1;
        double alpha = 1. - a * a * a;
        alpha = fmin(alpha, 2. / 3.);   // _goodStepUpperScale
        s.lambda *= fmax(1. / 3., alpha);   // _goodStepLowerScale
        s.ni = 2;
        s.currentChi = tempChi;
    } else {
        s.lambda *= s.ni;
        s.ni *= 2;
    }
    s.qmax++;
    return LmTrial{rho, accepted};
}

enum LmNext { kLmTrial, kLmIteration, kLmStop };

// What follows a trial (:149-168): another trial of this iteration (a NaN rho ends the trials without stopping), or,
// the iteration over, Terminate (the trials used up or rho == 0, also after an accepted trial with max_trials == 1;
// the third iteration in a row that gained less than 0.1 %) or OK.
OMV_LM_FN LmNext lm_next(LmState &s, double rho, int max_trials) {
    if (rho < 0 && s.qmax < max_trials) return kLmTrial;
    if (s.qmax == max_trials || rho == 0) return kLmStop;
    s.nBad = (s.iniChi - s.currentChi) * 1e3 < s.iniChi ? s.nBad + 1 : 0;
    return s.nBad >= 3 ? kLmStop : kLmIteration;
}

}  // namespace omv_lm
