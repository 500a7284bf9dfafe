"""What tests/optsim3_ref.py, tests/inertial_ref.py and tests/vba_ref.py share: the step control of g2o's
OptimizationAlgorithmLevenberg (optimization_algorithm_levenberg.cpp:61-185), line by line, as openmavis_amd/csrc/omv_lm.h
states it for the device.  The loops, the build / solve / oplus / chi2 / computeScale and the logs stay with the callers."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
TRIAL, ITERATION, STOP = "trial", "iteration", "stop"   # what follows a trial


class LmState:
    """_currentLambda, _ni, _nBad (kept between solve() calls) and currentChi, iniChi, qmax = _levenbergIterations."""
    def __init__(self):
        self.lam, self.ni, self.current_chi, self.ini_chi, self.qmax, self.n_bad = 0.0, 2.0, 0.0, 0.0, 0, 0


def lambda_init(user_lambda, max_diagonal):
    """computeLambdaInit (:171-185): a positive _userLambdaInit wins, otherwise _tau times the maximum of |H(j,j)|."""
    return float(user_lambda) if user_lambda > 0 else 1e-5 * float(max_diagonal)


def begin_iteration(s, iteration, chi, lam_init):
    """The start of solve(iteration) (:82-101); lam_init is read on iteration 0 only."""
    s.current_chi = s.ini_chi = float(chi)
    if iteration == 0:
        s.lam, s.ni, s.n_bad = float(lam_init), 2.0, 0
    s.qmax = 0


def good_step_factor(rho):
    """max(_goodStepLowerScale, min(1 - (2 rho - 1)^3, _goodStepUpperScale)) (:135-138).  The cube is the product, as in
    omv_lm.h, not pow(): the same bits everywhere, and the factor within 2^-51 relative of the one pow() gives (3.4e-16 at
    most over 5 million rho with the unclamped band 0.84 .. 0.95 sampled densely; test_lm_header_cpu.py has the bound)."""
    a = 2 * rho - 1
    return max(1. / 3., min(1. - a * a * a, 2. / 3.))


def trial(s, chi, solved, scale):
    """One pass of the do-while body after the trial's errors (:124-148): (rho, accepted).  A failed solve makes tempChi
    DBL_MAX, which is finite."""
    temp_chi = float(chi) if solved else DBL_MAX
    with np.errstate(all="ignore"):
        rho = float((np.float64(s.current_chi) - np.float64(temp_chi)) / (np.float64(scale) + np.float64(1e-3)))
    accepted = bool(rho > 0 and np.isfinite(temp_chi))
    if accepted:
        s.lam, s.ni, s.current_chi = s.lam * good_step_factor(rho), 2.0, temp_chi
    else:
        s.lam *= s.ni
        s.ni *= 2
    s.qmax += 1
    return rho, accepted


def gain_sides(s):
    """Both sides of Raul's stop test (:158): ((iniChi - currentChi) * 1e3, iniChi)."""
    return (s.ini_chi - s.current_chi) * 1e3, s.ini_chi


def next_step(s, rho, max_trials):
    """What follows a trial (:149-168): TRIAL (a NaN rho ends the trials without stopping), or, the iteration over, STOP
    (Terminate: the trials used up or rho == 0; the third iteration in a row that gained less than 0.1 %) or ITERATION."""
    if rho < 0 and s.qmax < max_trials:
        return TRIAL
    if s.qmax == max_trials or rho == 0:
        return STOP
    gain, ini = gain_sides(s)
    s.n_bad = s.n_bad + 1 if gain < ini else 0
    return STOP if s.n_bad >= 3 else ITERATION
