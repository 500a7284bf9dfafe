"""The visual bundle adjustment's test windows (openmavis_amd.synth_vba) and their reference runs (vba_ref), shared by
the CPU and GPU tests.  The shapes are the smallest that cross the solver's structure limits:

  small  4 KannalaBrandt8 cameras, 12 keyframes (7 optimisable), 300 points: more than one landmark group (128)
  pin    the same with Pinhole cameras and 40 % stereo edges on camera 0
  mixed  both camera models, stereo, 5 % gross outliers and a few KannalaBrandt8 edges planted behind their camera
  wide   40 optimisable + 8 fixed keyframes, 600 points, each seen from >= 34 optimisable keyframes: more keyframes
         than a landmark group holds (32)

Every window also has points seen from fixed keyframes only and points without edges.  The seeds are chosen so that the
reference alone meets the conditions test_vba_ref_cpu.py asserts: no marginal LM decision, few edges near an outlier
threshold.
"""
import functools

import numpy as np

import vba_ref
from openmavis_amd import synth_vba

CASES = {
    "small": dict(n_kf=12, n_opt=7, n_pts=300, seed=1, cams="kb8"),
    "pin": dict(n_kf=12, n_opt=7, n_pts=300, seed=2, cams="pinhole", stereo_frac=0.4),
    "mixed": dict(n_kf=12, n_opt=7, n_pts=300, seed=3, cams="mixed", stereo_frac=0.3, outlier_frac=0.05,
                  behind_frac=0.02),
    "wide": dict(n_kf=48, n_opt=40, n_pts=600, seed=4, cams="kb8", views=44, min_opt_views=34, speed=0.3,
                 yaw_rate=0.05),
}
LAMBDAS = (100.0, 0.0)   # an inertial map's user lambda; computeLambdaInit


@functools.lru_cache(maxsize=None)
def problem(name):
    return synth_vba.make_vba_problem(**CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, lambda_init, iterations=10):
    """vba_ref.optimize of the case from its initial state: (result, final state)."""
    prob = problem(name)
    G = vba_ref.Graph(prob)
    return vba_ref.optimize(G, vba_ref.start_of(prob), iterations, lambda_init)


@functools.lru_cache(maxsize=None)
def reference_two_rounds(name, lambda_init=0.0):
    """The merge overload's schedule: optimize(5), exclude the flagged edges and drop the robust kernels, optimize(10).
    Returns (first result, second result, final state)."""
    prob = problem(name)
    G = vba_ref.Graph(prob)
    r1, st = vba_ref.optimize(G, vba_ref.start_of(prob), 5, lambda_init)
    G.set_levels(r1["outlier"][:G.EM], r1["outlier"][G.EM:])
    r2, st = vba_ref.optimize(G, st, 10, lambda_init, hub=(0.0, 0.0))
    return r1, r2, st


def chi2_tol(chi2):
    """Per-edge chi2 tolerance (tests/test_lba_gpu.py's): the whitened residual may differ by 1e-3."""
    return 1e-6 * chi2 + 2e-3 * np.sqrt(chi2) + 1e-6


def band(G, chi2):
    """Edges whose chi2 lies within the tolerance of their outlier threshold."""
    thr = np.where(G.stereo, vba_ref.CHI2_STEREO, vba_ref.CHI2_MONO)
    return np.abs(chi2 - thr) <= chi2_tol(chi2)
