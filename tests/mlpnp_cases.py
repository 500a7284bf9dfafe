"""The seeded case lists tests/test_mlpnp_gpu.py runs on the device; tests/test_mlpnp_ref_cpu.py checks on the
reference alone that the share of hypotheses each case would leave out of a comparison stays under its cap."""
import numpy as np

from openmavis_amd import synth_pnp
from openmavis_amd.sim3solver import draw

KB8, PIN = 0, 1
LEFT_OUT_CAP = 0.05     # computePose: hypotheses with a decision within 2^-20 of its threshold, or kappa > 1e8
BAND_CAP = 1e-3         # CheckInliers: entries within 2^-10 of the threshold
DELTA = 2.0 ** -10

# (ns, H, models, scenes, noise_px, outlier_share, seed): one handle of len(ns) jobs, H hypotheses each.  The computePose
# cases put the world origin at the centre of the point cloud ("centred", depth 2-6 m): with the origin at the camera
# and depths to 15 m the conditioning kappa of six-point samples passes 1e8 for a third of them, and the comparison
# would leave those out.
B_CASES = [
    ((6,), 16, PIN, "centred", 0.5, 0.0, 11),
    ((7,), 64, KB8, "centred", 0.5, 0.0, 12),
    ((63, 64, 65), 32, (KB8, PIN, KB8), "centred", 0.5, 0.0, 13),
    ((130,), 64, PIN, "centred", 0.5, 0.3, 14),
    ((64,), 32, PIN, "planar", 0.2, 0.0, 15),
    ((65, 7), 32, KB8, "planar", 0.2, 0.0, 16),
]
C_CASES = [
    ((63, 64, 65), 64, (KB8, PIN, KB8), "general", 0.5, 0.2, 21),
    ((130, 6, 7), 64, (PIN, KB8, PIN), ("general", "general", "planar"), 0.5, 0.2, 22),
]


def make(case):
    """(jobs, draws [J][H][6]) of a case."""
    ns, H, models, scenes, noise, outl, seed = case
    jobs = synth_pnp.make_jobs(list(ns), seed=seed, models=models, scenes=scenes, noise_px=noise, outlier_share=outl,
                                depth=(2.0, 6.0))
    rng = np.random.default_rng(seed + 100)
    draws = np.stack([draw(rng, H, n, 6) for n in ns])
    return jobs, draws
