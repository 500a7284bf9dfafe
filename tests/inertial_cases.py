"""The seeded job lists tests/test_inertial_gpu.py runs on the device.  tests/test_inertial_ref_cpu.py checks on the
reference alone that its dense and structured solves take the same decisions on every one of them (so the 1e-7 state
bar cannot hide a stop-decision flip of the reference itself) and that no keyframe's bias norm lies in the band round
0.01 where the Reintegrate() flag may go either way."""
from openmavis_amd import synth_inertial as si
from openmavis_amd.inertial_init import BIAS, FULL, GS

BAND = 2.0 ** -10        # relative band round 0.01 inside which the float flag is not compared
BAND_CAP = 0.01          # at most this share of a call's keyframes may lie inside it
P_INIT, P_SECOND, P_STRONG, P_NONE = (1e2, 1e5), (1.0, 1e5), (1e2, 1e10), (0.0, 0.0)

# (K, mode, mono, (priorG, priorA), breaks, isolated, shuffle): keyframe counts 1, 2, 3 (0, 1, 2 edges), 10 / 11
# (InitializeIMU's minimum), 64 / 65 / 66 (63 / 64 / 65 edges: the wavefront boundary), 129 / 130 and 300 (two and five
# passes of 64); every mode, mono on and off, the four prior pairs ((0, 0): the tau lambda init); broken chains, isolated
# keyframes, shuffled input order
MAIN = [
    (1, FULL, 0, P_INIT, (), (), False),
    (1, BIAS, 0, P_SECOND, (), (), False),
    (2, FULL, 1, P_INIT, (), (), False),
    (3, BIAS, 0, P_STRONG, (), (), False),
    (3, GS, 0, P_NONE, (), (), False),
    (10, FULL, 1, P_INIT, (), (), False),
    (10, FULL, 0, P_NONE, (), (), False),
    (11, GS, 0, P_NONE, (), (), False),
    (11, BIAS, 0, P_SECOND, (), (), True),
    (64, FULL, 1, P_SECOND, (20,), (), False),
    (65, FULL, 0, P_INIT, (), (30,), False),
    (65, BIAS, 0, P_INIT, (1, 40), (), True),
    (66, GS, 0, P_NONE, (), (10,), False),
    (66, FULL, 1, P_NONE, (), (), True),
    (129, FULL, 0, P_STRONG, (), (), False),
    (130, BIAS, 0, P_SECOND, (), (), False),
    (130, FULL, 1, P_INIT, (64,), (100,), False),
    (300, FULL, 0, P_INIT, (), (), False),
    (300, GS, 0, P_NONE, (), (), False),
    (64, GS, 0, P_NONE, (33,), (), True),
    (2, GS, 0, P_NONE, (), (), False),
    (129, BIAS, 0, P_NONE, (), (), False),
    (1, GS, 0, P_NONE, (), (), False),
]
SEED = 100


def make(cases=MAIN, seed=SEED):
    return [si.make_job(K, seed + 7 * i, mode, mono, pg, pa, breaks=br, isolated=iso, shuffle=sh)
            for i, (K, mode, mono, (pg, pa), br, iso, sh) in enumerate(cases)]


def chain_jobs(n=20, seed=500):
    """The jobs of the chain test: FULL, stereo, the records integrated from zero bias."""
    Ks = [10, 11, 12, 20, 33, 64, 65, 66, 17, 24] * 2
    other = {9: 1527}   # a seed whose last Levenberg decision the reference itself takes both ways is replaced
    return [si.make_job(Ks[i % len(Ks)], other.get(i, seed + 3 * i), FULL, 0, *P_INIT) for i in range(n)]
