"""The float layer under every bit-exact kernel, as device code: omv_selftest_math runs openmavis_amd/csrc/omv_math.h
(and rcp_nr, the plain float `/`, the a * b + c contraction probes) as hipcc builds it for the kernels, with the
product's flags; oracle.math_map is the same text built by the host compiler.  The two must agree bit for bit on the
input sets of tests/math_inputs.py.  No libm is called for the float functions here, so this machine's C library does
not matter; tests/test_math_header_cpu.py ties the host build to glibc.

What a failure means: -ffp-contract=off not in force (MULADD_*), a `/` or sqrt that is not correctly rounded, flushed
denormals, a float -> int conversion or a folded constant that differs from the host's, or an edit that only one of
the two builds hides."""
import numpy as np
import pytest

import math_inputs as mi
from openmavis_amd import _lib, selftest as st

pytestmark = pytest.mark.gpu

IEEE_ONLY = [st.SINCOSF, st.ATANF, st.ATAN2F, st.TANF, st.SQRTF, st.FAST_ATAN2_DEG, st.ROUND_EVEN, st.DIVF,
             st.KB8_UNPROJECT, st.PINHOLE_PROJECT, st.PINHOLE_UNPROJECT, st.ROT_BIN, st.THREE_MAXIMA, st.GRID_CELL_OF,
             st.GRID_WINDOW, st.KP_IN_WINDOW]
CAMERA = [st.KB8_PROJECT, st.KB8_UNPROJECT, st.PINHOLE_PROJECT, st.PINHOLE_UNPROJECT]


def _calls(fn):
    return mi.camera_sets(fn) if fn in CAMERA else mi.SETS[fn]()


def _describe(fn, name, a, b, got, want, bad):
    rows = []
    for i in bad[:5]:
        args = a[i] if b is None or len(b) != len(a) else (a[i], b[i])
        rows.append(f"{args!r}: device {got[i]!r} != host {want[i]!r}")
    return f"{st.MATH_NAMES[fn]} [{name}]: {len(bad)} of {len(got)} differ, e.g. " + "; ".join(rows)


@pytest.mark.parametrize("fn", IEEE_ONLY, ids=lambda f: st.MATH_NAMES[f])
def test_device_equals_host_build(torch_cuda, oracle, fn):
    """selftest.math == oracle.math_map, bit for bit (NaN == NaN), on the whole input set of each function whose body
    uses IEEE operations only.  sincosf / tanf: |y| < 120, the restatement's domain (no large-argument reduction;
    orb_extract.hip's angles are in [0, 2 pi), imu.hip's arguments dt * theta, tri.hip's go through cosf_glibc).
    DIVF, SQRTF and ROUND_EVEN are also held to numpy's IEEE float32 divide, sqrt and rint.  ROT_BIN and THREE_MAXIMA
    are the matchers' rotation check (omv::rot_bin on all pairs of ~750 angles, omv::three_maxima on ~2,000
    histograms); GRID_CELL_OF, GRID_WINDOW and KP_IN_WINDOW are the keypoint grid and GetFeaturesInArea's window on
    the suite's two frame geometries (a few thousand elements); tests/test_math_header_cpu.py holds their host build
    to the reference's lines."""
    total = 0
    for name, a, b, c in _calls(fn):
        got, want = st.math(fn, a, b, c), oracle.math_map(fn, a, b, c)
        bad = mi.mismatches(got, want)
        assert len(bad) == 0, _describe(fn, name, a, b, got, want, bad)
        with np.errstate(all="ignore"):
            ref = {st.DIVF: lambda: a / b, st.SQRTF: lambda: np.sqrt(a),
                   st.ROUND_EVEN: lambda: np.rint(a).astype(np.int32)}.get(fn)
            if ref is not None:
                bad = mi.mismatches(got, ref())
                assert len(bad) == 0, "numpy: " + _describe(fn, name, a, b, got, ref(), bad)
        total += len(got)
    print(f"{st.MATH_NAMES[fn]}: {total} inputs, device == host")


@pytest.mark.parametrize("fn", [st.MULADD_F32, st.MULADD_F64], ids=lambda f: st.MATH_NAMES[f])
def test_device_does_not_contract(torch_cuda, oracle, fn):
    """a * b + c written with plain operators, on >= 10^5 triples whose fused and unfused values differ (selected with
    exact arithmetic on the host): the device returns the unfused value on every one, as the host build does."""
    a, b, c, unfused, fused = mi.muladd_f32() if fn == st.MULADD_F32 else mi.muladd_f64()
    assert len(a) >= 100000
    got = st.math(fn, a, b, c)
    n_fused = int(mi.same_bits(got, fused).sum())
    assert mi.same_bits(got, unfused).all(), f"{n_fused} of {len(a)} results are the fused value"
    assert mi.same_bits(got, oracle.math_map(fn, a, b, c)).all()


def test_rcp_nr_within_one_ulp(torch_cuda):
    """rcp_nr's own claim: within an ulp of the IEEE quotient 1 / x on normal numbers (2^22 doubles, reciprocal normal).
    Measured on gfx950: 100 % of the 4,194,304 results equal the quotient exactly (the share is printed)."""
    (_, x, _, _), = mi.rcp_nr()
    got = st.math(st.RCP_NR, x)
    q = 1.0 / x
    assert np.all(np.isfinite(q)) and np.all(np.abs(q) >= np.finfo(np.float64).tiny)
    err = np.abs(got - q) / np.spacing(np.abs(q))
    exact = float((got == q).mean())
    print(f"rcp_nr: {exact:.6%} of {len(x)} equal the IEEE quotient, max {err.max()} ulp")
    worst = np.argmax(err)
    assert err.max() <= 1.0, (x[worst], got[worst], q[worst])


def test_kb8_project(torch_cuda, oracle):
    """kb8_project_f calls the device library's double cos / sin where the host calls glibc's; the expectation is
    still equal bits.  Only a sample that differs is evaluated at 50 digits from its exact double operands, and
    accepted only if that value lies within 4 double ulps of a float rounding boundary and the device result is one of
    the two floats around it; such samples are printed, and at most 2 are allowed over the five calibrations.
    Measured on gfx950: 0 of 657,920 points differ (the host reference itself uses up 0, test_math_header_cpu)."""
    ties = 0
    for name, X, k, _ in mi.camera_sets(st.KB8_PROJECT):
        got, want = st.math(st.KB8_PROJECT, X, k), oracle.math_map(st.KB8_PROJECT, X, k)
        idx = mi.mismatches(got, want)
        print(f"kb8_project_f [{name}]: {len(idx)} of {len(X)} points differ from the host build")
        t, bad = mi.judge_kb8_project(k, X, got, idx[:50])
        assert not bad and len(idx) <= 2, (name, len(idx), bad[:5])
        ties += t
    assert ties <= 2


def test_predict_scale(torch_cuda, oracle):
    """(int)ceil(log((double)ratio) / (double)lsf) with the device library's double log, by the same rule: a differing
    sample must have its 50-digit quotient within 4 double ulps of an integer n and the device result n or n + 1; at
    most 2.  Measured on gfx950: 0 of 1,179,664 ratios differ (the host reference uses up 0)."""
    (_, ratio, lsf, _), = mi.predict_scale()
    got, want = st.math(st.PREDICT_SCALE, ratio, lsf), oracle.math_map(st.PREDICT_SCALE, ratio, lsf)
    idx = mi.mismatches(got, want)
    print(f"PredictScale: {len(idx)} of {len(ratio)} ratios differ from the host build")
    ties, bad = mi.judge_predict_scale(ratio, lsf[0], got, idx[:50])
    assert not bad and len(idx) <= 2, (len(idx), bad[:5])


def test_predict_scale_clamp(torch_cuda, oracle):
    """omv::predict_scale, the function the kernels call, is the clamp to [0, n_levels - 1] of the device's own
    unclamped level, on the PredictScale set and around both ends of the clamp (raw levels below 0 and at or above
    n_levels; the CPU test asserts the set holds them); the unclamped level of the added ratios is held to the host
    build by test_predict_scale's rule."""
    (_, ratio, lsf, _), = mi.predict_scale()
    ratio = np.concatenate([mi.predict_scale_clamp_ends(), ratio])
    raw = st.math(st.PREDICT_SCALE, ratio, lsf)
    got = st.math(st.PREDICT_SCALE_CLAMPED, ratio, np.array([lsf[0], mi.N_LEVELS], np.float32))
    assert np.array_equal(got, np.clip(raw, 0, mi.N_LEVELS - 1))
    assert raw.min() < 0 and raw.max() >= mi.N_LEVELS
    idx = mi.mismatches(raw, oracle.math_map(st.PREDICT_SCALE, ratio, lsf))
    ties, bad = mi.judge_predict_scale(ratio, lsf[0], raw, idx[:50])
    assert not bad and len(idx) <= 2, (len(idx), bad[:5])


def test_hook_argument_checks(torch_cuda):
    """An unknown fn or a null pointer with n > 0: OMV_ERR_ARG before any launch; n == 0: OMV_OK."""
    torch = torch_cuda
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = _lib.ptr(buf)
    for fn in (-1, len(st.MATH_NAMES), 1000):
        assert lib.omv_selftest_math(fn, 4, p, p, p, p, None) == _lib.OMV_ERR_ARG
        assert lib.omv_selftest_math(fn, 0, p, p, p, p, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.ATANF, -1, p, None, None, p, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.ATANF, 4, None, None, None, p, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.ATANF, 4, p, None, None, None, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.ATAN2F, 4, p, None, None, p, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.MULADD_F32, 4, p, p, None, p, None) == _lib.OMV_ERR_ARG
    assert lib.omv_selftest_math(st.KB8_PROJECT, 4, p, None, None, p, None) == _lib.OMV_ERR_ARG
    for fn in range(len(st.MATH_NAMES)):
        assert lib.omv_selftest_math(fn, 0, None, None, None, None, None) == _lib.OMV_OK
    assert lib.omv_selftest_math(st.ATANF, 4, p, None, None, p, None) == _lib.OMV_OK   # b, c unused: may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[:8], np.zeros(8, np.float32))               # atanf(0) = 0 in place
    assert st.math(st.SQRTF, np.zeros(0, np.float32)).shape == (0,)
