"""The product's float layer (openmavis_amd/csrc/omv_math.h) compiled for the host, against the C library itself.

Three links carry every "bit-exact" claim of the kernels, each a bit comparison of different things:
  1. device build of the header == host build of the header       tests/test_math_device_gpu.py (needs no libm)
  2. host build of the header == this machine's glibc              here: oracle.math_map == oracle.libm_map
  3. this glibc == the recorded answers of glibc 2.35              here: tests/golden/libm_kat.npz
The input sets are tests/math_inputs.py, shared with the GPU side."""
import numpy as np
import pytest

import math_inputs as mi
from openmavis_amd import selftest as st

LIBM_BACKED = [st.SINCOSF, st.ATANF, st.ATAN2F, st.TANF, st.SQRTF, st.FAST_ATAN2_DEG, st.ROUND_EVEN, st.PREDICT_SCALE]
CAMERA = [st.KB8_PROJECT, st.KB8_UNPROJECT, st.PINHOLE_PROJECT, st.PINHOLE_UNPROJECT]


def _calls(fn):
    return mi.camera_sets(fn) if fn in CAMERA else mi.SETS[fn]()


def _describe(fn, name, a, b, got, want, bad):
    rows = []
    for i in bad[:5]:
        args = a[i] if b is None or len(b) != len(a) else (a[i], b[i])
        rows.append(f"{args!r}: {got[i]!r} != {want[i]!r}")
    return f"{st.MATH_NAMES[fn]} [{name}]: {len(bad)} of {len(got)} differ, e.g. " + "; ".join(rows)


@pytest.mark.parametrize("fn", LIBM_BACKED + CAMERA, ids=lambda f: st.MATH_NAMES[f])
def test_host_header_equals_libm(oracle, fn):
    """oracle_math_map (the header) == oracle_libm_map (sinf / cosf / atanf / atan2f / tanf / sqrtf / nearbyintf, the
    oracle's kb8_project_f / kb8_unproject_f / Pinhole pair with glibc's double cos / sin / tan, oracle_fast_atan2, and
    ceil(log()) for PredictScale), bit for bit, NaN == NaN, on every input set.

    Asserted domain of sincosf / tanf: |y| < 120.  The restatement has glibc's reduce_fast only, no large-argument
    reduction, and first departs from libm near 200; nothing is asserted beyond 120.  The callers stay far inside:
    orb_extract.hip's angles are in [0, 2 pi), imu.hip's arguments are dt * theta (~1e-3), tri.hip takes cosines of
    parallax angles through cosf_glibc, and kb8_unproject_f's tanf argument is clamped to pi / 2.  atanf / atan2f are
    asserted over the whole float range, infinities and NaNs included."""
    total = 0
    for name, a, b, c in _calls(fn):
        got, want = oracle.math_map(fn, a, b, c), oracle.libm_map(fn, a, b, c)
        bad = mi.mismatches(got, want)
        assert len(bad) == 0, _describe(fn, name, a, b, got, want, bad)
        total += len(got)
    print(f"{st.MATH_NAMES[fn]}: {total} inputs, header == libm")


def test_input_sets_cover_the_unproject_branches():
    """The pixel sets reach the scale = 1 branch (the principal point), the pi / 2 clamp, and rigs that need all ten
    Newton steps (Hilti cameras 3 and 4 beyond the image; cameras 1 and 2 converge within four everywhere)."""
    ten = 0
    for ci, (_, k) in enumerate(mi.CALIBS):
        steps, clamped = mi.newton_steps(k, mi.unproject_pixels(ci))
        assert (steps == 0).sum() >= 1 and clamped.sum() >= 1000
        ten += int((steps == 10).sum())
    assert ten >= 1000
    for name, a, *_ in mi.trig():
        assert len(a) <= 1 << 24 and np.all(np.abs(a) < 120), name


def test_running_libm_reproduces_the_recorded_answers():
    """tests/golden/libm_kat.npz holds glibc 2.35's answers (tools/make_golden.py libm_kat) on 2,000 inputs per float
    function and 900 per double function.  A C library that rounds one of them differently fails here, as a libm
    difference, and not in the header comparison above as a header bug."""
    import os
    kat = np.load(os.path.join(os.path.dirname(__file__), "golden", "libm_kat.npz"))
    got = mi.kat_eval()
    assert sorted(got) == sorted(k for k in kat.files if k != "libc")
    for name, v in got.items():
        bad = mi.mismatches(v, kat[name])
        assert len(bad) == 0, (f"this C library's {name} differs from the recorded {kat['libc']} on {len(bad)} of {len(v)} "
                               f"inputs, e.g. {[a[bad[0]] for a in mi.kat_inputs()[name]]!r}: {v[bad[0]]!r} != "
                               f"{kat[name][bad[0]]!r}")


def _ulp32(v):
    import mpmath
    if v == 0:
        return mpmath.mpf(2) ** -149
    return mpmath.ldexp(1, max(int(mpmath.floor(mpmath.log(abs(v), 2))), -126) - 23)


def test_accuracy_against_mpmath(oracle):
    """A sanity check that the recorded libm is a sane one: the error of the host header and of libm against mpmath at
    50 digits, in ulps of float, on 4,096 samples per transcendental function drawn from the input sets.  The bar for
    the header is libm's own figure of the same run, with no margin (the two are bit-identical).

    Measured (glibc 2.35): sinf 0.5372, cosf 0.5291, tanf 0.6540, atanf 0.5871, atan2f 0.8618 ulp at most, header and
    libm alike."""
    import mpmath
    rng = np.random.default_rng(20240212)

    def pick(arrs, cond):
        ok = np.flatnonzero(cond(*arrs))
        idx = rng.choice(ok, 4096, replace=False)
        return [np.ascontiguousarray(a[idx]) for a in arrs]
    trig_in = np.concatenate([a for _, a, *_ in mi.trig()])
    (x,) = pick([trig_in], np.isfinite)
    (xa,) = pick([np.concatenate([a for _, a, *_ in mi.atanf()])], np.isfinite)
    sets = mi.atan2()
    y2, x2 = pick([np.concatenate([s[1] for s in sets]), np.concatenate([s[2] for s in sets])],
                  lambda y, x: np.isfinite(y) & np.isfinite(x) & ((y != 0) | (x != 0)))
    cases = [("sinf", st.SINCOSF, 0, (x,), mpmath.sin), ("cosf", st.SINCOSF, 1, (x,), mpmath.cos),
             ("tanf", st.TANF, None, (x,), mpmath.tan), ("atanf", st.ATANF, None, (xa,), mpmath.atan),
             ("atan2f", st.ATAN2F, None, (y2, x2), mpmath.atan2)]
    with mpmath.workdps(50):
        for name, fn, col, args, ref in cases:
            hdr, libm = oracle.math_map(fn, *args), oracle.libm_map(fn, *args)
            if col is not None:
                hdr, libm = hdr[:, col], libm[:, col]
            err = [mpmath.mpf(0), mpmath.mpf(0)]
            for i in range(4096):
                want = ref(*[mpmath.mpf(float(a[i])) for a in args])
                u = _ulp32(want)
                for j, got in enumerate((hdr[i], libm[i])):
                    err[j] = max(err[j], abs(mpmath.mpf(float(got)) - want) / u)
            print(f"{name}: header {float(err[0]):.4f} ulp, libm {float(err[1]):.4f} ulp")
            assert err[1] < 1.0, f"{name}: this libm is off by {float(err[1])} ulp"
            assert err[0] <= err[1], f"{name}: header {float(err[0])} ulp > libm {float(err[1])} ulp"


def _fast_atan2_numpy(y, x):
    """cv::fastAtan2 from OpenCV's published atan_f32 (modules/core/src/mathfuncs_core.simd.hpp), in numpy float32:
    every operation one IEEE float operation, the coefficients the float products p_k * (float)(180 / pi)."""
    f = np.float32
    r2d = f(180.0 / np.pi)
    p1, p3, p5, p7 = (f(v) * r2d for v in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
                                            -0.04432655554792128))
    eps = f(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        big = ax >= ay
        c = np.where(big, ay / (ax + eps), ax / (ay + eps))
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
        a = np.where(big, a, f(90.0) - a)
        a = np.where(x < 0, f(180.0) - a, a)
        a = np.where(y < 0, f(360.0) - a, a)
    assert a.dtype == np.float32
    return a


def test_numpy_restatements_agree_with_the_host_header(oracle):
    """fast_atan2_deg against OpenCV's formula in numpy float32; sqrtf_cr, `/` and round_even against numpy's IEEE
    float32 sqrt, divide and rint."""
    for name, y, x, _ in mi.fast_atan2():
        bad = mi.mismatches(oracle.math_map(st.FAST_ATAN2_DEG, y, x), _fast_atan2_numpy(y, x))
        assert len(bad) == 0, (name, len(bad), y[bad[:3]], x[bad[:3]])
    with np.errstate(all="ignore"):
        for name, a, *_ in mi.sqrtf():
            bad = mi.mismatches(oracle.math_map(st.SQRTF, a), np.sqrt(a))
            assert len(bad) == 0, (name, len(bad), a[bad[:3]])
        for name, a, b, _ in mi.divf():
            bad = mi.mismatches(oracle.math_map(st.DIVF, a, b), a / b)
            assert len(bad) == 0, (name, len(bad), a[bad[:3]], b[bad[:3]])
    for name, a, *_ in mi.round_even():
        assert np.array_equal(oracle.math_map(st.ROUND_EVEN, a), np.rint(a).astype(np.int32)), name


def test_rot_bin_against_the_reference_lines(oracle):
    """omv::rot_bin (host build) against ORBmatcher.cc:475-481 restated in numpy float32 with round half away from
    zero, on every ordered pair of math_inputs.rot_angles().  The set reaches every bin the formula can give (0..12:
    rot <= 360 and the factor is 1 / 30), both sides of every half-integer of rot / 30, and rot == 360 exactly."""
    (name, a1, a2, _), = mi.rot_bin()
    got, want = oracle.math_map(st.ROT_BIN, a1, a2), mi.rot_bin_ref(a1, a2)
    bad = mi.mismatches(got, want)
    assert len(bad) == 0, _describe(st.ROT_BIN, name, a1, a2, got, want, bad)
    assert sorted(np.unique(got)) == list(range(13))
    tiny = (a1 == 0) & (a2 > 0) & (a2 < 1e-30)
    assert tiny.sum() == 2 and np.all(got[tiny] == 12)   # the smallest negative differences: rot == 360


def test_three_maxima_against_the_reference_loop(oracle):
    """omv::three_maxima (host build) against the literal loop of ORBmatcher::ComputeThreeMaxima in Python with the
    10 % products in float32: the empty histogram (-1, -1, -1), a single bin, ties between bins (the first wins), and
    the 10 % rule one count below, at and one above max1 / 10 for the second and the third bin."""
    (name, h, _, _), = mi.three_maxima()
    got, want = oracle.math_map(st.THREE_MAXIMA, h), mi.three_maxima_ref(h)
    bad = mi.mismatches(got, want)
    assert len(bad) == 0, (len(bad), h[bad[0]], got[bad[0]], want[bad[0]])
    assert np.array_equal(got[0], [-1, -1, -1]) and not h[0].any()
    assert np.array_equal(got[1:31], np.stack([np.arange(30), np.full(30, -1), np.full(30, -1)], 1))
    full = np.flatnonzero((h == 4).all(axis=1))
    assert len(full) == 1 and np.array_equal(got[full[0]], [0, 1, 2])
    # the boundary rows: the second / third index is dropped exactly when its count is below a tenth of the first
    dropped2, dropped3 = (got[:, 1] < 0) & (got[:, 0] >= 0), (got[:, 2] < 0) & (got[:, 1] >= 0)
    assert dropped2.sum() >= 30 and dropped3.sum() >= 30 and (got[:, 2] >= 0).sum() >= 30


def test_grid_input_sets_cover_the_window_branches():
    """The grid sets reach, on both frame geometries: each of GetFeaturesInArea's four early returns; each of the four
    clamps on a window that hits the grid; window edges exactly on a cell boundary (and both float neighbours, by
    construction); r = 0 and r larger than the image; keypoints on the image border, one ulp outside it, and outside
    the grid on each side; for the keypoint test bCheckLevels false and true, maxL -1, equal to and above the octave,
    and |kx - x| == r, |ky - y| == r exactly."""
    for (name, win, g, _), (_, kp, _, _), (_, e, _, _), (_, w, h) in zip(mi.grid_window(), mi.grid_cell_of(),
                                                                       mi.kp_in_window(), mi.GRID_FRAMES):
        assert 500 <= len(win) <= 3000 and 300 <= len(kp) <= 5000 and 400 <= len(e) <= 3000, name
        rng4, ret, clamped = mi.grid_window_ref(win, g)
        for k in (1, 2, 3, 4):
            assert (ret == k).sum() >= 3, (name, k)
        hit = ret == 0
        for k in range(4):
            assert (hit & clamped[:, k]).sum() >= 3, (name, k)
            assert (hit & ~clamped[:, k]).sum() >= 3, (name, k)
        x, y, r = win[:, 0], win[:, 1], win[:, 2]
        for v in ((x - r) * g[2], (x + r) * g[2], (y - r) * g[3], (y + r) * g[3]):
            assert (hit & (v == np.rint(v)) & (r > 0)).sum() >= 5, name   # an edge exactly on a cell boundary
        assert (r == 0).sum() >= 10 and (r > max(w, h)).sum() >= 4, name
        cell = mi.grid_cell_of_ref(kp, g)
        kx, ky = kp[:, 0], kp[:, 1]
        for on, v, lim in ((kx, kx, w), (ky, ky, h)):
            assert (v == 0).any() and (v == lim).any() and (v == np.nextafter(np.float32(0), np.float32(-1))).any()
            assert (v == np.nextafter(np.float32(lim), np.float32(np.inf))).any(), name
        assert ((cell < 0) & (kx < 0)).any() and ((cell < 0) & (kx > 0) & (ky > 0) & (ky < h)).any(), name
        assert ((cell < 0) & (ky < 0)).any() and ((cell < 0) & (ky > 0) & (kx > 0) & (kx < w)).any(), name
        assert set(np.unique(cell // mi.GRID_ROWS)) >= {-1, 0, 63} and set(np.unique(cell[cell >= 0] % mi.GRID_ROWS)) >= {0, 47}
        o, lo, hi = e[:, 2], e[:, 6], e[:, 7]
        check = (lo > 0) | (hi >= 0)
        assert (~check).sum() >= 40 and ((lo > 0) & (hi < 0)).sum() >= 40 and ((lo == 0) & (hi >= 0)).sum() >= 40, name
        assert (check & (hi == o)).sum() >= 40 and (check & (hi > o)).sum() >= 40 and (check & (hi >= 0) & (hi < o)).sum() >= 20
        assert (check & (o < lo)).sum() >= 40, name
        edge = e[:, 5] > 0
        assert (edge & (np.abs(e[:, 0] - e[:, 3]) == e[:, 5])).sum() >= 6, name
        assert (edge & (np.abs(e[:, 1] - e[:, 4]) == e[:, 5])).sum() >= 6, name
        want = mi.kp_in_window_ref(e)
        assert (want == 1).sum() >= 50 and (want == 0).sum() >= 50, name


def test_grid_functions_against_the_reference_lines(oracle):
    """omv::grid_cell_of, grid_window and kp_in_window (host build) against Frame.cc:969-978, :890-930 and :932-963
    restated in numpy float32, exactly (integers), on both frame geometries."""
    for name, kp, g, _ in mi.grid_cell_of():
        got, want = oracle.math_map(st.GRID_CELL_OF, kp, g), mi.grid_cell_of_ref(kp, g)
        bad = mi.mismatches(got, want)
        assert len(bad) == 0, (name, len(bad), kp[bad[:3]], got[bad[:3]], want[bad[:3]])
    for name, win, g, _ in mi.grid_window():
        got, want = oracle.math_map(st.GRID_WINDOW, win, g), mi.grid_window_ref(win, g)[0]
        bad = mi.mismatches(got, want)
        assert len(bad) == 0, (name, len(bad), win[bad[:3]], got[bad[:3]], want[bad[:3]])
    for name, e, _, _ in mi.kp_in_window():
        got, want = oracle.math_map(st.KP_IN_WINDOW, e), mi.kp_in_window_ref(e)
        bad = mi.mismatches(got, want)
        assert len(bad) == 0, (name, len(bad), e[bad[:3]], got[bad[:3]], want[bad[:3]])


def test_a_keypoint_in_the_box_lies_in_a_visited_cell(oracle):
    """The agreement between the grid build and the window walk: for every keypoint and every window of the sets
    (~3,100 x ~800 pairs per geometry), a keypoint that lies in the grid and passes the box test |kx - x| < r &&
    |ky - y| < r is binned (grid_cell_of) into a cell that the window (grid_window) visits.  Otherwise
    GetFeaturesInArea would never see a keypoint its own test admits.  Both functions are the host build.

    Measured: no pair of either geometry fails, so no input is recorded here as the reference's own miss."""
    for (name, win, g, _), (_, kp, _, _) in zip(mi.grid_window(), mi.grid_cell_of()):
        cell = oracle.math_map(st.GRID_CELL_OF, kp, g)
        rng4 = oracle.math_map(st.GRID_WINDOW, win, g)
        assert np.array_equal(cell, mi.grid_cell_of_ref(kp, g)) and np.array_equal(rng4, mi.grid_window_ref(win, g)[0])
        px, py = (cell // mi.GRID_ROWS)[:, None], (cell % mi.GRID_ROWS)[:, None]
        box = (np.abs(kp[:, 0][:, None] - win[:, 0][None]) < win[:, 2][None]) & \
              (np.abs(kp[:, 1][:, None] - win[:, 1][None]) < win[:, 2][None]) & (cell >= 0)[:, None]
        x0, x1, y0, y1 = (rng4[:, k][None] for k in range(4))
        visited = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (x0 >= 0)
        bad = np.argwhere(box & ~visited)
        print(f"{name}: {int(box.sum())} of {box.size} pairs in the box")
        assert box.sum() >= len(win), name   # every window with r > 0 admits the edge keypoints made for it
        assert len(bad) == 0, (name, len(bad), [(kp[i], win[j], cell[i], rng4[j]) for i, j in bad[:3]])


def test_predict_scale_clamp(oracle):
    """omv::predict_scale is predict_scale_raw (the PREDICT_SCALE code, held to libm and to 50 digits above) clamped to
    [0, n_levels - 1]: on the PredictScale set and on ratios around both ends of the clamp, raw levels below 0 and at
    or above n_levels included."""
    (_, ratio, lsf, _), = mi.predict_scale()
    ratio = np.concatenate([mi.predict_scale_clamp_ends(), ratio])
    raw = oracle.math_map(st.PREDICT_SCALE, ratio, lsf)
    got = oracle.math_map(st.PREDICT_SCALE_CLAMPED, ratio, np.array([lsf[0], mi.N_LEVELS], np.float32))
    assert np.array_equal(got, np.clip(raw, 0, mi.N_LEVELS - 1))
    for level in (-12, -2, -1, 0, 1, mi.N_LEVELS - 2, mi.N_LEVELS - 1, mi.N_LEVELS, mi.N_LEVELS + 1, 25):
        assert (raw == level).any(), level


def test_host_build_does_not_contract(oracle):
    """The host build of the probes returns the unfused a * b + c on >= 10^5 triples each whose fused value differs
    (-ffp-contract=off in oracle/Makefile)."""
    for fn, (a, b, c, unfused, fused) in ((st.MULADD_F32, mi.muladd_f32()), (st.MULADD_F64, mi.muladd_f64())):
        assert len(a) >= 100000 and not mi.same_bits(unfused, fused).any()
        got = oracle.math_map(fn, a, b, c)
        assert mi.same_bits(got, unfused).all(), (st.MATH_NAMES[fn], int((~mi.same_bits(got, unfused)).sum()))


def test_host_double_libm_calls_against_50_digits(oracle):
    """kb8_project_f and PredictScale call glibc's double cos / sin / log.  On the committed seeds the host result is
    held to the rule of the GPU tests: it equals the correct rounding of the 50-digit value of the written expression,
    or that value lies within 4 double ulps of a rounding boundary (of an integer, for the ceil) and the result is one
    of the two neighbours; at most one such sample per test is the reference's to use up.

    Every sample is first evaluated in numpy's 80-bit long double; only samples whose long-double value is within 2^-40
    (relative) of a boundary, or whose host result differs from the long-double rounding, go to mpmath.

    Measured: the reference uses up 0 samples of kb8_project_f (5 calibrations x 131,584 points) and 0 of PredictScale
    (1,179,664 ratios)."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63
    # PredictScale
    (_, ratio, lsf, _), = mi.predict_scale()
    got = oracle.math_map(st.PREDICT_SCALE, ratio, lsf)
    v = np.log(ratio.astype(ld)) / ld(lsf[0])
    near = np.abs(v - np.rint(v)) <= np.abs(v) * ld(2.0) ** -40 + ld(2.0) ** -60
    idx = np.flatnonzero(near | (got != np.ceil(v).astype(np.int32)))
    ties, bad = mi.judge_predict_scale(ratio, lsf[0], got, idx)
    print(f"PredictScale: {len(idx)} of {len(ratio)} samples to mpmath, {ties} on a boundary")
    assert not bad and ties <= 1, (ties, bad[:5])
    # kb8_project_f
    total = 0
    for name, X, k, _ in mi.camera_sets(st.KB8_PROJECT):
        got = oracle.math_map(st.KB8_PROJECT, X, k)
        kr0, kr1, psi, k2, k3 = mi.kb8_project_operands(k, X)
        with np.errstate(all="ignore"):
            cand = np.zeros(len(X), bool)
            for col, kr, kk, f in ((0, kr0, k2, np.cos), (1, kr1, k3, np.sin)):
                v = kr.astype(ld) * f(psi.astype(ld)) + ld(kk)
                r = v.astype(np.float32)
                lo, hi = np.nextafter(r, np.float32(-np.inf)).astype(ld), np.nextafter(r, np.float32(np.inf)).astype(ld)
                gap = np.minimum(np.abs(v - (r.astype(ld) + lo) / 2), np.abs(v - (r.astype(ld) + hi) / 2))
                cand |= np.isfinite(v) & ((gap <= np.abs(v) * ld(2.0) ** -40) | ~mi.same_bits(got[:, col], r))
        idx = np.flatnonzero(cand)
        ties, bad = mi.judge_kb8_project(k, X, got, idx)
        print(f"kb8_project_f [{name}]: {len(idx)} of {len(X)} points to mpmath, {ties} on a boundary")
        assert not bad, bad[:5]
        total += ties
    assert total <= 1
