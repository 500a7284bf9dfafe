"""Input sets of the float-layer tests (tests/test_math_header_cpu.py, tests/test_math_device_gpu.py): fixed seeds, one
definition for the CPU and the GPU side.  Every generator returns a list of (name, a, b, c) calls, each of at most
2^24 elements; the arrays are cached and must be treated as read-only.

The argument sweeps of sincosf / tanf / atanf over |y| < 120 take every 97th float bit pattern of either sign (11.6 M
patterns per sign, one call per sign), which is as dense on [0, 2 pi] as the sweep these tests replace."""
import functools
from fractions import Fraction

import numpy as np

from openmavis_amd import selftest as st
from openmavis_amd.synth_ba_const import CAMS

F32, U32 = np.float32, np.uint32
SIGN = U32(0x80000000)
B120 = 0x42f00000            # bits of 120.0f
BINF = 0x7f800000
# branch thresholds of the restatements, as float bit patterns
THRESH_SINCOS = [0x39800000, 0x3f490fdb]                                            # 2^-12, pi/4 (top12 compares)
THRESH_ATAN = [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000]
THRESH_TAN = [0x39000000, 0x3f2ca140, 0x3f490fda]
SPECIAL_BITS = [0x00000000, 0x00000001, 0x007fffff, 0x00800000]                     # 0, denormal min / max, FLT_MIN


def f32(bits):
    return np.ascontiguousarray(bits, U32).view(F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def both_signs(b):
    b = np.asarray(b, U32)
    return np.concatenate([b, b | SIGN])


def around(centre_bits, ulps):
    """Every bit pattern within +-ulps of each centre (positive patterns, clipped at 0)."""
    c = np.asarray(centre_bits, np.int64)[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]
    return np.unique(c[(c >= 0) & (c <= BINF)]).astype(U32)


def same_bits(x, y):
    """Elementwise: equal bit patterns, or both NaN (a NaN's payload and sign are the hardware's)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape
    if x.dtype.kind != "f":
        return x == y
    u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    return (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))


def mismatches(x, y):
    """Indices (first axis) at which x and y are not same_bits."""
    ok = same_bits(x, y)
    return np.flatnonzero(~ok.reshape(len(ok), -1).all(axis=1))


@functools.lru_cache(None)
def trig_edges():
    """+-256 ulps of every branch threshold of sincosf / atanf / tanf and of n pi/2, n pi/4 (n = 1..76), +-0, the
    denormal extremes and +-FLT_MIN; |y| < 120."""
    n = np.arange(1, 77, dtype=np.float64)
    multiples = bits(np.concatenate([n * (np.pi / 2), n * (np.pi / 4)]).astype(F32))
    centres = np.concatenate([np.array(THRESH_SINCOS + THRESH_ATAN + THRESH_TAN, np.int64), multiples.astype(np.int64)])
    b = np.unique(np.concatenate([around(centres, 256), np.array(SPECIAL_BITS, U32)]))
    return f32(both_signs(b[b < B120]))


@functools.lru_cache(None)
def trig():
    """sincosf, tanf (and atanf): |y| < 120."""
    sweep = np.arange(0, B120, 97, dtype=np.int64).astype(U32)
    assert sweep[-1] > bits(F32(2 * np.pi))[()] and len(sweep) <= 1 << 24
    return [("sweep+", f32(sweep), None, None), ("sweep-", f32(sweep | SIGN), None, None),
            ("edges", trig_edges(), None, None)]


@functools.lru_cache(None)
def atanf():
    full = np.arange(0, BINF, 1021, dtype=np.int64).astype(U32)
    special = np.array([BINF, 0x7fc00000, 0x7f800001, 0x7fffffff], U32)   # inf, quiet / signalling / all-ones NaN
    wide = np.concatenate([both_signs(full), both_signs(special), both_signs(around([0x4c000000, BINF - 300], 256))])
    return trig() + [("full range", f32(wide), None, None)]


ATAN2_SPECIAL = [0.0, 1.0, np.inf, 1e-45, 1.17549435e-38, 3.4028234664e38, 1e30, 1e-30]


@functools.lru_cache(None)
def atan2():
    """atan2f and fast_atan2_deg: (name, y, x)."""
    rng = np.random.default_rng(20240201)
    ry, rx = (f32(rng.integers(0, 1 << 32, 1 << 23, dtype=np.uint64).astype(U32)) for _ in range(2))
    # near the diagonal: x = y (1 +- k 2^-23), the ax >= ay switch, over every normal exponent and all four quadrants
    n = 1 << 22
    y = f32((rng.integers(1, 254, n, dtype=np.uint64) << 23 | rng.integers(0, 1 << 23, n, dtype=np.uint64)).astype(U32))
    k = rng.integers(-8, 9, n).astype(np.float64)
    x = (y.astype(np.float64) * (1.0 + k * 2.0 ** -23)).astype(F32)
    y = f32(bits(y) | (rng.integers(0, 2, n, dtype=np.uint64).astype(U32) << 31))
    x = f32(bits(x) | (rng.integers(0, 2, n, dtype=np.uint64).astype(U32) << 31))
    v = np.array(ATAN2_SPECIAL, F32)
    v = np.concatenate([v, -v, np.array([np.nan], F32)])
    assert v[3] == f32([1])[0] and len(v) == 17
    sy, sx = (g.ravel().copy() for g in np.meshgrid(v, v, indexing="ij"))
    return [("random bits", ry, rx, None), ("near diagonal", y, x, None), ("special x special", sy, sx, None)]


@functools.lru_cache(None)
def fast_atan2():
    """fast_atan2_deg additionally on integer moments (m01, m10) in [-2^20, 2^20], as IC_Angle produces them."""
    rng = np.random.default_rng(20240202)
    m01, m10 = (rng.integers(-(1 << 20), (1 << 20) + 1, 1 << 21).astype(F32) for _ in range(2))
    g = np.arange(-40, 41).astype(F32)
    gy, gx = (a.ravel().copy() for a in np.meshgrid(g, g, indexing="ij"))
    e = np.array([-(1 << 20), -1, 0, 1, 1 << 20], F32)
    ey, ex = (a.ravel().copy() for a in np.meshgrid(e, e, indexing="ij"))
    return atan2() + [("integer moments", np.concatenate([m01, gy, ey]), np.concatenate([m10, gx, ex]), None)]


@functools.lru_cache(None)
def sqrtf():
    """Every 131st non-negative float (denormals included), +inf, and the few inputs with special results."""
    sweep = np.arange(0, BINF + 1, 131, dtype=np.int64).astype(U32)
    extra = np.array(SPECIAL_BITS + [BINF, 0x7f7fffff, 0x80000000, 0xbf800000, 0x80000001, 0x7fc00000], U32)
    squares = (np.arange(1, 4097, dtype=np.float64) ** 2).astype(F32)
    return [("sweep", f32(np.concatenate([sweep, extra, around(bits(squares), 1)])), None, None)]


@functools.lru_cache(None)
def divf():
    """Random bit patterns; a denormal operand on either side; denormal quotients; exact ties.  A quotient of two floats
    can lie exactly half-way between two floats only where the result is denormal: (2 j + 1) 2^-150, reached as
    d (2 j + 1) 2^(s - 150) / (d 2^s) with d = 1, 3."""
    rng = np.random.default_rng(20240203)
    n = 1 << 22
    ra, rb = (f32(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)) for _ in range(2))
    m = 1 << 20

    def normal(lo_exp, hi_exp, cnt):   # random mantissa, biased exponent in [lo_exp, hi_exp), random sign
        return f32((rng.integers(0, 2, cnt, dtype=np.uint64) << 31 | rng.integers(lo_exp, hi_exp, cnt, dtype=np.uint64) << 23
                    | rng.integers(0, 1 << 23, cnt, dtype=np.uint64)).astype(U32))
    den = f32((rng.integers(0, 2, m, dtype=np.uint64) << 31 | rng.integers(1, 1 << 23, m, dtype=np.uint64)).astype(U32))
    mid = normal(100, 150, m)
    # denormal quotient: the divisor's exponent 126..152 above the dividend's
    num = normal(1, 100, m)
    dexp = rng.integers(1, 27, m, dtype=np.uint64)
    div = f32(((bits(num) >> 23 & U32(0xff)).astype(np.uint64) + 126 + dexp << 23
               | rng.integers(0, 1 << 23, m, dtype=np.uint64)).astype(U32))
    j = rng.integers(0, 1 << 21, m).astype(np.float64)
    s = rng.integers(24, 100, m).astype(np.float64)
    d = np.where(rng.integers(0, 2, m) == 1, 3.0, 1.0)
    tie_a = (d * (2 * j + 1) * 2.0 ** (s - 150)).astype(F32)
    tie_b = (d * 2.0 ** s).astype(F32)
    assert np.array_equal(tie_a.astype(np.float64) / tie_b.astype(np.float64), (2 * j + 1) * 2.0 ** -150)
    a = np.concatenate([den, mid, num, tie_a, -tie_a])
    b = np.concatenate([mid, den, div, tie_b, tie_b])
    return [("random bits", ra, rb, None), ("denormals and ties", a, b, None)]


@functools.lru_cache(None)
def round_even():
    rng = np.random.default_rng(20240204)
    half = np.arange(-4096, 4097, dtype=np.float64).astype(F32) + F32(0.5)
    nb = np.concatenate([half, np.nextafter(half, F32(np.inf)), np.nextafter(half, F32(-np.inf))])
    rnd = (rng.random(1 << 20) * 2.0 ** 24 - 2.0 ** 23).astype(F32)
    rnd = rnd[np.abs(rnd) < 2.0 ** 23]
    small = f32(both_signs(np.array(SPECIAL_BITS, U32)))
    return [("halves and random", np.concatenate([nb, small, rnd]), None, None)]


@functools.lru_cache(None)
def muladd_f32():
    """Triples (a, b, c) on which the fused and the unfused a * b + c differ, and the unfused value.  Selected in
    float64, where the product of two floats (48 bits) is exact, and so are both sums: c is drawn within 2 binades of
    the product (or is its negated rounding, the cancellation case), so each sum spans at most 52 bits."""
    rng = np.random.default_rng(20240205)
    n = 1 << 20
    a, b = ((rng.random(n) + 1.0) * 2.0 ** rng.integers(-20, 21, n) * rng.choice([-1.0, 1.0], n) for _ in range(2))
    a, b = a.astype(F32), b.astype(F32)
    p = a.astype(np.float64) * b.astype(np.float64)
    pr = p.astype(F32)
    c = ((rng.random(n) + 1.0) * 2.0 ** rng.integers(-2, 3, n) * rng.choice([-1.0, 1.0], n) * np.abs(p)).astype(F32)
    c[: n // 4] = -pr[: n // 4]
    fused = (p + c.astype(np.float64)).astype(F32)
    unfused = (pr.astype(np.float64) + c.astype(np.float64)).astype(F32)
    sel = bits(fused) != bits(unfused)
    assert sel.sum() >= 100000
    return a[sel], b[sel], c[sel], unfused[sel], fused[sel]


@functools.lru_cache(None)
def muladd_f64():
    """The same for doubles, selected with fractions.Fraction: fused = the exact a b + c rounded once (float(Fraction)
    rounds correctly), unfused = Python's own a * b + c (two IEEE roundings).  Half of the candidates cancel the
    rounded product (c = -(a * b))."""
    rng = np.random.default_rng(20240206)
    n = 180000
    a, b = ((rng.random(n) + 1.0) * 2.0 ** rng.integers(-30, 31, n) * rng.choice([-1.0, 1.0], n) for _ in range(2))
    c = (rng.random(n) + 1.0) * 2.0 ** rng.integers(-2, 3, n) * rng.choice([-1.0, 1.0], n) * np.abs(a * b)
    c[: n // 2] = -(a * b)[: n // 2]
    keep, un, fu = [], [], []
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        f = float(Fraction(x) * Fraction(y) + Fraction(z))
        u = x * y + z
        if f != u:
            keep.append(i), un.append(u), fu.append(f)
    assert len(keep) >= 100000, len(keep)
    keep = np.array(keep)
    return a[keep], b[keep], c[keep], np.array(un), np.array(fu)


@functools.lru_cache(None)
def rcp_nr():
    """2^22 doubles with a normal reciprocal: random mantissas at exponents -1000..1000, and the mantissas 1, 1 + eps,
    2 - eps at every one of those exponents; both signs."""
    rng = np.random.default_rng(20240207)
    e = np.arange(-1000, 1001)
    edge = np.concatenate([np.ldexp(m, e) for m in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52)])
    n = (1 << 22) - 2 * len(edge)
    rnd = np.ldexp(1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52, rng.integers(-1000, 1001, n))
    rnd *= rng.choice([-1.0, 1.0], n)
    x = np.concatenate([edge, -edge, rnd])
    assert len(x) == 1 << 22
    return [("all", x, None, None)]


W, H = 720, 540
CALIBS = [("hilti cam%d" % (i + 1), np.array(k, F32)) for i, k in enumerate(CAMS)] + \
         [("no distortion", np.array(CAMS[0][:4] + [0.0] * 4, F32))]


@functools.lru_cache(None)
def project_points():
    """Points for kb8_project_f / pinhole_project_f: directions from the axis to behind the camera (theta up to pi),
    |X| from 1e-3 to 1e4, on the axis with both zero signs, and x or y exactly 0."""
    rng = np.random.default_rng(20240208)
    n = 1 << 17
    theta = rng.random(n) * np.pi
    theta[: n // 2] = rng.random(n // 2) * 1.2          # half of them inside the field of view
    psi = rng.random(n) * 2 * np.pi
    rad = 10.0 ** (rng.random(n) * 7 - 3)
    X = (rad[:, None] * np.stack([np.sin(theta) * np.cos(psi), np.sin(theta) * np.sin(psi), np.cos(theta)], 1)).astype(F32)
    # a coordinate exactly 0 (either sign): four points each.  There psi is +-pi/2 or pi as a float, sin / cos (psi) is
    # within 1e-15 of +-1, and k r sin(psi) + c is the sum of two floats to within a double ulp: it lands on the
    # midpoint of two floats about once in 16 points, where any double evaluation, glibc's included, rounds the tie
    # and not the exact value.  A handful exercises the branch; thousands would only count such midpoints.
    X[0:4, 0] = 0.0
    X[4:8, 0] = -0.0
    X[8:12, 1] = 0.0
    X[12:16, 1] = -0.0
    z = (10.0 ** (rng.random(64) * 7 - 3)).astype(F32)
    axis = np.concatenate([np.stack([np.full(64, sx, F32), np.full(64, sy, F32), sz * z], 1)
                           for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (1.0, -1.0)])
    return np.ascontiguousarray(np.concatenate([X, axis]), F32)


def newton_steps(k, px):
    """How many Newton steps kb8_unproject_f takes per pixel (0: the scale = 1 branch), from a float32 restatement
    that is used to describe the input set only, never as a reference.  Also returns the clamped flag."""
    k = np.asarray(k, F32)
    pwx, pwy = (px[:, 0] - k[2]) / k[0], (px[:, 1] - k[3]) / k[1]
    td = np.sqrt((pwx * pwx + pwy * pwy).astype(np.float64)).astype(F32)
    clamped = td > F32(np.pi / 2)
    td = np.minimum(td, F32(np.pi / 2))
    th, steps, live = td.copy(), np.zeros(len(td), int), td.astype(np.float64) > 1e-8
    for _ in range(10):
        t2 = th * th
        t4 = t2 * t2
        t6, t8 = t4 * t2, t4 * t4
        a, b, c, d = k[4] * t2, k[5] * t4, k[6] * t6, k[7] * t8
        fix = (th * (1 + a + b + c + d) - td) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
        th = np.where(live, th - fix, th)
        steps += live
        live = live & ~(np.abs(fix) < F32(1e-6))
    return steps, clamped


@functools.lru_cache(None)
def unproject_pixels(ci):
    """Pixels for kb8_unproject_f / pinhole_unproject_f with calibration CALIBS[ci]: a grid over the image plus a 50 %
    margin, the principal point itself (theta_d = 0: the scale = 1 branch) and its neighbours, rings of radius around
    and beyond fx pi / 2 (the clamp).  Where all 10 Newton steps are needed is a property of the calibration; the test
    counts them with newton_steps()."""
    k = CALIBS[ci][1].astype(np.float64)
    rng = np.random.default_rng(20240209 + ci)
    gx, gy = np.meshgrid(np.arange(-W / 2, 1.5 * W + 1, 3.0), np.arange(-H / 2, 1.5 * H + 1, 3.0))
    grid = np.stack([gx.ravel(), gy.ravel()], 1) + rng.random((gx.size, 2))
    grid[::7] = np.round(grid[::7])                      # keypoint coordinates are often integers at level 0
    pp = np.array([[k[2], k[3]]]) + np.array([[0, 0], [1e-5, 0], [0, -1e-5], [1e-3, 1e-3], [-0.5, 0.25]])
    ang = rng.random(4096) * 2 * np.pi
    r = k[0] * (np.pi / 2) * np.concatenate([rng.random(2048) * 0.1 + 0.95, 10.0 ** (rng.random(2048) * 2)])
    ring = np.stack([k[2] + r * np.cos(ang), k[3] + r * np.sin(ang)], 1)
    return np.ascontiguousarray(np.concatenate([grid, pp, ring]), F32)


LSF = np.array([np.log(1.2)], F32)   # mfLogScaleFactor = (float)log(1.2)


@functools.lru_cache(None)
def predict_scale():
    """Ratios within +-4096 ulps of float(1.2^k), k = -3..12 (where the ceil flips), and 2^20 random ratios in
    [0.3, 10]."""
    rng = np.random.default_rng(20240210)
    centres = bits((1.2 ** np.arange(-3, 13, dtype=np.float64)).astype(F32))
    rnd = (0.3 + rng.random(1 << 20) * 9.7).astype(F32)
    return [("all", np.concatenate([f32(around(centres, 4096)), rnd]), LSF, None)]


N_LEVELS = 8                         # the pyramid levels PredictScale is clamped to in the clamp test


def predict_scale_clamp_ends():
    """Ratios at the two ends of PredictScale's clamp for LSF and N_LEVELS: the float neighbours of 1.2^k for k = -2, -1, 0
    (raw levels below 0 up to the first kept one) and k = N_LEVELS - 2 .. N_LEVELS + 1 (the last unclamped level, then at
    and above N_LEVELS), and ratios far outside (raw -12 and 25)."""
    k = np.array([-2, -1, 0, N_LEVELS - 2, N_LEVELS - 1, N_LEVELS, N_LEVELS + 1], np.float64)
    return np.concatenate([f32(around(bits((1.2 ** k).astype(F32)), 8)), np.array([0.1, 90.0], F32)])


@functools.lru_cache(None)
def rot_angles():
    """The angles whose every ordered pair goes through rot_bin: a 0.5 degree grid over [0, 360); the two float
    neighbours of every rot in (0, 360) at which rot / 30 is a half-integer (15, 45, ..., 345; paired with 0 they are
    the difference itself); 0, the largest float below 360, and the smallest denormal and FLT_MIN, whose pairs with 0
    give the smallest negative differences, which + 360 round to exactly 360."""
    grid = np.arange(0, 720, dtype=np.float64) * 0.5
    half = (np.arange(12, dtype=np.float64) * 30 + 15).astype(F32)
    nb = np.concatenate([np.nextafter(half, F32(0)), np.nextafter(half, F32(360))])
    edge = np.concatenate([f32([0x00000000, 0x00000001, 0x00800000]), [np.nextafter(F32(360), F32(0))]])
    a = np.unique(np.concatenate([grid.astype(F32), nb, edge]).astype(F32))
    assert a.min() == 0 and a.max() < 360 and 700 < len(a) < 800
    return a


@functools.lru_cache(None)
def rot_bin():
    """(name, angle1, angle2): all ordered pairs of rot_angles()."""
    a = rot_angles()
    a1, a2 = (g.ravel().copy() for g in np.meshgrid(a, a, indexing="ij"))
    return [("all pairs", a1, a2, None)]


def rot_bin_ref(a1, a2):
    """ORBmatcher.cc:475-481 in float32, one IEEE operation per step; round() is half away from zero (the products
    are >= 0 and far below 2^23, so floor(v + 0.5) in float64 is exact)."""
    rot = a1 - a2
    rot = np.where(rot < 0, rot + F32(360.0), rot)
    v = rot * (F32(1.0) / F32(30))
    assert rot.dtype == F32 and v.dtype == F32
    b = np.floor(v.astype(np.float64) + 0.5).astype(np.int32)
    return np.where(b == 30, 0, b).astype(np.int32)


@functools.lru_cache(None)
def three_maxima():
    """About 2,000 histograms [n][30] int32: all zero; one non-empty bin at each position; equal counts in two, three
    and all bins; for max1 in {10, 20, 30, 100, 1000} the second and third counts at max1 / 10 - 1, max1 / 10 and
    max1 / 10 + 1 (the 10 % rule at its boundary), the three bins in every order of position; 800 random histograms
    with counts 0..3 (many ties); 800 with counts up to 2^20."""
    rng = np.random.default_rng(20240213)
    n = st.ROT_HIST_LEN
    h = [np.zeros((1, n), np.int32), np.eye(n, dtype=np.int32) * 7]
    for k in (2, 3):
        e = np.zeros((40, n), np.int32)
        for r in e:
            r[rng.choice(n, k, replace=False)] = 5
        h.append(e)
    h.append(np.full((1, n), 4, np.int32))
    rule = []
    for max1 in (10, 20, 30, 100, 1000):
        for s2 in (max1 // 10 - 1, max1 // 10, max1 // 10 + 1):
            for s3 in (max1 // 10 - 1, max1 // 10, max1 // 10 + 1):
                for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                    r = np.zeros(n, np.int32)
                    pos = np.sort(rng.choice(n, 3, replace=False))
                    r[pos[list(order)]] = (max1, s2, s3)
                    rule.append(r)
    h.append(np.array(rule))
    h.append(rng.integers(0, 4, (800, n)).astype(np.int32))
    h.append(rng.integers(0, (1 << 20) + 1, (800, n)).astype(np.int32))
    h = np.ascontiguousarray(np.concatenate(h))
    assert 1900 <= len(h) <= 2100
    return [("all", h, None, None)]


def three_maxima_ref(hists):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2537-2573), the literal loop; the 10 % products in float32."""
    out = np.empty((len(hists), 3), np.int32)
    for r, hist in enumerate(hists.tolist()):
        max1 = max2 = max3 = 0
        ind1 = ind2 = ind3 = -1
        for i, s in enumerate(hist):
            if s > max1:
                max3, max2, max1 = max2, max1, s
                ind3, ind2, ind1 = ind2, ind1, i
            elif s > max2:
                max3, max2 = max2, s
                ind3, ind2 = ind2, i
            elif s > max3:
                max3, ind3 = s, i
        if F32(max2) < F32(0.1) * F32(max1):
            ind2 = ind3 = -1
        elif F32(max3) < F32(0.1) * F32(max1):
            ind3 = -1
        out[r] = (ind1, ind2, ind3)
    return out


# ---- the keypoint grid and GetFeaturesInArea's window (omv::grid_cell_of / grid_window / kp_in_window) ----
GRID_COLS, GRID_ROWS = 64, 48
GRID_FRAMES = (("synthetic 720x540", 720, 540), ("pinhole 1920x1080", 1920, 1080))   # the suite's two frame geometries


def grid_floats(width, height):
    """(min_x, min_y, invW, invH) of a frame whose bounds are the image (Frame.cc:1878-1879, float)."""
    return np.array([0, 0, F32(GRID_COLS) / F32(width), F32(GRID_ROWS) / F32(height)], F32)


def _ulps(v):
    """v and its two float neighbours."""
    v = np.asarray(v, F32).ravel()
    return np.concatenate([np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))])


@functools.lru_cache(None)
def grid_windows(width, height):
    """(x, y, r) [n][3] for one geometry: window edges x -+ r (y -+ r) exactly on cell boundaries and one ulp to either
    side; windows off the grid on each side, just on and just off it; windows clipped by each clamp; r = 0; r larger
    than the image; 300 random windows around the image."""
    rng = np.random.default_rng(20240301 + width)
    cw, ch = width / GRID_COLS, height / GRID_ROWS   # 11.25 x 11.25 and 30 x 22.5: exact floats
    rows = []
    for r in (0.0, 4.0, 7.5, cw, 2.5 * 1.2 ** 3):
        for c in (0, 1, 7, 31, 62, 63, 64):      # column boundaries under the left and the right edge
            for x in np.concatenate([_ulps(c * cw + r), _ulps(c * cw - r)]):
                rows.append((x, 0.37 * height, r))
        for c in (0, 1, 5, 23, 46, 47, 48):      # row boundaries under the top and the bottom edge
            for y in np.concatenate([_ulps(c * ch + r), _ulps(c * ch - r)]):
                rows.append((0.61 * width, y, r))
    for r in (0.0, 3.0, 40.0):
        # off the grid: x - r at / past the right bound, x + r a whole cell left of 0, the same for y; and just on it
        for x in np.concatenate([_ulps(width + r), [width + r + 100], _ulps(-cw - r), [-cw - r - 100]]):
            rows.append((x, 0.5 * height, r))
        for y in np.concatenate([_ulps(height + r), [height + r + 100], _ulps(-ch - r), [-ch - r - 100]]):
            rows.append((0.5 * width, y, r))
        # x fine and y off, so that the third and the fourth return are reached after the first two pass
        rows += [(3.0, height + r + 1, r), (width - 3.0, -ch - r - 1, r)]
    for r in (15.0, 60.0):   # each clamp alone, then all four
        rows += [(r / 2, 0.5 * height, r), (width - r / 2, 0.5 * height, r), (0.5 * width, r / 2, r),
                 (0.5 * width, height - r / 2, r)]
    for r in (0.0, 2.0 * width, 5000.0):
        rows += [(0.0, 0.0, r), (0.5 * width, 0.5 * height, r), (float(width), float(height), r), (-r, -r, r)]
    n = 300
    rnd = np.stack([rng.uniform(-60, width + 60, n), rng.uniform(-60, height + 60, n),
                    rng.choice([2.5, 4.0, 6.0, 10.0, 14.93, 50.0, 100.0], n)], 1)
    return np.ascontiguousarray(np.concatenate([np.array(rows, np.float64), rnd]), F32)


@functools.lru_cache(None)
def grid_keypoints(width, height):
    """(x, y) [n][2] for one geometry: the image border and one ulp outside / inside it; the cell centres' edges, where
    roundf changes cell (half away from zero), +- one ulp; the last cell's far edge, where the keypoint leaves the
    grid; 300 random keypoints; a few outside the image; four keypoints just inside the box of every window of
    grid_windows()."""
    rng = np.random.default_rng(20240302 + width)
    cw, ch = width / GRID_COLS, height / GRID_ROWS
    xs = np.concatenate([_ulps([0.0, width, -0.5 * cw, (GRID_COLS - 0.5) * cw]), _ulps((np.array([0, 1, 31, 62, 63]) + 0.5) * cw)])
    ys = np.concatenate([_ulps([0.0, height, -0.5 * ch, (GRID_ROWS - 0.5) * ch]), _ulps((np.array([0, 1, 23, 46, 47]) + 0.5) * ch)])
    rows = [(x, 0.37 * height) for x in xs] + [(0.61 * width, y) for y in ys]
    rows += [(x, y) for x in _ulps([0.0, width]) for y in _ulps([0.0, height])]
    rows += [(-30.0, 10.0), (width + 30.0, 10.0), (10.0, -30.0), (10.0, height + 30.0)]
    rnd = np.stack([rng.uniform(0, width, 300), rng.uniform(0, height, 300)], 1)
    # just inside the box of every window of the set, at its left / right and top / bottom edge: the keypoints a
    # window admits that are nearest to the cells it might not visit
    win = grid_windows(width, height)
    win = win[win[:, 2] > 0]
    x, y, r = win[:, 0], win[:, 1], win[:, 2]
    edge = np.concatenate([np.stack([np.nextafter(x - r, F32(np.inf)), y], 1), np.stack([np.nextafter(x + r, F32(-np.inf)), y], 1),
                           np.stack([x, np.nextafter(y - r, F32(np.inf))], 1), np.stack([x, np.nextafter(y + r, F32(-np.inf))], 1)])
    return np.ascontiguousarray(np.concatenate([np.array(rows, np.float64), rnd, edge]), F32)


@functools.lru_cache(None)
def kp_window_cases(width, height):
    """[n][8] (kx, ky, octave, x, y, r, minL, maxL) for one geometry: 400 random keypoints near random windows with
    every level rule -- minL 0 and above, maxL -1 (with minL 0: bCheckLevels false), equal to and above the octave,
    below it -- and keypoints at |kx - x| == r and |ky - y| == r exactly and one ulp to either side (the test is
    strict)."""
    rng = np.random.default_rng(20240303 + width)
    rows = []
    levels = lambda o: [(0, -1), (1, -1), (o + 1, -1), (0, o), (o, o), (o - 1, o), (0, o + 2), (o + 1, o + 2), (0, o - 1), (-1, -1)]
    for _ in range(40):
        x, y, r = rng.uniform(0, width), rng.uniform(0, height), float(rng.choice([2.5, 4.0, 14.93, 50.0]))
        kx, ky, o = x + rng.uniform(-1.2, 1.2) * r, y + rng.uniform(-1.2, 1.2) * r, int(rng.integers(0, 8))
        rows += [(kx, ky, o, x, y, r, lo, hi) for lo, hi in levels(o)]
    for r in (0.0, 2.5, 4.0, 7.5):   # x, y, r chosen so that x + r and x - r are exact: the keypoint sits on the box
        x, y = F32(0.25 * width + 0.5), F32(0.75 * height + 0.25)
        for kx in np.concatenate([_ulps(x + F32(r)), _ulps(x - F32(r))]):
            rows += [(kx, y, 2, x, y, r, 1, 2), (kx, y, 2, x, y, r, 0, -1)]
        for ky in np.concatenate([_ulps(y + F32(r)), _ulps(y - F32(r))]):
            rows += [(x, ky, 2, x, y, r, 1, 2), (x, ky, 2, x, y, r, 0, -1)]
    return np.ascontiguousarray(np.array(rows, np.float64), F32)


def grid_cell_of_ref(kp, g):
    """Frame::PosInGrid (Frame.cc:969-978) in float32, one IEEE operation per step; round() is half away from zero."""
    v = [(kp[:, 0] - g[0]) * g[2], (kp[:, 1] - g[1]) * g[3]]
    assert v[0].dtype == F32
    px, py = (np.copysign(np.floor(np.abs(u).astype(np.float64) + 0.5), u).astype(np.int64) for u in v)
    out = (px < 0) | (px >= GRID_COLS) | (py < 0) | (py >= GRID_ROWS)
    return np.where(out, -1, px * GRID_ROWS + py).astype(np.int32)


def grid_window_ref(win, g):
    """Frame.cc:890-930 in float32: ([n][4] min / max column, min / max row, four -1 for a window that misses the grid;
    [n] which of the four early returns was taken, 0 none; [n][4] whether each clamp changed its value)."""
    x, y, r = win[:, 0], win[:, 1], win[:, 2]
    raw = [np.floor((x - g[0] - r) * g[2]), np.ceil((x - g[0] + r) * g[2]), np.floor((y - g[1] - r) * g[3]),
           np.ceil((y - g[1] + r) * g[3])]
    assert all(v.dtype == F32 for v in raw)
    raw = [v.astype(np.int64) for v in raw]
    cl = [np.maximum(0, raw[0]), np.minimum(GRID_COLS - 1, raw[1]), np.maximum(0, raw[2]), np.minimum(GRID_ROWS - 1, raw[3])]
    miss = [cl[0] >= GRID_COLS, cl[1] < 0, cl[2] >= GRID_ROWS, cl[3] < 0]
    ret = np.zeros(len(win), np.int32)
    for k in (3, 2, 1, 0):
        ret = np.where(miss[k], k + 1, ret)
    rng4 = np.where((ret > 0)[:, None], -1, np.stack(cl, 1)).astype(np.int32)
    return rng4, ret, np.stack([c != v for c, v in zip(cl, raw)], 1)


def kp_in_window_ref(e):
    """Frame.cc:932-963 for one keypoint of a visited cell, in float32."""
    kx, ky, o, x, y, r, lo, hi = (e[:, k] for k in range(8))
    check = (lo > 0) | (hi >= 0)
    lvl_ok = ~check | ((o >= lo) & ((hi < 0) | (o <= hi)))
    return (lvl_ok & (np.abs(kx - x) < r) & (np.abs(ky - y) < r)).astype(np.int32)


def grid_cell_of():
    return [(name, grid_keypoints(w, h), grid_floats(w, h), None) for name, w, h in GRID_FRAMES]


def grid_window():
    return [(name, grid_windows(w, h), grid_floats(w, h), None) for name, w, h in GRID_FRAMES]


def kp_in_window():
    return [(name, kp_window_cases(w, h), None, None) for name, w, h in GRID_FRAMES]


# fn -> the calls of its input set, for the functions with plain [n] arguments
SETS = {st.SINCOSF: trig, st.TANF: trig, st.ATANF: atanf, st.ATAN2F: atan2, st.FAST_ATAN2_DEG: fast_atan2,
        st.SQRTF: sqrtf, st.DIVF: divf, st.ROUND_EVEN: round_even, st.RCP_NR: rcp_nr, st.PREDICT_SCALE: predict_scale,
        st.ROT_BIN: rot_bin, st.THREE_MAXIMA: three_maxima, st.GRID_CELL_OF: grid_cell_of, st.GRID_WINDOW: grid_window,
        st.KP_IN_WINDOW: kp_in_window}


def camera_sets(fn):
    """The calls of a camera code: one per calibration (b = k[8])."""
    if fn in (st.KB8_PROJECT, st.PINHOLE_PROJECT):
        return [(name, project_points(), k, None) for name, k in CALIBS]
    return [(name, unproject_pixels(ci), k, None) for ci, (name, k) in enumerate(CALIBS)]


# ---- the two functions that call a double libm function (cos / sin in kb8_project_f, log in PredictScale) ----
# Device and host libraries may round a double cos / sin / log differently in the last place.  That can change the
# float (or the integer) only when the exact value of the written expression sits on a rounding boundary; the rule
# below accepts exactly that and nothing else.

def kb8_project_operands(k, X):
    """The double operands of kb8_project_f's last line for each point: (k0 r, k1 r, psi, k2, k3) with r and psi from
    the float chain (atan2f / sqrtf through the host header, the polynomial in numpy float32, left to right)."""
    import oracle
    k, X = np.asarray(k, F32), np.asarray(X, F32)
    x2y2 = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
    theta = oracle.math_map(st.ATAN2F, oracle.math_map(st.SQRTF, x2y2), X[:, 2].copy())
    psi = oracle.math_map(st.ATAN2F, X[:, 1].copy(), X[:, 0].copy())
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9
    return (k[0] * r).astype(np.float64), (k[1] * r).astype(np.float64), psi.astype(np.float64), float(k[2]), float(k[3])


def _ulp64(v):
    import mpmath
    return mpmath.ldexp(1, int(mpmath.floor(mpmath.log(abs(v), 2))) - 52) if v != 0 else mpmath.mpf(2) ** -1074


def float_tie_ok(value, got):
    """value: the 50-digit value of the expression; got: a float32 result.  True when `got` is the correct rounding;
    "tie" when value lies within 4 double ulps of the boundary between the two floats around it and got is one of
    them; False otherwise."""
    import mpmath
    near = F32(float(value))                      # some float next to value (double rounding cannot move it further)
    cands = sorted({float(near), float(np.nextafter(near, F32(-np.inf))), float(np.nextafter(near, F32(np.inf)))})
    lo = max(c for c in cands if mpmath.mpf(c) <= value)
    hi = min(c for c in cands if mpmath.mpf(c) >= value)
    if lo == hi:
        return float(got) == lo
    mid = (mpmath.mpf(lo) + mpmath.mpf(hi)) / 2
    right = lo if value < mid else hi if value > mid else (lo if (bits(F32(lo))[()] & 1) == 0 else hi)
    if float(got) == right:
        return True
    return "tie" if abs(value - mid) <= 4 * _ulp64(value) and float(got) in (lo, hi) else False


def ceil_tie_ok(value, got):
    """The same for (int)ceil(value): "tie" when value is within 4 double ulps of an integer n and got is n or n + 1."""
    import mpmath
    if int(got) == int(mpmath.ceil(value)):
        return True
    n = int(mpmath.nint(value))
    return "tie" if abs(value - n) <= 4 * _ulp64(value) and int(got) in (n, n + 1) else False


def kb8_project_exact(kr, psi, k2, which):
    import mpmath
    f = mpmath.cos if which == 0 else mpmath.sin
    return mpmath.mpf(kr) * f(mpmath.mpf(psi)) + mpmath.mpf(k2)


def predict_scale_exact(ratio, lsf):
    import mpmath
    return mpmath.log(mpmath.mpf(float(ratio))) / mpmath.mpf(float(lsf))


def judge_kb8_project(k, X, got, idx):
    """Apply the rule to the points `idx` of one KB8_PROJECT call: (number of ties, list of failures)."""
    import mpmath
    ties, bad = 0, []
    kr0, kr1, psi, k2, k3 = kb8_project_operands(k, X[idx])
    with mpmath.workdps(50):
        for j, i in enumerate(idx):
            for which, kr, kk in ((0, kr0[j], k2), (1, kr1[j], k3)):
                g = got[i, which]
                v = kb8_project_exact(kr, psi[j], kk, which)
                if not (mpmath.isfinite(v) and np.isfinite(g)):
                    ok = bool(np.isnan(g)) == bool(mpmath.isnan(v))
                else:
                    ok = float_tie_ok(v, g)
                if ok == "tie":
                    ties += 1
                    print(f"kb8_project tie: X {X[i]} component {which} exact {mpmath.nstr(v, 25)} got {g!r}")
                elif not ok:
                    bad.append((int(i), which, float(g), mpmath.nstr(v, 25)))
    return ties, bad


def judge_predict_scale(ratio, lsf, got, idx):
    import mpmath
    ties, bad = 0, []
    with mpmath.workdps(50):
        for i in idx:
            v = predict_scale_exact(ratio[i], lsf)
            ok = ceil_tie_ok(v, got[i])
            if ok == "tie":
                ties += 1
                print(f"predict_scale tie: ratio {ratio[i]!r} exact {mpmath.nstr(v, 25)} got {got[i]}")
            elif not ok:
                bad.append((int(i), float(ratio[i]), int(got[i]), mpmath.nstr(v, 25)))
    return ties, bad


# ---- known answers of this project's libm (tests/golden/libm_kat.npz, written by tools/make_golden.py) ----
KAT_F32, KAT_F64 = 2000, 900


@functools.lru_cache(None)
def kat_inputs():
    """name -> argument tuple of the libm known-answer test: float sinf / cosf / tanf / atanf / atan2f (2,000 each, half
    from the branch-threshold neighbourhoods) and double cos / sin / log (900 each) on promoted floats, as
    kb8_project_f and PredictScale call them."""
    rng = np.random.default_rng(20240211)
    edges = trig_edges()
    trig_in = np.concatenate([rng.choice(edges, KAT_F32 // 2, replace=False),
                              f32(rng.integers(0, B120, KAT_F32 // 2, dtype=np.uint64).astype(U32)
                                  | (rng.integers(0, 2, KAT_F32 // 2, dtype=np.uint64).astype(U32) << 31))])
    wide = atanf()[-1][1]
    atan_in = np.concatenate([rng.choice(edges, KAT_F32 // 2, replace=False), rng.choice(wide, KAT_F32 // 2, replace=False)])
    sets = atan2()
    pick = rng.choice(len(sets[0][1]), KAT_F32 - 800, replace=False)
    pick2 = rng.choice(len(sets[1][1]), 800 - 289, replace=False)
    y = np.concatenate([sets[0][1][pick], sets[1][1][pick2], sets[2][1]])
    x = np.concatenate([sets[0][2][pick], sets[1][2][pick2], sets[2][2]])
    psi = ((rng.random(KAT_F64) * 2 - 1) * np.pi).astype(F32).astype(np.float64)
    ratio = (0.3 + rng.random(KAT_F64) * 9.7).astype(F32).astype(np.float64)
    return {"sinf": (trig_in,), "cosf": (trig_in,), "tanf": (trig_in,), "atanf": (atan_in,), "atan2f": (y, x),
            "cos": (psi,), "sin": (psi,), "log": (ratio,)}


def kat_eval():
    """The running C library on kat_inputs(): name -> outputs."""
    import ctypes
    import ctypes.util
    import oracle
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    ins = kat_inputs()
    sc = oracle.libm_map(st.SINCOSF, ins["sinf"][0])
    out = {"sinf": sc[:, 0].copy(), "cosf": sc[:, 1].copy(), "tanf": oracle.libm_map(st.TANF, ins["tanf"][0]),
           "atanf": oracle.libm_map(st.ATANF, ins["atanf"][0]), "atan2f": oracle.libm_map(st.ATAN2F, *ins["atan2f"])}
    for name in ("cos", "sin", "log"):
        f = getattr(libm, name)
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
        out[name] = np.array([f(v) for v in ins[name][0].tolist()])
    return out
