// The pure float arithmetic under every bit-exact claim: rounding, cv::fastAtan2, the glibc sincosf / atanf / atan2f /
// tanf restatements, the correctly rounded sqrtf, the reference's float camera models, the matchers' rotation check
// (rot_bin, three_maxima), MapPoint::PredictScale, and the keypoint grid with Frame::GetFeaturesInArea's window
// (grid_cell_of, grid_window, kp_in_window).  Nothing in the bodies is
// HIP-specific, so one text is compiled twice: by hipcc into every kernel (through omv_device.h / omv_camera.h), and by
// the host compiler into the oracle library (oracle/math_host.cpp), where it is compared bit for bit with glibc
// itself (tests/test_math_header_cpu.py) and with its own device build (omv_selftest_math,
// tests/test_math_device_gpu.py).  Every float path here must be compiled with -ffp-contract=off: the reference's
// float expressions are evaluated without fused multiply-adds, and bit-exact keypoints/descriptors depend on
// reproducing their rounding.
#pragma once
#include <stdint.h>

#include "../../include/omv.h"

// OMV_MATH_FN: the small helpers (always inlined on the device); OMV_MATH_FN_BIG: the libm bodies (the device
// compiler's choice).  A plain C++ compiler sees `static inline` for both.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OMV_MATH_FN __device__ __forceinline__
#define OMV_MATH_FN_BIG __device__ inline
#else
#include <math.h>
#define OMV_MATH_FN static inline
#define OMV_MATH_FN_BIG static inline
#endif

namespace omv {

// float <-> bits (what HIP's __float_as_uint / __uint_as_float expand to)
OMV_MATH_FN uint32_t f32_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof(u));
    return u;
}
OMV_MATH_FN float f32_from_bits(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, sizeof(f));
    return f;
}

// cvRound(float): round half to even (x86 cvtss2si under the default MXCSR).
OMV_MATH_FN int round_even(float v) { return (int)__builtin_rintf(v); }

// cv::fastAtan2 (OpenCV 4.x atan_f32, degrees, float).  Coefficients are the float products
// 0.99978784f*(float)(180/pi) etc., folded exactly as the host compiler folds them.
OMV_MATH_FN float fast_atan2_deg(float y, float x) {
    const float r2d = (float)(180.0 / 3.14159265358979323846);
    const float k1 = 0.9997878412794807f * r2d;
    const float k3 = -0.3258083974640975f * r2d;
    const float k5 = 0.1555786518463281f * r2d;
    const float k7 = -0.04432655554792128f * r2d;
    const float eps = (float)2.220446049250313080847e-16;   // (float)DBL_EPSILON
    float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((k7 * c2 + k5) * c2 + k3) * c2 + k1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((k7 * c2 + k5) * c2 + k3) * c2 + k1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// ---- single-precision sin/cos, bit-identical to the host glibc (2.35) cosf/sinf ------------------
// The reference calls cos()/sin() on a float (src/ORBextractor.cc:49), i.e. glibc's cosf/sinf.
// Those evaluate a double-precision polynomial after a one-step pi/2 reduction; we restate that
// published algorithm with the same constants and explicit fma() where the x86-64 FMA build fuses.
// The host build of this text equals the host libm bit for bit on every float of a strided sweep of |y| < 120 and
// around every branch threshold (tests/test_math_header_cpu.py); the device build equals the host build on the same
// inputs (tests/test_math_device_gpu.py).
struct SinCosTab {
    double hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3;
};
OMV_MATH_FN float sincosf_poly(double x, double x2, const SinCosTab &p, int n) {
    if ((n & 1) == 0) {
        double x3 = x * x2;
        double s1 = __builtin_fma(x2, p.s3, p.s2);
        double x7 = x3 * x2;
        double s = __builtin_fma(x3, p.s1, x);
        return (float)__builtin_fma(x7, s1, s);
    }
    double x4 = x2 * x2;
    double c2 = __builtin_fma(x2, p.c4, p.c3);
    double c1 = __builtin_fma(x2, p.c1, p.c0);
    double x6 = x4 * x2;
    double c = __builtin_fma(x4, p.c2, c1);
    return (float)__builtin_fma(x6, c2, c);
}
OMV_MATH_FN uint32_t top12(float x) { return (f32_bits(x) >> 20) & 0x7ff; }

// Valid for |y| < 120 (the reduce_fast range), which covers every angle in [0, 2*pi).
OMV_MATH_FN void glibc_sincosf(float y, float *sinp, float *cosp) {
    const SinCosTab t0 = {0x1.45F306DC9C883p+23, 0x1.921FB54442D18p0, 0x1p0, -0x1.ffffffd0c621cp-2,
                          0x1.55553e1068f19p-5, -0x1.6c087e89a359dp-10, 0x1.99343027bf8c3p-16,
                          -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13};
    const SinCosTab t1 = {0x1.45F306DC9C883p+23, 0x1.921FB54442D18p0, -0x1p0, 0x1.ffffffd0c621cp-2,
                          -0x1.55553e1068f19p-5, 0x1.6c087e89a359dp-10, -0x1.99343027bf8c3p-16,
                          -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13};
    double x = y;
    if (top12(y) < top12(0x1.921FB6p-1f)) {
        if (top12(y) < top12(0x1p-12f)) {
            *sinp = y;
            *cosp = 1.0f;
            return;
        }
        double x2 = x * x;
        *sinp = sincosf_poly(x, x2, t0, 0);
        *cosp = sincosf_poly(x, x2, t0, 1);
        return;
    }
    double r = x * t0.hpi_inv;
    int n = ((int32_t)r + 0x800000) >> 24;
    double xr = __builtin_fma(-(double)n, t0.hpi, x);
    // glibc's sign table {1, -1, -1, 1}[n & 3] as a select (an indexed table is a memory load on the device)
    double s = ((n + 1) & 2) ? -1.0 : 1.0;
    const SinCosTab &p = (n & 2) ? t1 : t0;
    *sinp = sincosf_poly(xr * s, xr * xr, p, n);
    *cosp = sincosf_poly(xr * s, xr * xr, p, n ^ 1);
}

// glibc atan2f (fdlibm e_atan2f.c / s_atanf.c), float, no contraction.  KannalaBrandt8::project
// computes theta / psi with atan2f (KannalaBrandt8.cpp:30-31, :50-51); the host build of this text is
// bit-identical to the host libm (tests/test_math_header_cpu.py: random bit patterns, the near-diagonal
// switch and the special-value cross product; atanf over the full float range).
OMV_MATH_FN_BIG float glibc_atanf(float x) {
    const float atanhi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
    const float atanlo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
    const float aT[11] = {3.3333334327e-01f, -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f,
                          9.0908870101e-02f, -7.6918758452e-02f, 6.6610731184e-02f, -5.8335702866e-02f,
                          4.9768779427e-02f, -3.6531571299e-02f, 1.6285819933e-02f};
    const int32_t hx = (int32_t)f32_bits(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c000000) {
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {
        if (ix < 0x31000000) return x;
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {
            if (ix < 0x3f300000) id = 0, x = (2.0f * x - 1.0f) / (2.0f + x);
            else id = 1, x = (x - 1.0f) / (x + 1.0f);
        } else {
            if (ix < 0x401c0000) id = 2, x = (x - 1.5f) / (1.0f + 1.5f * x);
            else id = 3, x = -1.0f / x;
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -r : r;
}
OMV_MATH_FN_BIG float glibc_atan2f(float y, float x) {
    const float pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f,
                pi_lo = -8.7422776573e-08f, tiny = 1.0e-30f;
    const int32_t hx = (int32_t)f32_bits(x), ix = hx & 0x7fffffff, hy = (int32_t)f32_bits(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return glibc_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (iy == 0) {
        if (m < 2) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) {
            const float r[4] = {pi_o_4 + tiny, -pi_o_4 - tiny, 3.0f * pi_o_4 + tiny, -3.0f * pi_o_4 - tiny};
            return r[m];
        }
        const float r[4] = {0.0f, -0.0f, pi + tiny, -pi - tiny};
        return r[m];
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = glibc_atanf(fabsf(y / x));
    switch (m) {
        case 0: return z;
        case 1: return f32_from_bits(f32_bits(z) ^ 0x80000000u);
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

// Correctly rounded f32 sqrt (libm sqrtf): v_sqrt_f32 alone is 1 ulp; the f64 sqrt is correctly
// rounded and 53 >= 2*24+2 bits make the second rounding innocuous.
OMV_MATH_FN float sqrtf_cr(float x) { return (float)sqrt((double)x); }

// glibc 2.35 tanf (std::tan(float) in KannalaBrandt8::unproject): fdlibm's __kernel_tanf after a
// double-precision reduction (pi/4 < |x| < 120: n = nearbyint(x 2/pi), r = x - n pi/2).  The host build of this
// text is bit-identical to the host libm on a strided sweep of |x| < 120 and around every branch threshold
// (tests/test_math_header_cpu.py).
OMV_MATH_FN_BIG float glibc_kernel_tanf(float x, float y, int iy) {
    const float T[] = {3.3333334327e-01f, 1.3333334029e-01f, 5.3968254477e-02f, 2.1869488060e-02f,
                       8.8632395491e-03f, 3.5920790397e-03f, 1.4562094584e-03f, 5.8804126456e-04f,
                       2.4646313977e-04f, 7.8179444245e-05f, 7.1407252108e-05f, -1.8558637748e-05f,
                       2.5907305826e-05f};
    const float pio4 = 7.8539812565e-01f, pio4lo = 3.7748947079e-08f;
    float z, r, v, w, s;
    const int32_t hx = (int32_t)f32_bits(x), ix = hx & 0x7fffffff;
    if (ix < 0x39000000) {   // |x| < 2**-13
        if ((int)x == 0) {
            if ((ix | (iy + 1)) == 0) return 1.0f / fabsf(x);
            else if (iy == 1) return x;
            else return -1.0f / x;
        }
    }
    if (ix >= 0x3f2ca140) {   // |x| >= 0.6744
        if (hx < 0) x = -x, y = -y;
        z = pio4 - x;
        w = pio4lo - y;
        x = z + w;
        y = 0.0f;
        if (fabsf(x) < 0x1p-13f) return (1 - ((hx >> 30) & 2)) * iy * (1.0f - 2 * iy * x);
    }
    z = x * x;
    w = z * z;
    r = T[1] + w * (T[3] + w * (T[5] + w * (T[7] + w * (T[9] + w * T[11]))));
    v = z * (T[2] + w * (T[4] + w * (T[6] + w * (T[8] + w * (T[10] + w * T[12])))));
    s = z * x;
    r = y + z * (s * (r + v) + y);
    r += T[0] * s;
    w = x + r;
    if (ix >= 0x3f2ca140) {
        v = (float)iy;
        return (float)(1 - ((hx >> 30) & 2)) * (v - 2.0f * (x - (w * w / (w + v) - r)));
    }
    if (iy == 1) return w;
    float a, t;
    z = f32_from_bits(f32_bits(w) & 0xfffff000u);
    v = r - (z - x);
    t = a = -1.0f / w;
    t = f32_from_bits(f32_bits(t) & 0xfffff000u);
    s = 1.0f + t * z;
    return t + a * (s + t * v);
}
OMV_MATH_FN_BIG float glibc_tanf(float x) {
    const int32_t ix = (int32_t)(f32_bits(x) & 0x7fffffffu);
    if (ix <= 0x3f490fda) return glibc_kernel_tanf(x, 0.0f, 1);
    const double xd = (double)x, nd = rint(xd * 0.6366197723675814);
    const int n = (int)nd;
    const double r = xd - nd * 1.5707963267948966;
    const float y0 = (float)r, y1 = (float)(r - (double)y0);
    return glibc_kernel_tanf(y0, y1, 1 - ((n & 1) << 1));
}

// ---- the reference's float camera models (KannalaBrandt8, Pinhole and the GeometricCamera dispatch on the camera
// type), one definition for every float kernel that projects or unprojects.  Float arithmetic without contraction, in
// the reference's operation order.  The double-precision model of the g2o edges (g2o_types.h) is a different function
// of the reference.

// KannalaBrandt8::project(const Eigen::Vector3f&) (KannalaBrandt8.cpp:48-67): cos / sin of the promoted float
// (C double functions)
OMV_MATH_FN void kb8_project_f(const float *k, const float *X, float &u, float &v) {
    const float x2y2 = X[0] * X[0] + X[1] * X[1];
    const float theta = omv::glibc_atan2f(omv::sqrtf_cr(x2y2), X[2]);
    const float psi = omv::glibc_atan2f(X[1], X[0]);
    const float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float r = theta + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9;
    u = (float)((double)(k[0] * r) * cos((double)psi) + (double)k[2]);
    v = (float)((double)(k[1] * r) * sin((double)psi) + (double)k[3]);
}

// KannalaBrandt8::unproject (precision 1e-6, <= 10 Newton steps, scale = std::tan(theta) / theta_d)
OMV_MATH_FN void kb8_unproject_f(const float *k, float px, float py, float *ray) {
    const float pwx = (px - k[2]) / k[0], pwy = (py - k[3]) / k[1];
    float scale = 1.f;
    float theta_d = omv::sqrtf_cr(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-3.14159265358979323846 / 2.f), theta_d), (float)(3.14159265358979323846 / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2,
                        theta8 = theta4 * theta4;
            const float k0_theta2 = k[4] * theta2, k1_theta4 = k[5] * theta4;
            const float k2_theta6 = k[6] * theta6, k3_theta8 = k[7] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < 1e-6f) break;
        }
        scale = omv::glibc_tanf(theta) / theta_d;
    }
    ray[0] = pwx * scale, ray[1] = pwy * scale, ray[2] = 1.f;
}

// Pinhole::unprojectEig / project(const Eigen::Vector3f&) (Pinhole.cpp:26-32, :40-45): float, left to right
OMV_MATH_FN void pinhole_unproject_f(const float *k, float px, float py, float *ray) {
    ray[0] = (px - k[2]) / k[0], ray[1] = (py - k[3]) / k[1], ray[2] = 1.f;
}
OMV_MATH_FN void pinhole_project_f(const float *k, const float *X, float &u, float &v) {
    u = k[0] * X[0] / X[2] + k[2];
    v = k[1] * X[1] / X[2] + k[3];
}
// GeometricCamera::unprojectEig / project, dispatched on the camera type (the virtual calls of
// KannalaBrandt8::TriangulateMatches on pCamera2, KannalaBrandt8.cpp:330, :382)
OMV_MATH_FN void cam_unproject_f(int model, const float *k, float px, float py, float *ray) {
    if (model == OMV_CAM_PINHOLE) pinhole_unproject_f(k, px, py, ray);
    else kb8_unproject_f(k, px, py, ray);
}
OMV_MATH_FN void cam_project_f(int model, const float *k, const float *X, float &u, float &v) {
    if (model == OMV_CAM_PINHOLE) pinhole_project_f(k, X, u, v);
    else kb8_project_f(k, X, u, v);
}

// ---- the matchers' rotation-consistency check and MapPoint::PredictScale: one definition for every search, tested
// directly on both compilers (tests/test_math_header_cpu.py, tests/test_math_device_gpu.py).
constexpr int kRotHistLen = 30;   // HISTO_LENGTH

// The histogram bin of a match: rot = angle1 - angle2 (float), +360 if negative, bin = round(rot * factor) with
// factor = 1.0f / HISTO_LENGTH and HISTO_LENGTH -> 0 (ORBmatcher.cc:475-481 and its five siblings)
OMV_MATH_FN int rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    const int bin = (int)roundf(rot * (1.0f / kRotHistLen));
    return bin == kRotHistLen ? 0 : bin;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2537-2573): the indices of the three largest bins (strict >, so the
// first of equal bins wins), the second / third only when at least 10 % of the first; -1 for an absent index.
OMV_MATH_FN void three_maxima(const int *hist, int ind[3]) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kRotHistLen; i++) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2, max2 = max1, max1 = s;
            ind3 = ind2, ind2 = ind1, ind1 = i;
        } else if (s > max2) {
            max3 = max2, max2 = s;
            ind3 = ind2, ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    const float tenth = 0.1f * (float)max1;
    if (max2 < tenth) ind2 = -1, ind3 = -1;
    else if (max3 < tenth) ind3 = -1;
    ind[0] = ind1, ind[1] = ind2, ind[2] = ind3;
}
// Whether a match in `bin` survives the check.
OMV_MATH_FN bool rot_bin_kept(int bin, const int ind[3]) { return bin == ind[0] || bin == ind[1] || bin == ind[2]; }

// MapPoint::PredictScale (MapPoint.cc:624-637): ratio = mfMaxDistance / currentDist, log in double; the level before
// and after the clamp to [0, n_levels - 1]
OMV_MATH_FN int predict_scale_raw(float ratio, float log_scale_factor) {
    return (int)ceil(log((double)ratio) / (double)log_scale_factor);
}
OMV_MATH_FN int predict_scale(float ratio, float log_scale_factor, int n_levels) {
    const int s = predict_scale_raw(ratio, log_scale_factor);
    return s < 0 ? 0 : (s >= n_levels ? n_levels - 1 : s);
}

// ---- the keypoint grid of Frame (FRAME_GRID_COLS x FRAME_GRID_ROWS) and Frame::GetFeaturesInArea's window on it: one
// definition for the grid build and for every window walk, tested directly on both compilers.  The grid floats
// (mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv) go by value.
constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;

// Frame::PosInGrid (Frame.cc:969-978) as the cell index mGrid[posX][posY], posX * rows + posY; -1 outside the grid.
OMV_MATH_FN int grid_cell_of(float x, float y, float min_x, float min_y, float invW, float invH) {
    const int px = (int)roundf((x - min_x) * invW);
    const int py = (int)roundf((y - min_y) * invH);
    if (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) return -1;
    return px * kGridRows + py;
}

// The cells a GetFeaturesInArea(x, y, r) window visits (Frame.cc:890-930) into the GridRange w, both ends inclusive;
// MISS (a statement: return, break) runs when the window misses the grid, at the reference's four early returns in
// their order (the later fields of w are then unset).  A macro because the kernels pass fields of a kernel argument:
// its operands are read where the reference reads them, after the earlier returns, while a call would read all four
// grid floats first -- which renumbers the registers of every kernel that walks a window.  grid_window() below is the
// same text as a function, and the one the tests call.
#define OMV_GRID_WINDOW_OR(x, y, r, min_x, min_y, invW, invH, w, MISS)           \
    {                                                                            \
        const int x0_ = (int)floorf(((x) - (min_x) - (r)) * (invW));             \
        (w).x0 = x0_ < 0 ? 0 : x0_;                                              \
        if ((w).x0 >= omv::kGridCols) MISS;                                      \
        const int x1_ = (int)ceilf(((x) - (min_x) + (r)) * (invW));              \
        (w).x1 = x1_ > omv::kGridCols - 1 ? omv::kGridCols - 1 : x1_;            \
        if ((w).x1 < 0) MISS;                                                    \
        const int y0_ = (int)floorf(((y) - (min_y) - (r)) * (invH));             \
        (w).y0 = y0_ < 0 ? 0 : y0_;                                              \
        if ((w).y0 >= omv::kGridRows) MISS;                                      \
        const int y1_ = (int)ceilf(((y) - (min_y) + (r)) * (invH));              \
        (w).y1 = y1_ > omv::kGridRows - 1 ? omv::kGridRows - 1 : y1_;            \
        if ((w).y1 < 0) MISS;                                                    \
    }
struct GridRange {
    int x0, x1, y0, y1;
};
OMV_MATH_FN bool grid_window(float x, float y, float r, float min_x, float min_y, float invW, float invH,
                             GridRange &g) {
    OMV_GRID_WINDOW_OR(x, y, r, min_x, min_y, invW, invH, g, return false)
    return true;
}

// GetFeaturesInArea's test of one keypoint of a visited cell (Frame.cc:932-963): the octave against [minL, maxL] when
// bCheckLevels = (minLevel > 0) || (maxLevel >= 0), then the strict box |kx - x| < r && |ky - y| < r.
OMV_MATH_FN bool kp_in_window(float kx, float ky, int octave, float x, float y, float r, int minL, int maxL) {
    if ((minL > 0) || (maxL >= 0)) {
        if (octave < minL) return false;
        if (maxL >= 0 && octave > maxL) return false;
    }
    return fabsf(kx - x) < r && fabsf(ky - y) < r;
}

}  // namespace omv
