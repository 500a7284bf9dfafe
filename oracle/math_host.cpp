// =====================================================================================================
// TEST INFRASTRUCTURE ONLY — the product's float layer on the host.  Never linked into the product.
//
// oracle_math_map:  openmavis_amd/csrc/omv_math.h itself (the text hipcc compiles into every kernel), built by the
//                   host compiler with the oracle's flags (-ffp-contract=off), through the same per-element switch
//                   as the device hook omv_selftest_math (csrc/omv_math_map.h).  RCP_NR is the IEEE quotient here
//                   (rcp_nr is a device routine).
// oracle_libm_map:  the same fn codes through the C library and the oracle's existing restatements, restating
//                   nothing: sinf / cosf / atanf / atan2f / tanf / sqrtf / nearbyintf, double cos / sin / log / ceil
//                   inside the oracle's kb8_project_f (match_oracle.cpp), kb8_unproject_f (tri_oracle.cpp) and the
//                   PredictScale expression, oracle_fast_atan2 (orb_oracle.cpp).  DIVF, the MULADD probes, RCP_NR,
//                   ROT_BIN, THREE_MAXIMA, PREDICT_SCALE_CLAMPED and the three grid codes have no libm counterpart
//                   (return 1): numpy, exact arithmetic and the tests' literal restatements of the reference lines
//                   are their references.
// The chain the tests assert: device build of the header == host build (GPU tests), host build == this glibc (CPU
// tests), this glibc == recorded answers (tests/golden/libm_kat.npz).
// =====================================================================================================
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "../openmavis_amd/csrc/omv_math_map.h"

extern "C" {
float oracle_fast_atan2(float y, float x);                                  // orb_oracle.cpp
void oracle_kb8_project(const float *cam, const float *X, float *uv);       // match_oracle.cpp
void oracle_pinhole_project(const float *cam, const float *X, float *uv);   // match_oracle.cpp
void oracle_kb8_unproject(const float *cam, float x, float y, float *ray);  // tri_oracle.cpp
void oracle_pinhole_unproject(const float *cam, float x, float y, float *ray);
}

namespace {

template <class F>
void parallel_chunks(int64_t n, F f) {
    const int64_t kMin = 1 << 16;
    int nt = (int)std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), (n + kMin - 1) / kMin);
    if (nt <= 1) {
        f((int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(f, n * t / nt, n * (t + 1) / nt);
    for (auto &t : th) t.join();
}

bool libm_one(int fn, int64_t i, const void *a, const void *b, void *out) {
    const float *af = (const float *)a, *bf = (const float *)b;
    float *of = (float *)out;
    int32_t *oi = (int32_t *)out;
    switch (fn) {
        case OMV_MATH_SINCOSF: of[2 * i] = sinf(af[i]), of[2 * i + 1] = cosf(af[i]); return true;
        case OMV_MATH_ATANF: of[i] = atanf(af[i]); return true;
        case OMV_MATH_ATAN2F: of[i] = atan2f(af[i], bf[i]); return true;
        case OMV_MATH_TANF: of[i] = tanf(af[i]); return true;
        case OMV_MATH_SQRTF: of[i] = sqrtf(af[i]); return true;
        case OMV_MATH_FAST_ATAN2_DEG: of[i] = oracle_fast_atan2(af[i], bf[i]); return true;
        case OMV_MATH_ROUND_EVEN: oi[i] = (int)nearbyintf(af[i]); return true;
        case OMV_MATH_KB8_PROJECT: oracle_kb8_project(bf, af + 3 * i, of + 2 * i); return true;
        case OMV_MATH_KB8_UNPROJECT: oracle_kb8_unproject(bf, af[2 * i], af[2 * i + 1], of + 3 * i); return true;
        case OMV_MATH_PINHOLE_PROJECT: oracle_pinhole_project(bf, af + 3 * i, of + 2 * i); return true;
        case OMV_MATH_PINHOLE_UNPROJECT: oracle_pinhole_unproject(bf, af[2 * i], af[2 * i + 1], of + 3 * i); return true;
        case OMV_MATH_PREDICT_SCALE: oi[i] = (int)std::ceil(std::log((double)af[i]) / (double)bf[0]); return true;
        default: return false;
    }
}

bool args_ok(int fn, int64_t n, const void *a, const void *b, const void *c, const void *out) {
    omv::MathShape s;
    if (!omv::math_shape(fn, &s) || n < 0) return false;
    return n == 0 || (a && out && (!s.b || b) && (!s.c || c));
}

}  // namespace

extern "C" {

int oracle_math_map(int fn, int64_t n, const void *a, const void *b, const void *c, void *out) {
    if (!args_ok(fn, n, a, b, c, out)) return 1;
    parallel_chunks(n, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) omv::math_map_one(fn, i, a, b, c, out);
    });
    return 0;
}

int oracle_libm_map(int fn, int64_t n, const void *a, const void *b, const void *c, void *out) {
    if (!args_ok(fn, n, a, b, c, out)) return 1;
    if (fn == OMV_MATH_DIVF || fn == OMV_MATH_MULADD_F32 || fn == OMV_MATH_MULADD_F64 || fn == OMV_MATH_RCP_NR ||
        fn == OMV_MATH_ROT_BIN || fn == OMV_MATH_THREE_MAXIMA || fn >= OMV_MATH_PREDICT_SCALE_CLAMPED)
        return 1;
    parallel_chunks(n, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) libm_one(fn, i, a, b, out);
    });
    return 0;
}

}  // extern "C"
