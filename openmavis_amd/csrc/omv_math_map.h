// One element of omv_selftest_math (device, selftest_math.hip) and of oracle_math_map (host, oracle/math_host.cpp):
// the same text on both sides, so that a bit difference between the two is a difference of compilers and flags and
// never one of the test's own code.  `fn` is an OMV_MATH_* code of include/omv.h; the caller has validated it.
#pragma once
#include "omv_math.h"
#if defined(__HIPCC__)
#include "omv_device.h"
#endif

namespace omv {

// element sizes (bytes per element of a / b / c / out; 0: not read).  b of the camera codes is one k[8], b of
// PREDICT_SCALE one float, of PREDICT_SCALE_CLAMPED two and of the grid codes the four grid floats, shared by every
// element.
struct MathShape {
    int a, b, c, out;
    bool b_shared;
};
inline bool math_shape(int fn, MathShape *s) {
    switch (fn) {
        case OMV_MATH_SINCOSF: *s = {4, 0, 0, 8, false}; return true;
        case OMV_MATH_ATANF:
        case OMV_MATH_TANF:
        case OMV_MATH_SQRTF:
        case OMV_MATH_ROUND_EVEN: *s = {4, 0, 0, 4, false}; return true;
        case OMV_MATH_ATAN2F:
        case OMV_MATH_FAST_ATAN2_DEG:
        case OMV_MATH_DIVF: *s = {4, 4, 0, 4, false}; return true;
        case OMV_MATH_MULADD_F32: *s = {4, 4, 4, 4, false}; return true;
        case OMV_MATH_MULADD_F64: *s = {8, 8, 8, 8, false}; return true;
        case OMV_MATH_RCP_NR: *s = {8, 0, 0, 8, false}; return true;
        case OMV_MATH_KB8_PROJECT:
        case OMV_MATH_PINHOLE_PROJECT: *s = {12, 32, 0, 8, true}; return true;
        case OMV_MATH_KB8_UNPROJECT:
        case OMV_MATH_PINHOLE_UNPROJECT: *s = {8, 32, 0, 12, true}; return true;
        case OMV_MATH_PREDICT_SCALE: *s = {4, 4, 0, 4, true}; return true;
        case OMV_MATH_PREDICT_SCALE_CLAMPED: *s = {4, 8, 0, 4, true}; return true;
        case OMV_MATH_ROT_BIN: *s = {4, 4, 0, 4, false}; return true;
        case OMV_MATH_THREE_MAXIMA: *s = {4 * kRotHistLen, 0, 0, 12, false}; return true;
        case OMV_MATH_GRID_CELL_OF: *s = {8, 16, 0, 4, true}; return true;
        case OMV_MATH_GRID_WINDOW: *s = {12, 16, 0, 16, true}; return true;
        case OMV_MATH_KP_IN_WINDOW: *s = {32, 0, 0, 4, false}; return true;
        default: return false;
    }
}

OMV_MATH_FN void math_map_one(int fn, int64_t i, const void *a, const void *b, const void *c, void *out) {
    const float *af = (const float *)a, *bf = (const float *)b, *cf = (const float *)c;
    const double *ad = (const double *)a, *bd = (const double *)b, *cd = (const double *)c;
    float *of = (float *)out;
    double *od = (double *)out;
    const int32_t *ai = (const int32_t *)a;
    int32_t *oi = (int32_t *)out;
    switch (fn) {
        case OMV_MATH_SINCOSF: glibc_sincosf(af[i], of + 2 * i, of + 2 * i + 1); break;
        case OMV_MATH_ATANF: of[i] = glibc_atanf(af[i]); break;
        case OMV_MATH_ATAN2F: of[i] = glibc_atan2f(af[i], bf[i]); break;
        case OMV_MATH_TANF: of[i] = glibc_tanf(af[i]); break;
        case OMV_MATH_SQRTF: of[i] = sqrtf_cr(af[i]); break;
        case OMV_MATH_FAST_ATAN2_DEG: of[i] = fast_atan2_deg(af[i], bf[i]); break;
        case OMV_MATH_ROUND_EVEN: oi[i] = round_even(af[i]); break;
        case OMV_MATH_DIVF: of[i] = af[i] / bf[i]; break;
        case OMV_MATH_MULADD_F32: of[i] = af[i] * bf[i] + cf[i]; break;
        case OMV_MATH_MULADD_F64: od[i] = ad[i] * bd[i] + cd[i]; break;
#if defined(__HIPCC__)
        case OMV_MATH_RCP_NR: od[i] = rcp_nr(ad[i]); break;
#else
        case OMV_MATH_RCP_NR: od[i] = 1.0 / ad[i]; break;   // rcp_nr is the device's; the host gives the IEEE quotient
#endif
        case OMV_MATH_KB8_PROJECT: kb8_project_f(bf, af + 3 * i, of[2 * i], of[2 * i + 1]); break;
        case OMV_MATH_KB8_UNPROJECT: kb8_unproject_f(bf, af[2 * i], af[2 * i + 1], of + 3 * i); break;
        case OMV_MATH_PINHOLE_PROJECT: pinhole_project_f(bf, af + 3 * i, of[2 * i], of[2 * i + 1]); break;
        case OMV_MATH_PINHOLE_UNPROJECT: pinhole_unproject_f(bf, af[2 * i], af[2 * i + 1], of + 3 * i); break;
        case OMV_MATH_PREDICT_SCALE: oi[i] = predict_scale_raw(af[i], bf[0]); break;
        case OMV_MATH_PREDICT_SCALE_CLAMPED: oi[i] = predict_scale(af[i], bf[0], (int)bf[1]); break;
        case OMV_MATH_ROT_BIN: oi[i] = rot_bin(af[i], bf[i]); break;
        case OMV_MATH_THREE_MAXIMA: three_maxima(ai + kRotHistLen * i, oi + 3 * i); break;
        case OMV_MATH_GRID_CELL_OF: oi[i] = grid_cell_of(af[2 * i], af[2 * i + 1], bf[0], bf[1], bf[2], bf[3]); break;
        case OMV_MATH_GRID_WINDOW: {
            GridRange g;
            const bool hit = grid_window(af[3 * i], af[3 * i + 1], af[3 * i + 2], bf[0], bf[1], bf[2], bf[3], g);
            oi[4 * i] = hit ? g.x0 : -1, oi[4 * i + 1] = hit ? g.x1 : -1;
            oi[4 * i + 2] = hit ? g.y0 : -1, oi[4 * i + 3] = hit ? g.y1 : -1;
            break;
        }
        case OMV_MATH_KP_IN_WINDOW: {
            const float *e = af + 8 * i;
            oi[i] = kp_in_window(e[0], e[1], (int)e[2], e[3], e[4], e[5], (int)e[6], (int)e[7]);
            break;
        }
        default: break;
    }
}

}  // namespace omv
