// omv_selftest_math: the float layer under every bit-exact kernel (omv_math.h, rcp_nr, the plain float `/` and the
// a * b + c contraction probes), evaluated elementwise on plain device arrays with the product's build flags.  The host
// compiles the same omv_math_map.h into the oracle library; tests/test_math_device_gpu.py compares the two bit for bit.
#include <hip/hip_runtime.h>

#include "omv_host.h"
#include "omv_math_map.h"

namespace {

template <int FN>
__global__ void __launch_bounds__(256) selftest_math_kernel(int64_t n, const void *a, const void *b, const void *c,
                                                            void *out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) omv::math_map_one(FN, i, a, b, c, out);
}

template <int FN>
void launch(int grid, hipStream_t st, int64_t n, const void *a, const void *b, const void *c, void *out) {
    selftest_math_kernel<FN><<<grid, 256, 0, st>>>(n, a, b, c, out);
}

}  // namespace

extern "C" omv_status omv_selftest_math(int fn, int64_t n, const void *a, const void *b, const void *c, void *out,
                                        void *stream) {
    omv::MathShape s;
    if (!omv::math_shape(fn, &s) || n < 0) return OMV_ERR_ARG;
    if (n == 0) return OMV_OK;
    if (!a || !out || (s.b && !b) || (s.c && !c)) return OMV_ERR_ARG;
    const int64_t blocks = (n + 255) / 256;
    const int grid = (int)(blocks < 16384 ? blocks : 16384);
    hipStream_t st = (hipStream_t)stream;
    switch (fn) {
#define OMV_MATH_CASE(F) \
    case F: launch<F>(grid, st, n, a, b, c, out); break;
        OMV_MATH_CASE(OMV_MATH_SINCOSF)
        OMV_MATH_CASE(OMV_MATH_ATANF)
        OMV_MATH_CASE(OMV_MATH_ATAN2F)
        OMV_MATH_CASE(OMV_MATH_TANF)
        OMV_MATH_CASE(OMV_MATH_SQRTF)
        OMV_MATH_CASE(OMV_MATH_FAST_ATAN2_DEG)
        OMV_MATH_CASE(OMV_MATH_ROUND_EVEN)
        OMV_MATH_CASE(OMV_MATH_DIVF)
        OMV_MATH_CASE(OMV_MATH_MULADD_F32)
        OMV_MATH_CASE(OMV_MATH_MULADD_F64)
        OMV_MATH_CASE(OMV_MATH_RCP_NR)
        OMV_MATH_CASE(OMV_MATH_KB8_PROJECT)
        OMV_MATH_CASE(OMV_MATH_KB8_UNPROJECT)
        OMV_MATH_CASE(OMV_MATH_PINHOLE_PROJECT)
        OMV_MATH_CASE(OMV_MATH_PINHOLE_UNPROJECT)
        OMV_MATH_CASE(OMV_MATH_PREDICT_SCALE)
        OMV_MATH_CASE(OMV_MATH_PREDICT_SCALE_CLAMPED)
        OMV_MATH_CASE(OMV_MATH_ROT_BIN)
        OMV_MATH_CASE(OMV_MATH_THREE_MAXIMA)
        OMV_MATH_CASE(OMV_MATH_GRID_CELL_OF)
        OMV_MATH_CASE(OMV_MATH_GRID_WINDOW)
        OMV_MATH_CASE(OMV_MATH_KP_IN_WINDOW)
#undef OMV_MATH_CASE
        default: return OMV_ERR_ARG;
    }
    HIP_OK(hipGetLastError());
    return OMV_OK;
}
