// The 3x3 inverse by cofactors, shared by the device edges (g2o_types.h) and the host-only Local BA plan
// (lba_plan.h): one text, compiled by hipcc for both sides and by a plain C++ compiler for the host.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OMV_INV3_FN __host__ __device__ inline
#else
#define OMV_INV3_FN inline
#endif

namespace omv_g2o {

template <typename T>
OMV_INV3_FN bool inv3(const T *a, T *r) {
    T c[9];
    c[0] = a[4] * a[8] - a[5] * a[7];
    c[1] = a[2] * a[7] - a[1] * a[8];
    c[2] = a[1] * a[5] - a[2] * a[4];
    c[3] = a[5] * a[6] - a[3] * a[8];
    c[4] = a[0] * a[8] - a[2] * a[6];
    c[5] = a[2] * a[3] - a[0] * a[5];
    c[6] = a[3] * a[7] - a[4] * a[6];
    c[7] = a[1] * a[6] - a[0] * a[7];
    c[8] = a[0] * a[4] - a[1] * a[3];
    const T det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6];
    const T id = T(1) / det;
    for (int k = 0; k < 9; ++k) r[k] = c[k] * id;
    return det != T(0);
}

}  // namespace omv_g2o
