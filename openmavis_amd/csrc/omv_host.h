// Host-side helpers shared by the translation units that implement the C ABI of include/omv.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/omv.h"

// Evaluate a HIP runtime call inside a function that returns omv_status: on failure, report the call and HIP's
// message on stderr and return OMV_ERR_HIP.
#define HIP_OK(x)                                                                    \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "omv: %s failed: %s\n", #x, hipGetErrorString(e_));      \
            return OMV_ERR_HIP;                                                      \
        }                                                                            \
    } while (0)
