// The sorted insertion of the matchers' candidate lists (match.hip's TopPos), stated once: one text, compiled by hipcc
// for the device and by a plain C++ compiler for the host test (tests/cpp/topk_host.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OMV_TOPK_FN __host__ __device__ inline
#else
#define OMV_TOPK_FN inline
#endif

namespace omv {

OMV_TOPK_FN uint32_t topk_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
OMV_TOPK_FN uint32_t topk_max(uint32_t a, uint32_t b) { return a < b ? b : a; }
// The median of three in the min / max shape that the gfx9 back end folds into one v_med3_u32.
OMV_TOPK_FN uint32_t topk_med3(uint32_t a, uint32_t b, uint32_t c) {
    return topk_max(topk_min(a, b), topk_min(topk_max(a, b), c));
}

// key[0..K) ascending, ~0u in the empty slots behind the keys: insert k and keep the K smallest.
// Precondition: k != ~0u and k differs from every key in the list (strictly ordered unique keys, such as
// distance << 16 | position).  The new key[q] is the median of k and the old key[q - 1], key[q]: the old key[q - 1] where
// k sorts before it, k where it falls between the two, the old key[q] otherwise.  Every slot reads old values only
// (q descends, so key[q - 1] is still the old one): K independent instructions, no compare / select chain.
template <int K>
OMV_TOPK_FN void topk_insert(uint32_t *key, uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = K - 1; q > 0; --q) key[q] = topk_med3(k, key[q - 1], key[q]);
    key[0] = topk_min(k, key[0]);
}

}  // namespace omv
