// Device-side helpers for the gfx950 kernels.  The pure float arithmetic (rounding, fastAtan2, the glibc sincosf /
// atanf / atan2f / tanf restatements, sqrtf_cr) lives in omv_math.h, which the host compiles too; what needs the
// device (LDS, builtins of the target, block indices) stays here.  Every float path must be compiled with
// -ffp-contract=off: the reference's float expressions are evaluated without fused multiply-adds, and bit-exact
// keypoints/descriptors depend on reproducing their rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "omv_math.h"

namespace omv {


__device__ __forceinline__ int reflect101(int p, int n) {
    // single reflection suffices: callers stay within one image width of the border
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - 2 - p : p;
}

// Hamming distance of two 256-bit descriptors held as 4 x u64.
__device__ __forceinline__ int hamming256(const uint64_t *a, const uint64_t *b) {
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}
// A 32-byte descriptor (8-byte aligned) as 4 x u64.
__device__ __forceinline__ void load_desc(const uint8_t *p, uint64_t d[4]) {
    const uint64_t *q = reinterpret_cast<const uint64_t *>(p);
    d[0] = q[0], d[1] = q[1], d[2] = q[2], d[3] = q[3];
}

// Wave-synchronous step over LDS: other lanes read what this wave just wrote.  A wavefront's LDS operations complete
// in order, so a wavefront-scope fence (it only has to stop the compiler) and no workgroup barrier: the other waves
// run their own rounds on their own slots.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The same step where the lanes exchange through global memory too: the LDS / global writes of this wave's lanes
// become visible to its other lanes.
__device__ __forceinline__ void wave_mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Butterfly reductions over the 64 lanes of a wavefront (every lane active): all lanes get the result.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Inclusive prefix sum over the 64 lanes of a wavefront (every lane active; `lane` is the caller's lane index): lane l
// gets v[0] + .. + v[l].
__device__ __forceinline__ int wave_incl_scan_i32(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// 1 / x by v_rcp_f64 and two Newton steps (within an ulp of the IEEE quotient on normal numbers; a zero / non-finite
// argument is the caller's to flag)
__device__ __forceinline__ double rcp_nr(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}


// XCD-aware block order: the dispatcher deals workgroup b to XCD b % 8, so consecutive logical blocks
// (neighbouring cells / keypoints / map points of one image or frame, which share bytes) are given to one XCD:
// physical b runs logical (b % 8) * ceil(n / 8) + b / 8 and those bytes are fetched into one L2, not eight.
// The grid is padded to a multiple of 8; returns -1 for a padding block.
__device__ __forceinline__ int xcd_block(int n_logical) {
    const int chunk = (n_logical + 7) >> 3;
    const int b = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    return b < n_logical ? b : -1;
}
__host__ inline int xcd_grid(int n_logical) { return (n_logical + 7) & ~7; }

}  // namespace omv
// v_mul_u32_u24 (full rate) for operands the caller knows are < 2^24: HIP's __umul24 masks its operands and the
// backend then emits v_and + v_mul_lo_u32 (quarter rate) unless it can prove the mask redundant.
extern "C" __device__ __attribute__((const)) uint32_t omv_llvm_mul_u24(uint32_t, uint32_t) __asm("llvm.amdgcn.mul.u24.i32");
extern "C" __device__ __attribute__((const)) uint32_t omv_llvm_mulhi_u24(uint32_t, uint32_t) __asm("llvm.amdgcn.mulhi.u24");
namespace omv {
__device__ __forceinline__ int mul_u24(int a, int b) { return (int)omv_llvm_mul_u24((uint32_t)a, (uint32_t)b); }
// v_mul_hi_u32_u24 (full rate): bits 32..47 of the product of two operands the caller knows are < 2^24.  With
// b < 2^16 and s < 2^16, mulhi_u24(b << 8, s << 8) == (b * s) >> 16 exactly: the product b s 2^16 is < 2^48, so
// nothing is lost above, and its low 16 bits are zero, so the shift by 32 drops the same bits as b s >> 16.
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b) { return omv_llvm_mulhi_u24(a, b); }

// Test knobs of a matcher handle (OMV_BOW_TOP, OMV_TRI_SLICES, OMV_TRI_ECAP, OMV_TRI_WALK, OMV_CAND, OMV_CAND_PW,
// OMV_CAND_SPLIT, OMV_KNN, OMV_KNN_IDX_LIMIT),
// read once by omv_matcher_create (not per call); -1 / 0: unset.  Defined in match.hip for the other matcher
// translation units.
struct MatcherKnobs {
    int bow_top = -1, tri_slices = -1, tri_ecap = -1, tri_walk_seq = 0;
    int cand_mode = 0;     // OMV_CAND: SearchByProjection candidates 0 by batch size, 1 "global" (no LDS staging), 2 "lds"
    int cand_pw = -1;      // OMV_CAND_PW: map points per wave of the LDS-staged candidate kernel
    int cand_split = -1;   // OMV_CAND_SPLIT: window entries per lane above which the staged kernel splits a window over
                           // more lanes (a huge value: one lane per window)
    int knn_mode = 0;      // OMV_KNN: knnMatch(k=2) kernel 0 by shape, 1 "mfma" (matrix cores), 2 "lanes"
    int knn_idx_limit = 1 << 16;   // OMV_KNN_IDX_LIMIT: train capacity from which the matrix-core knn is not used
};
MatcherKnobs matcher_knobs(const struct ::omv_matcher *m);
// omv_matcher_search_kf's entry capacity of a handle (max_frames x n_cams x max_mps)
size_t matcher_kf_entry_cap(const struct ::omv_matcher *m);

}  // namespace omv
