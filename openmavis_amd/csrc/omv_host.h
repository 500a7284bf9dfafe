// Host-side helpers shared by the translation units that implement the C ABI of include/omv.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <memory>
#include <vector>

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

namespace omv {

// The state behind omv_debug_live_allocations / omv_debug_fail_allocation (omv_host.hip), one per process
inline std::atomic<int64_t> g_live_allocations{0};
inline std::atomic<int> g_fail_countdown{0};   // > 0: that many allocations from now, one fails
inline bool injected_allocation_failure() {
    return g_fail_countdown.load(std::memory_order_relaxed) > 0 && g_fail_countdown.fetch_sub(1) == 1;
}

// Owner of device, pinned-host and stream-ordered memory: every allocation of the library is made here, by a thin
// wrapper of hipMalloc / hipHostMalloc / hipMallocAsync, and freed when its arena goes out of scope.  A handle has one
// as a member beside its raw pointers.  A per-call workspace is an arena on the stack: the success path ends with a
// checked HIP_OK(ws.free(&p)) where the stream order wants the free, every early return frees through the destructor.
class DeviceArena {
public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { reset(); }
    // max(1, count) elements of T into *p; on failure *p is null and the reason is on stderr
    template <class T>
    bool alloc(T **p, size_t count) { return take(p, count, kDevice, nullptr); }
    template <class T>
    bool alloc_pinned(T **p, size_t count) { return take(p, count, kPinned, nullptr); }
    template <class T>
    bool alloc_async(T **p, size_t count, hipStream_t st) { return take(p, count, kStream, st); }
    // Free one allocation of this arena and null the pointer (a null pointer is fine).
    template <class T>
    hipError_t free(T **p) {
        hipError_t e = hipSuccess;
        for (size_t i = 0; *p && i < blocks_.size(); ++i)
            if (blocks_[i].p == (void *)*p) {
                e = release(blocks_[i]);
                blocks_.erase(blocks_.begin() + i);
                break;
            }
        *p = nullptr;
        return e;
    }
    // A buffer with a capacity field, replaced when a call needs more.  The old buffer goes first and the capacity is
    // set last: after a failure *p is null and *cap is 0.  grow_async: in stream order, and a failing free fails it.
    template <class T>
    bool grow(T **p, size_t *cap, size_t need) { return regrow(p, cap, need, kDevice, nullptr); }
    template <class T>
    bool grow_async(T **p, size_t *cap, size_t need, hipStream_t st) { return regrow(p, cap, need, kStream, st); }
    void reset() {   // in allocation order
        for (const Block &b : blocks_) (void)release(b);
        blocks_.clear();
    }

private:
    enum Kind { kDevice, kPinned, kStream };
    struct Block {
        void *p;
        Kind kind;
        hipStream_t st;
    };
    template <class T>
    bool take(T **p, size_t count, Kind k, hipStream_t st) {
        static const char *const call[] = {"hipMalloc", "hipHostMalloc", "hipMallocAsync"};
        const size_t bytes = std::max<size_t>(1, count) * sizeof(T);
        void *q = nullptr;
        *p = nullptr;
        blocks_.push_back(Block{nullptr, k, st});   // the slot first: no block is lost if the vector cannot grow
        const bool injected = injected_allocation_failure();
        const hipError_t e = injected       ? hipErrorOutOfMemory
                             : k == kDevice ? hipMalloc(&q, bytes)
                             : k == kPinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault)
                                            : hipMallocAsync(&q, bytes, st);
        if (e != hipSuccess) {
            fprintf(stderr, "omv: %s of %zu bytes failed: %s\n", call[k], bytes,
                    injected ? "injected by omv_debug_fail_allocation" : hipGetErrorString(e));
            if (!injected) (void)hipGetLastError();   // reported here: not again by a later launch check
            blocks_.pop_back();
            return false;
        }
        ++g_live_allocations;
        blocks_.back().p = q;
        *p = (T *)q;
        return true;
    }
    template <class T>
    bool regrow(T **p, size_t *cap, size_t need, Kind k, hipStream_t st) {
        const hipError_t e = free(p);
        *cap = 0;
        if ((k == kStream && e != hipSuccess) || !take(p, need, k, st)) return false;
        *cap = need;
        return true;
    }
    static hipError_t release(const Block &b) {
        --g_live_allocations;
        return b.kind == kDevice ? hipFree(b.p) : b.kind == kPinned ? hipHostFree(b.p) : hipFreeAsync(b.p, b.st);
    }
    std::vector<Block> blocks_;
};

// A problem's upload into an arena, one allocation per array.  The first allocation or copy that fails clears `ok`;
// every later call then allocates nothing and returns null, so the caller checks `ok` where it must and at the end.
struct Uploader {
    DeviceArena &mem;
    bool ok = true;
    template <class T>
    T *copy(const T *src, size_t n) {   // a device copy of n host elements
        T *d = nullptr;
        if (ok && (!mem.alloc(&d, n) || (n > 0 && hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)))
            ok = false, d = nullptr;
        return d;
    }
    template <class T>
    T *copy(const std::vector<T> &v) { return copy(v.data(), v.size()); }
    template <class T>
    void buffer(T **d, size_t n) { ok = ok && mem.alloc(d, n); }   // an uninitialised work buffer
};

}  // namespace omv
