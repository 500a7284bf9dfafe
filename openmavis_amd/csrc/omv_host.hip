// The two test hooks on omv_host.h's allocation owner (include/omv.h).
#include "omv_host.h"

extern "C" {

omv_status omv_debug_live_allocations(int64_t *n) {
    if (!n) return OMV_ERR_ARG;
    *n = omv::g_live_allocations.load();
    return OMV_OK;
}

omv_status omv_debug_fail_allocation(int nth) {
    if (nth < 0) return OMV_ERR_ARG;
    omv::g_fail_countdown.store(nth);
    return OMV_OK;
}

}  // extern "C"
