// =====================================================================================================
// TEST INFRASTRUCTURE ONLY — the product's Local BA plan on the host.  Never linked into the product.
//
// oracle_lba_plan: openmavis_amd/csrc/lba_plan.h itself (the text hipcc compiles into omv_lba_set_problem), built by
// the host compiler, with every array and scalar of the LbaPlan written out as a sequence of records
//     name[22] | kind 'i' / 'u' / 'f' | element bytes | int64 count | data, padded to 8 bytes
// (Int2 / Int4 records as 2 / 4 ints each; scalars and the shared limits kGrp* / kPanel / kLdltLds as one int64).
// Query, then fill: *need receives the bytes of the whole sequence, which is written only when it fits `cap`.
// Returns plan_lba's status.
// tests/test_lba_plan_cpu.py asserts the properties the kernels rely on.
// =====================================================================================================
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../openmavis_amd/csrc/lba_plan.h"

namespace {

using omv_lba_plan::Int2;
using omv_lba_plan::Int4;
using omv_lba_plan::LbaPlan;

struct Writer {
    uint8_t *buf;
    int64_t cap, at = 0;
    void raw(const char *name, char kind, int elem, int64_t count, const void *data) {
        const int64_t bytes = count * elem, padded = (bytes + 7) & ~(int64_t)7;
        if (at + 32 + padded <= cap) {
            uint8_t *r = buf + at;
            std::memset(r, 0, 32 + padded);
            std::strncpy((char *)r, name, 21);
            r[22] = (uint8_t)kind, r[23] = (uint8_t)elem;
            std::memcpy(r + 24, &count, 8);
            if (bytes) std::memcpy(r + 32, data, bytes);
        }
        at += 32 + padded;
    }
    template <class T>
    void vec(const char *name, const std::vector<T> &v) {
        if constexpr (std::is_same_v<T, Int2> || std::is_same_v<T, Int4>)
            raw(name, 'i', 4, (int64_t)(v.size() * sizeof(T) / 4), v.data());
        else
            raw(name, std::is_floating_point_v<T> ? 'f' : std::is_signed_v<T> ? 'i' : 'u', sizeof(T), (int64_t)v.size(),
                v.data());
    }
    void num(const char *name, int64_t v) { raw(name, 'i', 8, 1, &v); }
};

void write_plan(const LbaPlan &P, Writer &w) {
#define V(x) w.vec(#x, P.x)
#define N(x) w.num(#x, (int64_t)P.x)
    V(order), V(perm_edge), V(e_pt), V(e_kf), V(e_cam), V(e_slot), V(pt_edge), V(pt_slot), V(slot_kf), V(slot_edge);
    V(e_obs), V(e_w), V(e_ur), V(track_depth), V(offP), V(offV), V(offG), V(offA);
    V(perm), V(slot_kr), V(slot_kc), V(dslot), V(lev_start), V(lev_col), V(ug_start), V(ug_split), V(ug_task_start);
    V(crit_grp), V(ug), V(inv_rec), V(rs_start), V(rs), V(cs_start), V(cs), V(blob);
    V(grp_pt), V(grp_w), V(grp_tp), V(grp_blk), V(blkoff), V(grp_kf), V(rhsoff), V(lkf_kf), V(big_grp), V(blk_start);
    V(rhs_start), V(tp), V(slot_lkf), V(e_lkf), V(ib_start), V(iv_start), V(imu_blk), V(imu_vec);
    V(info9), V(infoG), V(infoA);
    N(n_pt_slots), N(n_red), N(n_slots), N(n_lev), N(n_lgrp), N(n_big), N(use_lds), N(n_lds), N(blob_ints), N(ldlt_lds);
    N(n_reduce);
    const LbaPlan::BlobOff &o = P.off;
    const std::vector<int64_t> off = {(int64_t)o.perm, (int64_t)o.dslot, (int64_t)o.lev_start, (int64_t)o.lev_col,
                                      (int64_t)o.ug_start, (int64_t)o.ug_split, (int64_t)o.crit_grp,
                                      (int64_t)o.ug_task_start, (int64_t)o.ug, (int64_t)o.rs_start, (int64_t)o.rs,
                                      (int64_t)o.cs_start, (int64_t)o.cs, (int64_t)o.inv_rec};
    w.vec("blob_off", off);
    // the limits the plan shares with the kernels: the tests' bounds
    using namespace omv_lba_plan;
    w.num("kGrpEdges", kGrpEdges), w.num("kGrpLand", kGrpLand), w.num("kGrpSlots", kGrpSlots), w.num("kGrpW", kGrpW);
    w.num("kPanel", kPanel), w.num("kLdltLds", (int64_t)kLdltLds);
#undef V
#undef N
}

}  // namespace

extern "C" {

int oracle_lba_plan(const omv_lba_problem *p, int rank, int world, int lds_ok, const int32_t *limits5, uint8_t *buf,
                    int64_t cap, int64_t *need) {
    const omv_lba_plan::LbaLimits lim{limits5[0], limits5[1], limits5[2], limits5[3], limits5[4]};
    LbaPlan plan;
    const omv_status rs = omv_lba_plan::plan_lba(*p, rank, world, lim, lds_ok != 0, plan);
    if (rs != OMV_OK) return rs;
    Writer w{buf, buf ? cap : 0};
    write_plan(plan, w);
    *need = w.at;
    return OMV_OK;
}

}  // extern "C"
