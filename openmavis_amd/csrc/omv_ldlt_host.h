// The host side of the block LDL^T solver (omv_ldlt.h) on a planned pattern (lba_plan.h's LbaPlan), one text for
// lba.hip and essgraph.hip: the kernels' LDS opt-in, the pattern's upload, the scratch size, the launch, and the
// read-back of a solved system for the debug_solve hooks.  The first part needs no HIP runtime and compiles under the
// host compiler too (tests/cpp/ldlt_host.cpp, tests/test_ldlt_host_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>

#include "lba_plan.h"
#include "omv_blk16.h"

namespace omv_ldlt_host {

// What debug_solve reports of a solved system: the stored blocks (`blocks`: n_slots packed 16x16 blocks, block t between
// rows 16 slot_kr[t].. and columns 16 slot_kc[t]..) as the dense symmetric n x n matrix S, n = 16 nb -- a diagonal
// block's upper triangle is not read, as the solver does not read it -- and plan[] = mode, stored blocks, blocks in
// LDS, levels, then the columns of each level.  plan has room for 4 + n_lev entries.
inline void expand_solved(const double *blocks, const int *slot_kr, const int *slot_kc, const int *lev_start, int nb,
                          int n_slots, int n_lds, int n_lev, int use_lds, double *S, int32_t *plan) {
    const size_t n = 16 * (size_t)nb;
    std::fill(S, S + n * n, 0.0);
    for (int t = 0; t < n_slots; ++t) {
        const size_t kr = slot_kr[t], kc = slot_kc[t];
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c < (kr == kc ? r + 1 : 16); ++c) {
                const double v = blocks[(size_t)t * 256 + sw16(r, c)];
                S[(16 * kr + r) * n + 16 * kc + c] = v;
                S[(16 * kc + c) * n + 16 * kr + r] = v;
            }
    }
    plan[0] = use_lds, plan[1] = n_slots, plan[2] = n_lds, plan[3] = n_lev;
    for (int l = 0; l < n_lev; ++l) plan[4 + l] = lev_start[l + 1] - lev_start[l];
}

}  // namespace omv_ldlt_host

#ifdef __HIPCC__
#include <vector>

#include "omv_host.h"
#include "omv_ldlt.h"

namespace {

// The solver of one planned pattern: the device pattern and how to launch on it.  A value; the arrays are the arena's.
struct LdltSolver {
    BlockPat pat{};
    int use_lds = 0;       // LbaPlan::use_lds
    size_t lds_bytes = 0;  // dynamic LDS of a launch

    // The solver's kernels may take kLdltLds of dynamic LDS (a handle asks once, at its creation).
    static bool opt_in_lds() {
        const int lds = (int)omv_lba_plan::kLdltLds;
        const hipFuncAttribute attr = hipFuncAttributeMaxDynamicSharedMemorySize;
        const bool ok = hipFuncSetAttribute((const void *)ldlt_kernel<0>, attr, lds) == hipSuccess &&
                        hipFuncSetAttribute((const void *)ldlt_kernel<2>, attr, lds) == hipSuccess;
        (void)hipGetLastError();
        return ok;
    }
    // Doubles of global scratch a solve on plan `pl` needs.
    static size_t scratch_doubles(const omv_lba_plan::LbaPlan &pl) { return pl.use_lds == 1 ? 8 : pl.n_reduce + 8; }
    // slot_kr, slot_kc and the packed schedule of `pl` (LbaPlan::blob at LbaPlan::off) on the device, three allocations
    // in that order.  On a failure up.ok is false and the solver is empty.
    static LdltSolver upload(const omv_lba_plan::LbaPlan &pl, omv::Uploader &up) {
        const int *kr = up.copy(pl.slot_kr), *kc = up.copy(pl.slot_kc), *d = up.copy(pl.blob);
        if (!up.ok) return LdltSolver{};
        const omv_lba_plan::LbaPlan::BlobOff &o = pl.off;
        return LdltSolver{BlockPat{pl.nb, pl.n_slots, pl.n_lev, pl.n_lds, d + o.perm, kr, kc, d + o.dslot, d + o.lev_start,
                                   d + o.lev_col, d + o.ug_start, d + o.ug_split, d + o.crit_grp, d + o.ug_task_start,
                                   (const int4 *)(d + o.ug), (const int4 *)(d + o.inv_rec), d + o.rs_start,
                                   (const int2 *)(d + o.rs), d + o.cs_start, (const int2 *)(d + o.cs), d, pl.blob_ints},
                          pl.use_lds, pl.ldlt_lds};
    }
    // One solve of S x = b - coef on `stream`, gated by ctl (null: always); the caller checks hipGetLastError.
    void launch(hipStream_t stream, const double *S, const double *b, const double *coef, double *x, double *scratch,
                int *fail, const LmCtl *ctl) const {
        const int T = kLdltThreads;
        if (use_lds == 1) ldlt_kernel<0><<<1, T, lds_bytes, stream>>>(S, pat, b, coef, x, scratch, fail, ctl);
        else if (use_lds == 2) ldlt_kernel<2><<<1, T, lds_bytes, stream>>>(S, pat, b, coef, x, scratch, fail, ctl);
        else ldlt_kernel<1><<<1, T, 0, stream>>>(S, pat, b, coef, x, scratch, fail, ctl);
    }
    // debug_solve's read-back once the stream has finished a solve of plan `pl`: the packed blocks at d_S as the dense
    // S and plan[] (expand_solved), x and the fail flag.  The right-hand side is the caller's.
    omv_status read_solved(const omv_lba_plan::LbaPlan &pl, const double *d_S, const double *d_x, const int *d_fail,
                           double *S, double *x, int32_t *fail, int32_t *plan) const {
        std::vector<double> blocks((size_t)pat.n_slots * 256);
        HIP_OK(hipMemcpy(blocks.data(), d_S, blocks.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(x, d_x, 16 * (size_t)pat.nb * sizeof(double), hipMemcpyDeviceToHost));
        int f = 0;
        HIP_OK(hipMemcpy(&f, d_fail, sizeof(int), hipMemcpyDeviceToHost));
        *fail = f;
        omv_ldlt_host::expand_solved(blocks.data(), pl.slot_kr.data(), pl.slot_kc.data(), pl.lev_start.data(), pat.nb,
                                     pat.n_slots, pat.n_lds, pat.n_lev, use_lds, S, plan);
        return OMV_OK;
    }
};

}  // namespace
#endif
