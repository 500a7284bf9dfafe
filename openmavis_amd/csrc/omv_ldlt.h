// The block LDL^T solver of the reduced systems (16x16 f64 MFMA tiles, level-scheduled on a host-planned pattern:
// lba_plan.h's plan_schedule / plan_lds), its block pattern and the device LM control block that gates it.  One text for
// the translation units that solve with it: lba.hip (LocalInertialBA, the visual kind, FullInertialBA) and essgraph.hip
// (the pose graphs).  Internal linkage: every translation unit has its own instantiations.
#pragma once
#include <hip/hip_runtime.h>

#include "omv_blk16.h"
#include "omv_device.h"
#include "omv_lm.h"
#include "omv_math.h"

namespace {

// Device-resident Levenberg-Marquardt control (the rules: omv_lm.h), for the
// single-rank path: the accept / reject decision, the lambda schedule and the iteration / stop logic run in
// finish_trial_kernel, so one LM trial is a fixed kernel sequence (captured once as a hipGraph) whose kernels
// read lambda and their gate from here, and the host reads the outcome back once per optimize().
struct LmCtl {
    omv_lm::LmState lm;
    double errors_chi, err0, lambda_init, rho;
    int it, trials, its, opt_it, max_trials;
    int done;                // the optimisation has ended
    int errors_of_current;   // the last computed errors belong to the current state (A)
    int need_build;          // the next step starts a new iteration (buildSystem)
    int accepted;            // the last trial was accepted: the trial state becomes current
    int n_acc;               // accepted updates since optimize()'s start: ImuCamPose::its of every optimisable
                             // keyframe (created with its 0, popped with a rejected trial), Rwb normalised after every
                             // third Update (G2oTypes.cc:220-225) -- a trial normalises iff n_acc % 3 == 2
    // double-buffered state and errors (device driver): buffer `cur` holds the current state and its errors, the
    // trial writes buffer cur ^ 1 and an accepted trial flips `cur` -- no copy, and no recomputation of the
    // current errors after a rejected trial (they are still in their buffer); `last` = the buffer of the last
    // computed errors (the reference reports those: g2o keeps a rejected trial's errors after the pop)
    int cur, last;
    int init_pending;        // optimize()'s initial chi not summed yet (the first step's bookkeeping does it)
    double cur_chi;          // activeRobustChi2 of the current state
    int g_active, g_errA, g_build;   // gates of the next step (set by ctl_init / finish_trial)
};
enum { kGateAlways = 0, kGateErrA = 1, kGateBuild = 2, kGateTrial = 3 };
__device__ __forceinline__ bool gate_open(const LmCtl *c, int g) {
    if (!c || g == kGateAlways) return true;
    if (g == kGateErrA) return c->g_errA != 0;
    if (g == kGateBuild) return c->g_build != 0;
    return c->g_active != 0;
}

typedef double v4d __attribute__((ext_vector_type(4)));

// ---- trial: the reduced system, assembled per block -------------------------------------------------------
// The reduced system is stored as 16x16 blocks (keyframe block = pose 6 | v 3 | bg 3 | ba 3 | pad 1,
// padded to one f64 MFMA tile) on the symbolic LDL^T pattern (fill-in included) of the elimination order
// `perm` (position -> keyframe, host-chosen, see plan_order): slot(pi, pj) for block row pi >= block column
// pj, row-major 16x16 each, holding H's block (perm[pi], perm[pj]).  Padding rows have zero gradient and
// lambda on the diagonal, so they solve to exactly zero and add nothing to computeScale.  b and the Schur
// right-hand side stay in keyframe order (16 k + r).
// Entry (r, c) of a block: sw16(r, c), omv_blk16.h.

struct BlockPat {
    int nb, n_slots, n_lev;
    int n_lds;                       // hybrid solver (G = 2): slots 0 .. n_lds-1 in LDS, the rest in global scratch
    const int *perm;                 // [nb] position -> keyframe
    const int *slot_kr, *slot_kc;    // [n_slots] keyframes of the block's row / column
    const int *dslot;                // [nb] diagonal slot per position
    const int *lev_start, *lev_col;  // elimination-tree levels: the positions of level l
    const int *ug_start;             // [n_lev+1] update groups of a level (one target block each)
    const int *ug_split;             // [n_lev] groups ug_start[l] .. ug_split[l]: the diagonal blocks of level l + 1
    const int *crit_grp;             // [nb] per position: the group updating its diagonal from the level below, or -1
    const int *ug_task_start;        // [n_groups+1]
    const int4 *ug;                  //   (slot(i, j), slot(i, k), slot(j, k), dslot(k)), ascending k
    const int4 *inv_rec;             // [2 nb] per lev_col entry: (dslot, crit group's first / end update, -), its first
                                     // update (the inverse task in two reads instead of five dependent ones)
    const int *rs_start;             // [nb+1] row structure of position i: (slot(i, k), k), k < i
    const int2 *rs;
    const int *cs_start;             // [nb+1] column structure of position k: (slot(i, k), i), i > k
    const int2 *cs;
    // every array above but slot_kr / slot_kc lives in one contiguous device blob; when blob_ints > 0 the solver stages
    // it into LDS after the blocks, so the per-level schedule reads on its critical path are LDS reads, not dependent
    // global loads
    const int *blob;
    int blob_ints;
};

// ---- trial: block LDL^T of the reduced system (one workgroup, 16x16 f64 MFMA tiles) -------------

// Wave-synchronous step: LDS operations of one wavefront complete in order, so the fence only has
// to stop the compiler (wavefront scope); the global-memory fallback needs workgroup scope.
template <int G>
__device__ __forceinline__ void wave_sync() {
    if (G) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// The reduced system is factored as a block LDL^T with 16x16 block pivots: A = L D L^T, L_ik = S_ik D_k^-1, D_k = S_kk
// (each S the block as it stands when column k is eliminated).  Nothing but the blocks themselves and D_k^-1 is kept:
// the diagonal slot of column k is overwritten by D_k^-1, the panels S_ik stay unscaled in place, and
//   trailing update   S_ij -= S_ik D_k^-1 S_jk^T             (two f64 MFMA products, the inner one in registers)
//   forward           z_k = D_k^-1 (y_k - sum_{j < k} S_kj z_j)
//   backward          x_k = z_k - D_k^-1 sum_{i > k} S_ik^T x_i
// so a level is one diagonal-inverse phase and one phase of updates + forward columns.  The solution is that of the
// damped system (SimplicialLDLT's scalar LDL^T on its own AMD order, linear_solver_eigen.h:94-120, differs only in
// rounding).

// One wavefront: D (16x16 symmetric, lower triangle read) -> D^-1 in place (full), by sixteen 1x1 sweeps held in
// registers (the sweep operator): with pivot p = M_kk, r = 1 / p,
//   i, j != k : M_ij - M_ik (M_kj r)      row k : M_kj r      column k : M_ik r      M_kk : -r
// after all sixteen M = -D^-1 (no pivoting: D is the damped, positive definite Hessian block).  Lane l owns column
// j = l & 15, rows q + 4t (q = l >> 4).  Per pass the pivot is a uniform read (v_readlane), the row M_k. a cross-row
// ds_bpermute issued ahead of the reciprocal, and the column M_.k a DPP row broadcast of lane k of each 16-lane row --
// no LDS store / load round trip between passes (a v_permlane16/32_swap row broadcast measured slower: more
// instructions on an issue-bound pass; so did 2x2 pivot blocks, 4,200 vs 3,760 cycles).  A zero / non-finite
// pivot flags the solve (through the non-finite entries it leaves).
__device__ __forceinline__ double readlane_f64(double x, int l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)b, l), hi = __builtin_amdgcn_readlane((uint32_t)(b >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
template <int K>
__device__ __forceinline__ double row_bcast_f64(double x) {   // lane K of each 16-lane row, to the whole row
    const long long b = __builtin_bit_cast(long long, x);
    const long long r = __builtin_amdgcn_update_dpp(b, b, 0x150 + K, 0xf, 0xf, false);   // all lanes written
    return __builtin_bit_cast(double, r);
}
template <int K>
__device__ __forceinline__ void sweep_pass(double cur[4], int q, int j) {
    constexpr int tk = K >> 2, qk = K & 3;
    const double p = readlane_f64(cur[tk], 16 * qk + K);
    const double mkj = __shfl(cur[tk], 16 * qk + j, 64);   // issued early: its latency hides behind the reciprocal
    const double r = omv::rcp_nr(p);
    const double f = mkj * r;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double mik = row_bcast_f64<K>(cur[t]);
        double v = j == K ? mik * r : __builtin_fma(-mik, f, cur[t]);
        if (t == tk) v = q == qk ? (j == K ? -r : f) : v;
        cur[t] = v;
    }
}
template <int K>
__device__ __forceinline__ void sweep_all(double cur[4], int q, int j) {
    if constexpr (K < 16) {
        sweep_pass<K>(cur, q, j);
        sweep_all<K + 1>(cur, q, j);
    }
}

template <int G>
__device__ __forceinline__ void inv16(double *D, int lane, int *bad) {
    const int q = lane >> 4, j = lane & 15;
    double cur[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = q + 4 * t;
        cur[t] = D[i >= j ? sw16(i, j) : sw16(j, i)];
    }
    sweep_all<0>(cur, q, j);
#pragma unroll
    for (int t = 0; t < 4; ++t) D[sw16(q + 4 * t, j)] = -cur[t];
    // a zero or non-finite pivot leaves an infinite or NaN entry (1 / 0 = inf spreads through its row and column):
    // one check of the result instead of one per pass
    const bool fin = isfinite(cur[0]) && isfinite(cur[1]) && isfinite(cur[2]) && isfinite(cur[3]);
    if (__ballot(!fin) && lane == 0) *bad = 1;
    wave_sync<G>();
}

// One wavefront: S_ij -= S_ik Dinv_k S_jk^T.  Q = Dinv_k S_jk^T by four 16x16x4 f64 MFMAs leaves Q[kq + 4s][rc] in
// accumulator s of lane (rc, kq) -- exactly the B operand of step s of the second product -- so Q never leaves the
// registers.  A/B operand lane maps: A[l&15][4s + (l>>4)], B[4s + (l>>4)][l&15]; D: col l&15, row (l>>4) + 4i.
__device__ __forceinline__ void update16(double *Sij, const double *Sik, const double *Sjk, const double *Dinv, int lane) {
    const int rc = lane & 15, kq = lane >> 4;
    v4d Q = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int kk = 4 * s + kq;
        Q = __builtin_amdgcn_mfma_f64_16x16x4f64(Dinv[sw16(rc, kk)], Sjk[sw16(rc, kk)], Q, 0, 0, 0);
    }
    v4d acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = Sij[sw16(kq + 4 * i, rc)];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Sik[sw16(rc, 4 * s + kq)], Q[s], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) Sij[sw16(kq + 4 * i, rc)] = acc[i];
}

constexpr int kLdltThreads = 512;

// Forward substitution of one column (one wavefront): z_i = Dinv_i (y_i - sum_k S_ik z_k) over the row structure
// (descendants, final by then); lane group grp takes the terms m = 4 grp .. 4 grp + 3 of every block (four loads of
// S and four of z per lane and block, all lanes busy whatever the block count).
// Block s of the solver's storage: LDS, or (hybrid, s >= n_lds) global scratch.  A value type: a reference-capturing
// lambda here put the kernel's locals on the private stack (144 B of scratch per lane, ~9 us more per solve).
template <int G>
struct BlkAt {
    double *pk, *gs;
    int n_lds;
    __device__ __forceinline__ double *operator()(int s) const {
        return G == 2 && s >= n_lds ? gs + (size_t)s * 256 : pk + (size_t)s * 256;
    }
};

template <typename Blk>
__device__ __forceinline__ void forward_col(const Blk blk, double *y, const BlockPat &P, int i, int lane) {
    const int r16 = lane & 15, grp = lane >> 4;
    double acc[4] = {0, 0, 0, 0};   // four chains (the sum is latency-bound)
    for (int q = P.rs_start[i]; q < P.rs_start[i + 1]; ++q) {
        const int2 e = P.rs[q];
        const double *Sik = blk(e.x);
        const double *zk = y + 16 * e.y + 4 * grp;
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = __builtin_fma(Sik[sw16(r16, 4 * grp + m)], zk[m], acc[m]);
    }
    double a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    a += __shfl_xor(a, 16, 64);
    a += __shfl_xor(a, 32, 64);
    const double v = y[16 * i + r16] - a;
    // Dinv_i v: lane group grp takes columns 4 grp .. 4 grp + 3, then the four partial sums
    const double *Di = blk(P.dslot[i]);
    double out = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) out = __builtin_fma(Di[sw16(r16, 4 * grp + m)], __shfl(v, 4 * grp + m, 16), out);
    out += __shfl_xor(out, 16, 64);
    out += __shfl_xor(out, 32, 64);
    if (lane < 16) y[16 * i + lane] = out;
}

// Block LDL^T on the host-planned elimination order, level by level of its elimination tree: the columns of one level
// are independent (their trailing updates only reach ancestors, at higher levels), so a level's diagonal inverses run
// on separate wavefronts, then its trailing updates -- grouped by target block, each group on one wavefront in
// ascending column order (no two wavefronts write a block) -- beside its columns' forward substitutions.  Backward
// substitution gathers each column's structure (ancestors) level by level downwards.
// G: 0 blocks in LDS, 1 blocks in global scratch (pattern too large for LDS), 2 the first P.n_lds blocks in LDS and
// the rest in global scratch
template <int G>
__global__ void __launch_bounds__(kLdltThreads) ldlt_kernel(const double *Sp, BlockPat Pg, const double *b,
                                                            const double *coef, double *x, double *gscratch,
                                                            int *fail, const LmCtl *ctl) {
    extern __shared__ __attribute__((aligned(16))) double lsm[];
    __shared__ int bad;
    if (!gate_open(ctl, kGateTrial)) return;
    const int nb = Pg.nb, nv = 16 * nb;
    double *pk = G == 1 ? gscratch : lsm;
    const int n_lds = G == 2 ? Pg.n_lds : Pg.n_slots;
    double *y = pk + (size_t)n_lds * 256;
    double *xs = y + nv;
    const BlkAt<G> blk{pk, gscratch, n_lds};
    BlockPat P = Pg;   // the schedule, rebased onto its LDS copy when staged
    if (G != 1 && Pg.blob_ints > 0) {
        int *sched = reinterpret_cast<int *>(xs + nv);
        for (int q = threadIdx.x; q < Pg.blob_ints; q += blockDim.x) sched[q] = Pg.blob[q];
        auto rb = [&](auto *p) { return reinterpret_cast<decltype(p)>(sched + (reinterpret_cast<const int *>(p) - Pg.blob)); };
        P.perm = rb(Pg.perm), P.dslot = rb(Pg.dslot), P.lev_start = rb(Pg.lev_start), P.lev_col = rb(Pg.lev_col);
        P.ug_start = rb(Pg.ug_start), P.ug_split = rb(Pg.ug_split), P.crit_grp = rb(Pg.crit_grp);
        P.ug_task_start = rb(Pg.ug_task_start), P.ug = rb(Pg.ug), P.rs_start = rb(Pg.rs_start), P.rs = rb(Pg.rs);
        P.cs_start = rb(Pg.cs_start), P.cs = rb(Pg.cs), P.inv_rec = rb(Pg.inv_rec);
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (tid == 0) bad = 0;
#ifdef OMV_LDLT_PROFILE
    const long long t_0 = wall_clock64();
    long long t_1 = 0, t_3 = 0;
    __shared__ int pf_task[4];   // inverse ticks, forward ticks, inverse count, forward count
    __shared__ int pf_lev[16][4];   // per level: phase ticks, max inverse task ticks, inverses, other tasks (the
                                    // static LDS must stay under the 512 B beside kLdltLds, or the plan changes)
    if (tid < 4) pf_task[tid] = 0;
    if (tid < 64) pf_lev[tid >> 2][tid & 3] = 0;
#endif
    {
        const double2 *src = (const double2 *)Sp;
        double2 *dst = (double2 *)pk;
        // eight loads in flight per thread (a dependent load-store loop waits one memory latency per 8 KB)
        const int n2 = n_lds * 128, T = blockDim.x;
        for (int q0 = tid; q0 < n2; q0 += 8 * T) {
            double2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = src[min(q0 + k * T, n2 - 1)];   // unconditional: all eight in flight
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[min(q0 + k * T, n2 - 1)] = v[k];   // past the end: the last entry again
        }
        if (G == 2) {   // the global part, at its own offsets of the scratch
            double2 *gd = (double2 *)gscratch;
            for (int q = n2 + tid; q < P.n_slots * 128; q += T) gd[q] = src[q];
        }
        for (int q = tid; q < nv; q += blockDim.x) {
            const int g = 16 * Pg.perm[q >> 4] + (q & 15);   // (the LDS copy is not complete before the barrier)
            y[q] = b[g] - coef[g];
        }
    }
    __syncthreads();
#ifdef OMV_LDLT_PROFILE
    long long pf_fac = 0, pf_upd = 0, tp = wall_clock64();
#define OMV_LDLT_TICK(acc)                       \
    {                                            \
        const long long tn = wall_clock64();     \
        acc += tn - tp;                          \
        tp = tn;                                 \
    }
#else
#define OMV_LDLT_TICK(acc)
#endif
    // One phase per level l: level l's diagonal inverses -- each preceded, on its wavefront, by the updates of its
    // diagonal block from level l - 1 (the only trailing updates an inverse of level l waits for) -- beside level
    // l - 1's forward columns (their inverses and all their descendants' z are final) and level l - 1's other trailing
    // updates (no block of these is touched by an inverse of level l), so the bulk of each level's updates runs beside
    // the next level's inverses.  Each target block's updates come in ascending column order on one wavefront.
    // Wavefronts 0 .. ni-1 start on the inverses; with fewer than four inverses the wavefronts sharing their SIMDs
    // (w + 4) stay idle so the inverses -- the critical path -- issue alone; every other wavefront (and an inverse
    // wavefront once done) claims tasks from an LDS counter.  A phase advances the counter by its claimed tasks plus
    // one final failed claim per participating wavefront, so phase bases need no reset.
    __shared__ int claim;
    if (tid == 0) claim = 0;
    __syncthreads();
    int base = 0;
    for (int lev = 0; lev <= P.n_lev; ++lev) {
        const int c0 = P.lev_start[min(lev, P.n_lev)], c1 = lev < P.n_lev ? P.lev_start[lev + 1] : c0;
        const int f0 = lev > 0 ? P.lev_start[lev - 1] : 0, f1 = lev > 0 ? P.lev_start[lev] : 0;
        const int r0 = lev > 0 ? P.ug_split[lev - 1] : 0, r1 = lev > 0 ? P.ug_start[lev] : 0;
        const int ni = c1 - c0, nf = f1 - f0, na = ni + nf + (r1 - r0);
        const int ns = min(ni, nw);   // statically placed inverses
        const int n_idle = ni < 4 ? max(0, min(ni, nw - 4)) : 0;
        const bool idle = ni < 4 && wave >= 4 && wave - 4 < ni;
        if (!idle) {
            int q = wave < ns ? wave : -1;
            for (;;) {
                if (q < 0) {
                    int qn = 0;
                    if (lane == 0) qn = atomicAdd(&claim, 1);
                    q = ns + __shfl(qn, 0, 64) - base;
                    if (q >= na) break;
                }
#ifdef OMV_LDLT_PROFILE
                const long long tq = wall_clock64();
#endif
                if (q < ni) {
                    const int4 ir = P.inv_rec[2 * (c0 + q)], t0 = P.inv_rec[2 * (c0 + q) + 1];
                    if (ir.y < ir.z) {
                        for (int u = ir.y; u < ir.z; ++u) {
                            const int4 t = u == ir.y ? t0 : P.ug[u];
                            update16(blk(t.x), blk(t.y), blk(t.z), blk(t.w), lane);
                        }
                        wave_sync<G>();
                    }
                    inv16<G>(blk(ir.x), lane, &bad);
                } else if (q < ni + nf) {
                    forward_col(blk, y, P, P.lev_col[f0 + q - ni], lane);
                } else {
                    const int g = r0 + q - ni - nf;
                    for (int u = P.ug_task_start[g]; u < P.ug_task_start[g + 1]; ++u) {
                        const int4 t = P.ug[u];
                        update16(blk(t.x), blk(t.y), blk(t.z), blk(t.w), lane);
                    }
                }
#ifdef OMV_LDLT_PROFILE
                if (lane == 0 && q < ni + nf) atomicAdd(q < ni ? &pf_task[0] : &pf_task[1], (int)(wall_clock64() - tq));
                if (lane == 0 && q < ni + nf) atomicAdd(q < ni ? &pf_task[2] : &pf_task[3], 1);
                if (lane == 0 && lev < 16 && q < ni) atomicMax(&pf_lev[lev][1], (int)(wall_clock64() - tq));
#endif
                q = -1;
            }
        }
        base += (na - ns) + (nw - n_idle);
        __syncthreads();
#ifdef OMV_LDLT_PROFILE
        if (tid == 0 && lev < 16) pf_lev[lev][0] = (int)(wall_clock64() - tp), pf_lev[lev][2] = ni, pf_lev[lev][3] = na - ni;
#endif
        OMV_LDLT_TICK(pf_fac)
    }
#undef OMV_LDLT_TICK
#ifdef OMV_LDLT_PROFILE
    t_1 = wall_clock64();
#endif
    const int r16 = lane & 15, grp = lane >> 4;
    // backward: x_k = z_k - Dinv_k sum_i S_ik^T x_i
    for (int lev = P.n_lev - 1; lev >= 0; --lev) {
        for (int c = P.lev_start[lev] + wave; c < P.lev_start[lev + 1]; c += nw) {
            const int k = P.lev_col[c];
            double acc4[4] = {0, 0, 0, 0};   // lane group grp: rows 4 grp .. 4 grp + 3 of every block
            for (int q = P.cs_start[k]; q < P.cs_start[k + 1]; ++q) {
                const int2 e = P.cs[q];
                const double *Sik = blk(e.x);
                const double *xi = xs + 16 * e.y + 4 * grp;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc4[r] = __builtin_fma(Sik[sw16(4 * grp + r, r16)], xi[r], acc4[r]);
            }
            double acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
            acc += __shfl_xor(acc, 16, 64);
            acc += __shfl_xor(acc, 32, 64);
            const double *Dk = blk(P.dslot[k]);
            double out = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m) out = __builtin_fma(Dk[sw16(r16, 4 * grp + m)], __shfl(acc, 4 * grp + m, 16), out);
            out += __shfl_xor(out, 16, 64);
            out += __shfl_xor(out, 32, 64);
            if (lane < 16) xs[16 * k + lane] = y[16 * k + r16] - out;
        }
        __syncthreads();
    }
#ifdef OMV_LDLT_PROFILE
    t_3 = wall_clock64();
    if (tid == 0)
        printf("ldlt ticks(100MHz): factor+fwd %lld (diag inverse+fwd %lld updates %lld) bwd %lld slots %d levels %d; "
               "per inverse %.1f per forward col %.1f\n",
               t_1 - t_0, pf_fac, pf_upd, t_3 - t_1, P.n_slots, P.n_lev, (double)pf_task[0] / max(pf_task[2], 1),
               (double)pf_task[1] / max(pf_task[3], 1));
    if (tid == 0)
        for (int l = 0; l <= min(P.n_lev, 15); ++l)
            printf("  level %d: phase %d max-inverse %d inverses %d other %d\n", l, pf_lev[l][0], pf_lev[l][1],
                   pf_lev[l][2], pf_lev[l][3]);
#endif
    for (int q = tid; q < nv; q += blockDim.x) x[16 * P.perm[q >> 4] + (q & 15)] = xs[q];
    if (tid == 0) *fail = bad;
}

}  // namespace
