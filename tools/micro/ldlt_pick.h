// Pivot pick order of the pose kernels' LDL^T (the first phase of pose.hip's ldlt_pick_solve) as a function of its own,
// for the LDL^T microbenchmarks that replace the later phases.  Include after pose.hip.
#pragma once

namespace {

// Eigen's pick order of the N x N symmetric H into pick[] (one wavefront); false on a NaN diagonal.
template <int N>
__device__ __forceinline__ bool micro_pick_order(const double *H, int *pick, int lane) {
    static_assert(N <= 32, "rows on lanes 0..31");
    const bool in = lane < N;
    const double dv = in ? fabs(H[lane * (N + 1)]) : 0.0;
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double o = fabs(H[j * (N + 1)]);
        gt += o > dv ? 1 : 0;
        eq += o == dv ? 1 : 0;
    }
    if (__ballot(in && !(dv == dv))) return false;
    if (!__ballot(in && eq > 1)) {
        if (in) pick[gt] = lane;
    } else {
        int pos = lane;
        bool picked = false;
        for (int k = 0; k < N; ++k) {
            uint64_t cand = __ballot(in && !picked && gt <= k && k < gt + eq);
            int e = __builtin_ctzll(cand);
            if (cand & (cand - 1)) {
                int bp = __builtin_amdgcn_readlane(pos, e);
                for (uint64_t m = cand & (cand - 1); m; m &= m - 1) {
                    const int c = __builtin_ctzll(m), pc = __builtin_amdgcn_readlane(pos, c);
                    if (pc < bp) bp = pc, e = c;
                }
            }
            const int xk = __builtin_ctzll(__ballot(in && pos == k));
            const int pe = __builtin_amdgcn_readlane(pos, e);
            if (lane == xk) pos = pe;
            if (lane == e) pos = k, picked = true;
            if (lane == 0) pick[k] = e;
        }
    }
    return true;
}

}  // namespace
