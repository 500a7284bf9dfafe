// MI355X-native KeyFrameDatabase: DetectNBestCandidates (src/KeyFrameDatabase.cc:581-713) and
// DetectRelocalizationCandidates (:715-828) for a batch of queries, behind the omv_kfdb handle of include/omv.h.
//
// Dense formulation: no inverted file.  The database is a table of BowVectors by slot ([max_kf][max_bow] ascending word
// ids + double values, a count, an `add` sequence number and an occupancy flag per slot).  The reference walks
// mvInvertedFile[word] for the query's words in ascending order and lists a keyframe the first time it meets it; every
// list is in `add` order and `erase` removes entries, so the position of a keyframe in lKFsSharingWords is the
// ascending order of (smallest word shared with the query, sequence number of its latest add), and
// mnPlaceRecognitionWords / mnRelocWords is the size of the intersection.
//   kfdb_share_kernel   one wavefront per (query, slot): lanes stride over the shorter list and binary-search the
//                       longer, four searches in flight per lane; per 64 elements a ballot gives the shared words in
//                       ascending order, and the terms
//                       fabs(vi - wi) - fabs(vi) - fabs(wi) are added in that order in double (L1Scoring::score,
//                       Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68: a sequential sum, never a tree), read lane by
//                       lane out of the registers: no LDS, no scratch row, no atomics.  Every sharing pair is scored
//                       here: the sum costs one add per shared word, and the pairs the selection later drops are by
//                       definition the ones that share the fewest.
//   kfdb_select_kernel  one workgroup for the call, the queries in order (the per-slot state makes query j depend on
//                       the queries before it): marks the listed keyframes, maxCommonWords / minCommonWords, puts the
//                       scored ones (words > minCommonWords) in list order by a bitonic sort of their unique (first
//                       word, sequence) keys, stores the scores, accumulates over the ten covisibility neighbours,
//                       sorts (accScore descending, list position ascending), stable by construction, and runs the
//                       reference's final walk.  The listed keyframes that are not scored need no order (only the
//                       test hook shows it: kfdb_list_sort_kernel).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/omv.h"
#include "omv_device.h"
#include "omv_host.h"

namespace {

constexpr int kNeigh = 10;           // GetBestCovisibilityKeyFrames(10)
constexpr int kSelThreads = 1024;
constexpr int kLdsSortMax = 8192;    // (key, value) pairs sorted in LDS (12 bytes each); beyond that in HBM scratch
constexpr int kModeNBest = 0, kModeReloc = 1;
constexpr int kUnroll = 4;          // share kernel: searches in flight per lane

struct Table {   // the database, device pointers
    int max_kf, max_bow;
    int32_t *word;       // [max_kf][max_bow] ascending
    double *value;       // [max_kf][max_bow]
    int32_t *n;          // [max_kf]
    uint32_t *seq;       // [max_kf] sequence number of the latest add
    uint8_t *occ;        // [max_kf] in the database
    int32_t *map;        // [max_kf] GetMap()
    int32_t *neigh;      // [max_kf][10] GetBestCovisibilityKeyFrames(10) as slots, -1 padded
    uint8_t *flags;      // [max_kf] bit 0 isBad(), bit 1 GetMap()->IsBad()
    int64_t *st_query[2];   // [max_kf] mnPlaceRecognitionQuery / mnRelocQuery
    float *st_score[2];     // [max_kf] mPlaceRecognitionScore / mRelocScore
};

__global__ void __launch_bounds__(256) kfdb_add_kernel(Table t, const int32_t *slot, const int32_t *map_id,
                                                       const int32_t *bow_word, const double *bow_value,
                                                       const int32_t *bow_n, int stride, uint32_t seq0) {
    const int i = blockIdx.x, s = slot[i];
    const int m = min(max(bow_n[i], 0), t.max_bow);   // the host has checked bow_n against max_bow
    const int32_t *w = bow_word + (size_t)i * stride;
    const double *v = bow_value + (size_t)i * stride;
    for (int q = threadIdx.x; q < m; q += blockDim.x) {
        t.word[(size_t)s * t.max_bow + q] = w[q];
        t.value[(size_t)s * t.max_bow + q] = v[q];
    }
    if (threadIdx.x < kNeigh) t.neigh[s * kNeigh + threadIdx.x] = -1;
    if (threadIdx.x == 0) {   // a fresh KeyFrame (src/KeyFrame.cc:24-37): query ids and scores 0
        t.n[s] = m, t.seq[s] = seq0 + (uint32_t)i, t.occ[s] = 1, t.map[s] = map_id[i], t.flags[s] = 0;
        t.st_query[0][s] = 0, t.st_query[1][s] = 0, t.st_score[0][s] = 0.f, t.st_score[1][s] = 0.f;
    }
}

// what 0 erase (occ = 0), 1 set_neighbours, 2 set_flags
__global__ void __launch_bounds__(256) kfdb_scatter_kernel(Table t, int what, int n, const int32_t *slot,
                                                           const int32_t *neigh, const uint8_t *flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i];
    if (what == 0) t.occ[s] = 0;
    if (what == 1)
        for (int k = 0; k < kNeigh; ++k) t.neigh[s * kNeigh + k] = neigh[i * kNeigh + k];
    if (what == 2) t.flags[s] = flags[i];
}

// clear (all != 0) / clearMap
__global__ void __launch_bounds__(256) kfdb_clear_kernel(Table t, int all, int map_id) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < t.max_kf && (all || t.map[s] == map_id)) t.occ[s] = 0;
}

__device__ __forceinline__ double lane_read(double x, int l) {   // x of lane l (wave-uniform l)
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ void __launch_bounds__(256) kfdb_share_kernel(Table t, int hi, const int32_t *q_word, const double *q_value,
                                                         const int32_t *q_n, int stride, int max_query_bow,
                                                         int32_t *words, int32_t *first, double *score) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), j = blockIdx.y;
    if (s >= hi) return;   // wave-uniform
    int nq = q_n[j];
    if (nq < 0 || nq > max_query_bow || nq > stride) nq = 0;   // flagged by the select kernel (count -1)
    const int ns = t.occ[s] ? t.n[s] : 0;
    // A: the shorter list (the lanes' elements), B: the longer (searched)
    const bool a_is_q = nq <= ns;
    const int32_t *qw = q_word + (size_t)j * stride, *sw = t.word + (size_t)s * t.max_bow;
    const double *qv = q_value + (size_t)j * stride, *sv = t.value + (size_t)s * t.max_bow;
    const int32_t *A = a_is_q ? qw : sw, *B = a_is_q ? sw : qw;
    const double *AV = a_is_q ? qv : sv, *BV = a_is_q ? sv : qv;
    const int na = a_is_q ? nq : ns, nb = a_is_q ? ns : nq;
    int cnt = 0, fw = -1;
    double sum = 0.0;
    int top = 1;   // the largest power of two <= nb
    while (2 * top <= nb) top <<= 1;
    // kUnroll x 64 elements of A per round: the searches are chains of dependent loads, and kUnroll of them in flight
    // per lane hide each other's latency.  A search has a fixed number of steps, so the kUnroll chains stay in step.
    for (int base = 0; base < na; base += 64 * kUnroll) {
        int w[kUnroll], pos[kUnroll];
        for (int u = 0; u < kUnroll; ++u) {
            const int i = base + 64 * u + lane;
            w[u] = i < na ? A[i] : 0x7fffffff;
            pos[u] = 0;   // -> the number of elements of B below w (lower_bound)
        }
        for (int step = top; step > 0; step >>= 1)
            for (int u = 0; u < kUnroll; ++u) {
                const int np = pos[u] + step;
                if (B[min(np, nb) - 1] < w[u] && np <= nb) pos[u] = np;
            }
        for (int u = 0; u < kUnroll; ++u) {
            const int i = base + 64 * u + lane;
            bool hit = false;
            double term = 0.0;
            if (i < na && pos[u] < nb && B[pos[u]] == w[u]) {
                hit = true;
                const double va = AV[i], vb = BV[pos[u]];
                const double vi = a_is_q ? va : vb, wi = a_is_q ? vb : va;   // score(query, keyframe)
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
            unsigned long long m = __ballot(hit);
            if (m) {
                if (fw < 0) fw = __builtin_amdgcn_readlane(w[u], (int)__builtin_ctzll(m));
                cnt += __popcll(m);
                while (m) {   // ascending lanes = ascending words: the reference's += order
                    sum += lane_read(term, (int)__builtin_ctzll(m));
                    m &= m - 1;
                }
            }
        }
    }
    if (lane == 0) {
        const size_t o = (size_t)j * t.max_kf + s;
        words[o] = cnt, first[o] = fw, score[o] = -sum / 2.0;
    }
}

struct SelArgs {
    Table t;
    int hi, n_q, mode, n_cand, max_query_bow, stride;
    const int64_t *qid;
    const int32_t *qmap, *cstart, *cslot, *q_n;
    const int32_t *words, *first;
    const double *score;
    int64_t *conn_stamp, *add_stamp;   // [max_kf]
    int64_t stamp0;
    uint64_t *gkey;   // [P] sort scratch in HBM (used when P > kLdsSortMax)
    int32_t *gval;
    int32_t *tmp_best;    // [max_kf]
    uint32_t *tmp_bits;   // [max_kf]
    uint8_t *cls;         // [max_kf]
    // per query, kept for omv_kfdb_debug
    int32_t *q_info;      // [max_q][4] maxCommonWords, minCommonWords, n_list, n_scored
    int32_t *list_slot, *sc_slot, *acc_best;   // [max_q][max_kf]
    float *sc_si;
    uint32_t *acc_bits;
    int32_t *out_a, *n_a, *out_b, *n_b;   // loop / merge (n_best) or candidates (reloc: out_a, n_a)
};

// Ascending bitonic sort of P (power of two) keys with their values, by the whole workgroup.
__device__ void bitonic_sort_kv(uint64_t *k, int32_t *v, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < P; i += blockDim.x) {
                const int p = i ^ stride;
                if (p > i) {
                    const uint64_t a = k[i], b = k[p];
                    const bool up = (i & size) == 0;
                    if ((a > b) == up) {
                        const int32_t va = v[i], vb = v[p];
                        k[i] = b, k[p] = a, v[i] = vb, v[p] = va;
                    }
                }
            }
            __syncthreads();
        }
}

// float -> uint32 whose unsigned order is the float order (-0 and +0 equal, as `>` sees them)
__device__ __forceinline__ uint32_t float_order(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__global__ void __launch_bounds__(kSelThreads) kfdb_select_kernel(SelArgs a) {
    extern __shared__ uint64_t lds_sort[];
    __shared__ int s_n, s_maxw, s_total, s_bestbits, s_chunk[64], s_cnt[2];
    const Table &t = a.t;
    const int tid = threadIdx.x, T = blockDim.x, mk = t.max_kf;
    int P_cap = 1;
    while (P_cap < a.hi) P_cap <<= 1;
    uint64_t *key = P_cap <= kLdsSortMax ? lds_sort : a.gkey;
    int32_t *val = P_cap <= kLdsSortMax ? (int32_t *)(lds_sort + P_cap) : a.gval;
    int64_t *stq = t.st_query[a.mode];
    float *sts = t.st_score[a.mode];
    const int out_w = a.mode == kModeNBest ? a.n_cand : mk;

    for (int j = 0; j < a.n_q; ++j) {
        const int64_t qid = a.qid[j], stamp = a.stamp0 + j;
        const int qmap = a.qmap[j];
        const size_t row = (size_t)j * mk;
        const int32_t *words = a.words + row, *first = a.first + row;
        const double *score = a.score + row;
        int32_t *list_slot = a.list_slot + row, *sc_slot = a.sc_slot + row, *acc_best = a.acc_best + row;
        uint32_t *acc_bits = a.acc_bits + row;
        float *sc_si = a.sc_si + row;
        int32_t *out_a = a.out_a + (size_t)j * out_w, *out_b = a.out_b ? a.out_b + (size_t)j * out_w : nullptr;
        const int qn = a.q_n[j];
        const bool bad_query = qn < 0 || qn > a.max_query_bow || qn > a.stride;

        if (tid == 0) s_n = 0, s_maxw = 0, s_total = 0, s_bestbits = 0, s_cnt[0] = 0, s_cnt[1] = 0;
        for (int i = tid; i < out_w; i += T) {
            out_a[i] = -1;
            if (out_b) out_b[i] = -1;
        }
        if (a.mode == kModeNBest)   // spConnectedKF
            for (int i = a.cstart[j] + tid; i < a.cstart[j + 1]; i += T) a.conn_stamp[a.cslot[i]] = stamp;
        __syncthreads();
        // lKFsSharingWords: shares a word, not connected, not yet marked with this query's id; marking stores the id.
        // Kept unordered here: only the scored subset below needs the list's order.
        for (int s = tid; s < a.hi; s += T) {
            if (!t.occ[s] || words[s] <= 0) continue;
            if (a.mode == kModeNBest && a.conn_stamp[s] == stamp) continue;
            if (stq[s] == qid) continue;
            stq[s] = qid;
            list_slot[atomicAdd(&s_n, 1)] = s;
            atomicMax(&s_maxw, words[s]);
        }
        __syncthreads();
        const int n_list = s_n, maxw = s_maxw;
        const int minw = (int)((float)maxw * (a.mode == kModeNBest ? 0.2f : 0.8f));
        // lScoreAndMatch: the listed keyframes with more than minCommonWords words, in list order = ascending
        // (first shared word, add sequence)
        for (int i = tid; i < n_list; i += T) {
            const int s = list_slot[i];
            if (words[s] > minw) {
                const int pos = atomicAdd(&s_total, 1);
                key[pos] = ((uint64_t)(uint32_t)first[s] << 32) | t.seq[s];
                val[pos] = s;
            }
        }
        __syncthreads();
        const int n_sc = s_total;
        if (n_sc > 0) {
            int P = 1;
            while (P < n_sc) P <<= 1;
            for (int i = n_sc + tid; i < P; i += T) key[i] = ~0ull, val[i] = -1;
            __syncthreads();
            bitonic_sort_kv(key, val, P);
            for (int i = tid; i < n_sc; i += T) {
                const int s = val[i];
                const float si = (float)score[s];
                sts[s] = si, sc_slot[i] = s, sc_si[i] = si;
            }
            __syncthreads();
        }
        if (n_sc > 0) {
            // lAccScoreAndMatch: the stored scores of the neighbours that carry this query's id
            const bool sorted = a.mode == kModeNBest;
            for (int i = tid; i < n_sc; i += T) {
                const int s = sc_slot[i];
                float best = sc_si[i], acc = best;
                int best_kf = s;
                for (int k = 0; k < kNeigh; ++k) {
                    const int nb = t.neigh[s * kNeigh + k];
                    if (nb < 0 || stq[nb] != qid) continue;
                    const float sc = sts[nb];
                    acc += sc;
                    if (sc > best) best_kf = nb, best = sc;
                }
                const uint32_t bits = __float_as_uint(acc);
                if (sorted) {
                    a.tmp_bits[i] = bits, a.tmp_best[i] = best_kf;
                    key[i] = ((uint64_t)(~float_order(bits)) << 32) | (uint32_t)i;
                    val[i] = i;
                } else {
                    acc_bits[i] = bits, acc_best[i] = best_kf;
                    if (acc > 0.f) atomicMax(&s_bestbits, (int)bits);   // bestAccScore: positive floats order as ints
                }
            }
            if (sorted) {
                int P = 1;
                while (P < n_sc) P <<= 1;
                for (int i = n_sc + tid; i < P; i += T) key[i] = ~0ull, val[i] = -1;
                __syncthreads();
                bitonic_sort_kv(key, val, P);   // lAccScoreAndMatch.sort(compFirst): stable, descending
                for (int i = tid; i < n_sc; i += T) acc_bits[i] = a.tmp_bits[val[i]], acc_best[i] = a.tmp_best[val[i]];
            }
            __syncthreads();
            // the class of every entry for the final walk
            const float thr = 0.75f * __int_as_float(s_bestbits);
            for (int i = tid; i < n_sc; i += T) {
                const int b = acc_best[i];
                uint8_t c;
                if (sorted) {
                    const uint8_t f = t.flags[b];
                    c = (f & 1) ? 0 : (t.map[b] == qmap ? 1 : ((f & 2) ? 0 : 2));
                } else {
                    c = (__uint_as_float(acc_bits[i]) > thr && t.map[b] == qmap) ? 1 : 0;
                }
                a.cls[i] = c;
            }
            __syncthreads();
            if (tid < 64) {   // the walk: 64 entries at a time, lane 0 takes the flagged ones in order
                int n0 = 0, n1 = 0;
                for (int base = 0; base < n_sc; base += 64) {
                    const int i = base + tid;
                    const int c = i < n_sc ? a.cls[i] : 0;
                    s_chunk[tid] = i < n_sc ? acc_best[i] : -1;
                    const unsigned long long m1 = __ballot(c == 1), m2 = __ballot(c == 2);
                    omv::wave_lds_sync();
                    if (tid == 0) {
                        if (sorted) {
                            for (unsigned long long m = m1; m && n0 < a.n_cand; m &= m - 1) {
                                const int b = s_chunk[__builtin_ctzll(m)];
                                bool dup = false;   // spAlreadyAddedKF: see DESIGN.md on why the pushed ones suffice
                                for (int k = 0; k < n0; ++k) dup |= out_a[k] == b;
                                if (!dup) out_a[n0++] = b;
                            }
                            for (unsigned long long m = m2; m && n1 < a.n_cand; m &= m - 1) {
                                const int b = s_chunk[__builtin_ctzll(m)];
                                bool dup = false;
                                for (int k = 0; k < n1; ++k) dup |= out_b[k] == b;
                                if (!dup) out_b[n1++] = b;
                            }
                        } else {
                            for (unsigned long long m = m1; m; m &= m - 1) {
                                const int b = s_chunk[__builtin_ctzll(m)];
                                if (a.add_stamp[b] != stamp) a.add_stamp[b] = stamp, out_a[n0++] = b;
                            }
                        }
                        s_cnt[0] = n0, s_cnt[1] = n1;
                    }
                    omv::wave_lds_sync();
                    n0 = s_cnt[0], n1 = s_cnt[1];
                    if (sorted && n0 >= a.n_cand && n1 >= a.n_cand) break;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            a.n_a[j] = bad_query ? -1 : s_cnt[0];
            if (a.n_b) a.n_b[j] = bad_query ? -1 : s_cnt[1];
            int32_t *qi = a.q_info + 4 * j;
            qi[0] = n_list > 0 ? maxw : 0, qi[1] = n_list > 0 ? minw : 0, qi[2] = n_list, qi[3] = n_sc;
        }
        __syncthreads();
    }
}

// Test hook: lKFsSharingWords of one query in the reference's order.  The select kernel leaves the listed slots
// unordered (it orders the scored ones only); this sorts them with the same keys and the same routine.
__global__ void __launch_bounds__(kSelThreads) kfdb_list_sort_kernel(Table t, const int32_t *first, int32_t *list_slot,
                                                                     int n_list, uint64_t *gkey, int32_t *gval) {
    extern __shared__ uint64_t lds_sort[];
    int P = 1;
    while (P < n_list) P <<= 1;
    uint64_t *key = P <= kLdsSortMax ? lds_sort : gkey;
    int32_t *val = P <= kLdsSortMax ? (int32_t *)(lds_sort + P) : gval;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int s = i < n_list ? list_slot[i] : -1;
        key[i] = s < 0 ? ~0ull : (((uint64_t)(uint32_t)first[s] << 32) | t.seq[s]);
        val[i] = s;
    }
    __syncthreads();
    bitonic_sort_kv(key, val, P);
    for (int i = threadIdx.x; i < n_list; i += blockDim.x) list_slot[i] = val[i];
}

}  // namespace

struct omv_kfdb {
    Table t{};
    int max_q = 0, max_qbow = 0, P_cap = 1;
    size_t conn_cap = 0;
    // per call
    int32_t *words = nullptr, *first = nullptr;
    double *score = nullptr;
    int64_t *conn_stamp = nullptr, *add_stamp = nullptr;
    uint64_t *gkey = nullptr;
    int32_t *gval = nullptr, *tmp_best = nullptr;
    uint32_t *tmp_bits = nullptr, *acc_bits = nullptr;
    uint8_t *cls = nullptr;
    int32_t *q_info = nullptr, *list_slot = nullptr, *sc_slot = nullptr, *acc_best = nullptr;
    float *sc_si = nullptr;
    // staging of the host arguments
    int64_t *d_qid = nullptr;
    int32_t *d_qmap = nullptr, *d_cstart = nullptr, *d_cslot = nullptr, *d_islot = nullptr, *d_imap = nullptr,
            *d_ineigh = nullptr;
    uint8_t *d_iflags = nullptr;
    char *pin = nullptr;   // pinned host copy of a detect call's host arrays: the call returns before they are read
    size_t pin_bytes = 0;
    hipEvent_t pin_free = nullptr;
    bool pin_busy = false;
    // host mirror
    std::vector<uint8_t> h_occ;
    std::vector<int32_t> h_map;
    uint64_t next_seq = 0;
    int64_t next_stamp = 1;
    int last_nq = 0, last_hi = 0;
    omv::DeviceArena mem;   // owns the table, the per-call and staging buffers and `pin`
    ~omv_kfdb() { if (pin_free) (void)hipEventDestroy(pin_free); }
};

namespace {

int high_slot(const omv_kfdb *h) {   // one past the highest occupied slot
    int hi = 0;
    for (int s = 0; s < h->t.max_kf; ++s)
        if (h->h_occ[s]) hi = s + 1;
    return hi;
}

bool slots_ok(const omv_kfdb *h, int n, const int32_t *slot) {
    for (int i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= h->t.max_kf) return false;
    return true;
}

omv_status detect(omv_kfdb *h, int mode, int n_q, const int64_t *query_id, const int32_t *query_map,
                  const int32_t *conn_start, const int32_t *conn_slot, const int32_t *q_bow_word,
                  const double *q_bow_value, const int32_t *q_bow_n, int stride, int n_cand, int32_t *out_a,
                  int32_t *n_a, int32_t *out_b, int32_t *n_b, void *stream) {
    if (!h || n_q < 0 || n_q > h->max_q || stride < 0 || n_cand < 0) return OMV_ERR_ARG;
    if (n_q == 0) return OMV_OK;
    if (!query_id || !query_map || !q_bow_word || !q_bow_value || !q_bow_n || !out_a || !n_a || stride == 0)
        return OMV_ERR_ARG;
    int n_conn = 0;
    if (mode == kModeNBest) {
        if (!conn_start || !out_b || !n_b || conn_start[0] != 0) return OMV_ERR_ARG;
        for (int j = 0; j < n_q; ++j)
            if (conn_start[j + 1] < conn_start[j]) return OMV_ERR_ARG;
        n_conn = conn_start[n_q];
        if (n_conn > 0 && !conn_slot) return OMV_ERR_ARG;
        if (!slots_ok(h, n_conn, conn_slot)) return OMV_ERR_ARG;
        if ((size_t)n_conn > h->conn_cap) return OMV_ERR_CAPACITY;
    }
    hipStream_t st = (hipStream_t)stream;
    if (h->pin_busy) HIP_OK(hipEventSynchronize(h->pin_free));   // the previous call's copies have left the buffer
    char *p = h->pin;
    int64_t *p_qid = (int64_t *)p;
    int32_t *p_qmap = (int32_t *)(p + 8 * (size_t)h->max_q);
    int32_t *p_cstart = p_qmap + h->max_q, *p_cslot = p_cstart + h->max_q + 1;
    memcpy(p_qid, query_id, 8 * (size_t)n_q);
    memcpy(p_qmap, query_map, 4 * (size_t)n_q);
    HIP_OK(hipMemcpyAsync(h->d_qid, p_qid, 8 * (size_t)n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->d_qmap, p_qmap, 4 * (size_t)n_q, hipMemcpyHostToDevice, st));
    if (mode == kModeNBest) {
        memcpy(p_cstart, conn_start, 4 * (size_t)(n_q + 1));
        HIP_OK(hipMemcpyAsync(h->d_cstart, p_cstart, 4 * (size_t)(n_q + 1), hipMemcpyHostToDevice, st));
        if (n_conn > 0) {
            memcpy(p_cslot, conn_slot, 4 * (size_t)n_conn);
            HIP_OK(hipMemcpyAsync(h->d_cslot, p_cslot, 4 * (size_t)n_conn, hipMemcpyHostToDevice, st));
        }
    }
    HIP_OK(hipEventRecord(h->pin_free, st));
    h->pin_busy = true;
    const int hi = high_slot(h);
    if (hi > 0) {
        const dim3 grid((hi + 3) / 4, n_q);
        kfdb_share_kernel<<<grid, 256, 0, st>>>(h->t, hi, q_bow_word, q_bow_value, q_bow_n, stride, h->max_qbow,
                                                h->words, h->first, h->score);
    }
    SelArgs a{};
    a.t = h->t, a.hi = hi, a.n_q = n_q, a.mode = mode, a.n_cand = n_cand, a.max_query_bow = h->max_qbow;
    a.stride = stride, a.qid = h->d_qid, a.qmap = h->d_qmap, a.cstart = h->d_cstart, a.cslot = h->d_cslot;
    a.q_n = q_bow_n, a.words = h->words, a.first = h->first, a.score = h->score, a.conn_stamp = h->conn_stamp;
    a.add_stamp = h->add_stamp, a.stamp0 = h->next_stamp, a.gkey = h->gkey, a.gval = h->gval;
    a.tmp_best = h->tmp_best, a.tmp_bits = h->tmp_bits, a.cls = h->cls, a.q_info = h->q_info;
    a.list_slot = h->list_slot, a.sc_slot = h->sc_slot, a.acc_best = h->acc_best, a.sc_si = h->sc_si;
    a.acc_bits = h->acc_bits, a.out_a = out_a, a.n_a = n_a, a.out_b = out_b, a.n_b = n_b;
    h->next_stamp += n_q;
    int P = 1;
    while (P < hi) P <<= 1;
    const size_t lds = P <= kLdsSortMax ? (size_t)P * 12 : 0;
    kfdb_select_kernel<<<1, kSelThreads, lds, st>>>(a);
    HIP_OK(hipGetLastError());
    h->last_nq = n_q, h->last_hi = hi;
    return OMV_OK;
}

}  // namespace

extern "C" {

omv_status omv_kfdb_destroy(omv_kfdb *h) {
    delete h;   // NULL: nothing to do, OMV_OK
    return OMV_OK;
}

omv_status omv_kfdb_create(int scoring, int max_kf, int max_bow, int max_queries, int max_query_bow, omv_kfdb **out) {
    if (!out || scoring != 0 || max_kf <= 0 || max_bow <= 0 || max_queries <= 0 || max_query_bow <= 0)
        return OMV_ERR_ARG;   // L1 scoring only (omv_vocab.scoring == 0)
    if ((long long)max_kf * kNeigh > 0x7fffffffLL) return OMV_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return OMV_ERR_NO_DEVICE;
    std::unique_ptr<omv_kfdb> h(new (std::nothrow) omv_kfdb);
    if (!h) return OMV_ERR_HIP;
    Table &t = h->t;
    omv::DeviceArena &mem = h->mem;
    t.max_kf = max_kf, t.max_bow = max_bow, h->max_q = max_queries, h->max_qbow = max_query_bow;
    while (h->P_cap < max_kf) h->P_cap <<= 1;
    h->conn_cap = (size_t)max_queries * max_kf;
    const size_t mk = max_kf, tb = mk * max_bow, qk = (size_t)max_queries * mk;
    h->pin_bytes = 8 * (size_t)max_queries + 4 * (size_t)max_queries + 4 * ((size_t)max_queries + 1) + 4 * h->conn_cap;
    bool ok = mem.alloc(&t.word, tb) && mem.alloc(&t.value, tb) && mem.alloc(&t.n, mk) && mem.alloc(&t.seq, mk) &&
              mem.alloc(&t.occ, mk) && mem.alloc(&t.map, mk) && mem.alloc(&t.neigh, mk * kNeigh) &&
              mem.alloc(&t.flags, mk) && mem.alloc(&t.st_query[0], mk) && mem.alloc(&t.st_query[1], mk) &&
              mem.alloc(&t.st_score[0], mk) && mem.alloc(&t.st_score[1], mk) && mem.alloc(&h->words, qk) &&
              mem.alloc(&h->first, qk) && mem.alloc(&h->score, qk) && mem.alloc(&h->conn_stamp, mk) &&
              mem.alloc(&h->add_stamp, mk) && mem.alloc(&h->gkey, (size_t)h->P_cap) &&
              mem.alloc(&h->gval, (size_t)h->P_cap) && mem.alloc(&h->tmp_best, mk) && mem.alloc(&h->tmp_bits, mk) &&
              mem.alloc(&h->acc_bits, qk) && mem.alloc(&h->cls, mk) && mem.alloc(&h->q_info, (size_t)4 * max_queries) &&
              mem.alloc(&h->list_slot, qk) && mem.alloc(&h->sc_slot, qk) && mem.alloc(&h->acc_best, qk) &&
              mem.alloc(&h->sc_si, qk) && mem.alloc(&h->d_qid, (size_t)max_queries) &&
              mem.alloc(&h->d_qmap, (size_t)max_queries) && mem.alloc(&h->d_cstart, (size_t)max_queries + 1) &&
              mem.alloc(&h->d_cslot, h->conn_cap) && mem.alloc(&h->d_islot, mk) && mem.alloc(&h->d_imap, mk) &&
              mem.alloc(&h->d_ineigh, mk * kNeigh) && mem.alloc(&h->d_iflags, mk) &&
              mem.alloc_pinned(&h->pin, h->pin_bytes) &&
              hipEventCreateWithFlags(&h->pin_free, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemset(t.occ, 0, mk) == hipSuccess && hipMemset(t.n, 0, mk * 4) == hipSuccess &&
         hipMemset(t.seq, 0, mk * 4) == hipSuccess && hipMemset(t.map, 0, mk * 4) == hipSuccess &&
         hipMemset(t.neigh, 0xff, mk * kNeigh * 4) == hipSuccess && hipMemset(t.flags, 0, mk) == hipSuccess &&
         hipMemset(t.st_query[0], 0, mk * 8) == hipSuccess && hipMemset(t.st_query[1], 0, mk * 8) == hipSuccess &&
         hipMemset(t.st_score[0], 0, mk * 4) == hipSuccess && hipMemset(t.st_score[1], 0, mk * 4) == hipSuccess &&
         hipMemset(h->conn_stamp, 0, mk * 8) == hipSuccess && hipMemset(h->add_stamp, 0, mk * 8) == hipSuccess &&
         hipMemset(h->q_info, 0, (size_t)16 * max_queries) == hipSuccess;
    if (ok && h->P_cap <= kLdsSortMax && (size_t)h->P_cap * 12 > 48 * 1024)
        ok = hipFuncSetAttribute((const void *)kfdb_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kLdsSortMax * 12) == hipSuccess &&
             hipFuncSetAttribute((const void *)kfdb_list_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kLdsSortMax * 12) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return OMV_ERR_HIP;
    }
    h->h_occ.assign(mk, 0), h->h_map.assign(mk, 0);
    *out = h.release();
    return OMV_OK;
}

omv_status omv_kfdb_add(omv_kfdb *h, int n, const int32_t *slot, const int32_t *map_id, const int32_t *bow_word,
                        const double *bow_value, const int32_t *bow_n, int stride, void *stream) {
    if (!h || n < 0 || stride < 0) return OMV_ERR_ARG;
    if (n == 0) return OMV_OK;
    if (!slot || !map_id || !bow_word || !bow_value || !bow_n || stride == 0 || n > h->t.max_kf) return OMV_ERR_ARG;
    if (!slots_ok(h, n, slot)) return OMV_ERR_ARG;
    std::vector<uint8_t> seen(h->t.max_kf, 0);
    for (int i = 0; i < n; ++i) {   // an occupied slot, or one named twice
        if (h->h_occ[slot[i]] || seen[slot[i]]) return OMV_ERR_ARG;
        seen[slot[i]] = 1;
    }
    if (h->next_seq + (uint64_t)n > 0xffffffffull) return OMV_ERR_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> bn(n);
    HIP_OK(hipMemcpyAsync(bn.data(), bow_n, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        if (bn[i] < 0 || bn[i] > stride) return OMV_ERR_ARG;
        if (bn[i] > h->t.max_bow) return OMV_ERR_CAPACITY;
    }
    HIP_OK(hipMemcpyAsync(h->d_islot, slot, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->d_imap, map_id, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    kfdb_add_kernel<<<n, 256, 0, st>>>(h->t, h->d_islot, h->d_imap, bow_word, bow_value, bow_n, stride,
                                       (uint32_t)h->next_seq);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));   // the host arrays and the staging buffers are free again
    for (int i = 0; i < n; ++i) h->h_occ[slot[i]] = 1, h->h_map[slot[i]] = map_id[i];
    h->next_seq += (uint64_t)n;
    return OMV_OK;
}

static omv_status scatter(omv_kfdb *h, int what, int n, const int32_t *slot, const int32_t *neigh, const uint8_t *flags,
                          void *stream) {
    if (!h || n < 0) return OMV_ERR_ARG;
    if (n == 0) return OMV_OK;
    if (!slot || n > h->t.max_kf || (what == 1 && !neigh) || (what == 2 && !flags)) return OMV_ERR_ARG;
    if (!slots_ok(h, n, slot)) return OMV_ERR_ARG;
    if (what == 1)
        for (int i = 0; i < n * kNeigh; ++i)
            if (neigh[i] < -1 || neigh[i] >= h->t.max_kf) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(h->d_islot, slot, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    if (what == 1) HIP_OK(hipMemcpyAsync(h->d_ineigh, neigh, 4 * (size_t)n * kNeigh, hipMemcpyHostToDevice, st));
    if (what == 2) HIP_OK(hipMemcpyAsync(h->d_iflags, flags, (size_t)n, hipMemcpyHostToDevice, st));
    kfdb_scatter_kernel<<<(n + 255) / 256, 256, 0, st>>>(h->t, what, n, h->d_islot, h->d_ineigh, h->d_iflags);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    if (what == 0)
        for (int i = 0; i < n; ++i) h->h_occ[slot[i]] = 0;
    return OMV_OK;
}

omv_status omv_kfdb_erase(omv_kfdb *h, int n, const int32_t *slot, void *stream) {
    return scatter(h, 0, n, slot, nullptr, nullptr, stream);
}

omv_status omv_kfdb_set_neighbours(omv_kfdb *h, int n, const int32_t *slot, const int32_t *neigh, void *stream) {
    return scatter(h, 1, n, slot, neigh, nullptr, stream);
}

omv_status omv_kfdb_set_flags(omv_kfdb *h, int n, const int32_t *slot, const uint8_t *flags, void *stream) {
    return scatter(h, 2, n, slot, nullptr, flags, stream);
}

static omv_status clear(omv_kfdb *h, int all, int map_id, void *stream) {
    if (!h) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    kfdb_clear_kernel<<<(h->t.max_kf + 255) / 256, 256, 0, st>>>(h->t, all, map_id);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    for (int s = 0; s < h->t.max_kf; ++s)
        if (all || h->h_map[s] == map_id) h->h_occ[s] = 0;
    return OMV_OK;
}

omv_status omv_kfdb_clear(omv_kfdb *h, void *stream) { return clear(h, 1, 0, stream); }

omv_status omv_kfdb_clear_map(omv_kfdb *h, int map_id, void *stream) { return clear(h, 0, map_id, stream); }

omv_status omv_kfdb_detect_n_best(omv_kfdb *h, int n_q, const int64_t *query_id, const int32_t *query_map,
                                  const int32_t *conn_start, const int32_t *conn_slot, const int32_t *q_bow_word,
                                  const double *q_bow_value, const int32_t *q_bow_n, int stride, int n_candidates,
                                  int32_t *loop_out, int32_t *n_loop, int32_t *merge_out, int32_t *n_merge,
                                  void *stream) {
    return detect(h, kModeNBest, n_q, query_id, query_map, conn_start, conn_slot, q_bow_word, q_bow_value, q_bow_n,
                  stride, n_candidates, loop_out, n_loop, merge_out, n_merge, stream);
}

omv_status omv_kfdb_detect_reloc(omv_kfdb *h, int n_q, const int64_t *frame_id, const int32_t *map_id,
                                 const int32_t *q_bow_word, const double *q_bow_value, const int32_t *q_bow_n,
                                 int stride, int32_t *cand_out, int32_t *n_cand, void *stream) {
    return detect(h, kModeReloc, n_q, frame_id, map_id, nullptr, nullptr, q_bow_word, q_bow_value, q_bow_n, stride, 0,
                  cand_out, n_cand, nullptr, nullptr, stream);
}

omv_status omv_kfdb_debug(omv_kfdb *h, int query, int32_t *max_common_words, int32_t *min_common_words,
                          int32_t *n_list, int32_t *list_slot, int32_t *list_words, int32_t *n_scored,
                          int32_t *scored_slot, double *score, float *si, uint32_t *acc_bits, int32_t *acc_best,
                          void *stream) {
    if (!h || query < 0 || query >= h->last_nq) return OMV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t mk = h->t.max_kf, row = (size_t)query * mk;
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    int32_t qi[4];
    HIP_OK(hipMemcpyAsync(qi, h->q_info + 4 * query, sizeof(qi), k, st));
    HIP_OK(hipStreamSynchronize(st));
    const int nl = qi[2], ns = qi[3];
    if (max_common_words) *max_common_words = qi[0];
    if (min_common_words) *min_common_words = qi[1];
    if (n_list) *n_list = nl;
    if (n_scored) *n_scored = ns;
    std::vector<int32_t> ls(nl), ss(ns), w(h->last_hi);
    std::vector<double> sc(h->last_hi);
    if (nl && (list_slot || list_words)) {
        int P = 1;
        while (P < nl) P <<= 1;
        kfdb_list_sort_kernel<<<1, kSelThreads, P <= kLdsSortMax ? (size_t)P * 12 : 0, st>>>(
            h->t, h->first + row, h->list_slot + row, nl, h->gkey, h->gval);
        HIP_OK(hipGetLastError());
    }
    if (nl) HIP_OK(hipMemcpyAsync(ls.data(), h->list_slot + row, 4 * (size_t)nl, k, st));
    if (ns) HIP_OK(hipMemcpyAsync(ss.data(), h->sc_slot + row, 4 * (size_t)ns, k, st));
    if (h->last_hi) {
        HIP_OK(hipMemcpyAsync(w.data(), h->words + row, 4 * (size_t)h->last_hi, k, st));
        HIP_OK(hipMemcpyAsync(sc.data(), h->score + row, 8 * (size_t)h->last_hi, k, st));
    }
    if (si && ns) HIP_OK(hipMemcpyAsync(si, h->sc_si + row, 4 * (size_t)ns, k, st));
    if (acc_bits && ns) HIP_OK(hipMemcpyAsync(acc_bits, h->acc_bits + row, 4 * (size_t)ns, k, st));
    if (acc_best && ns) HIP_OK(hipMemcpyAsync(acc_best, h->acc_best + row, 4 * (size_t)ns, k, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < nl; ++i) {
        if (list_slot) list_slot[i] = ls[i];
        if (list_words) list_words[i] = w[ls[i]];
    }
    for (int i = 0; i < ns; ++i) {
        if (scored_slot) scored_slot[i] = ss[i];
        if (score) score[i] = sc[ss[i]];
    }
    return OMV_OK;
}

}  // extern "C"
