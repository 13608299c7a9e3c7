// Device-side building blocks of the prefilter kernels (pf_kernels.hip, pf_shard_kernels.hip) and of the prefilter -> alignment
// hand-over (sw_kernel.hip): wavefront primitives, the block-wide sorting network, and the steps of the selection that more than one
// kernel performs.  Device only; every function is forced inline and has internal linkage (the anonymous namespace: each of the
// including files is a code object of its own).
#pragma once

#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
// __ballot() takes an int: a bool argument is materialised (v_cndmask 0 / 1) and compared with zero again - two VALU
// instructions per ballot in kernels that are bound by instruction issue.  The builtin takes the condition as it is.
__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// Inclusive scans over the wavefront with DPP moves (row shifts inside the 16-lane rows, then the row ends handed to the
// following rows): six VALU operations instead of six ds_bpermute round trips.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111 /* row_shr:1 */, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112 /* row_shr:2 */, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114 /* row_shr:4 */, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118 /* row_shr:8 */, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142 /* row_bcast:15 */, 0xA, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143 /* row_bcast:31 */, 0xC, 0xF, false);
    return (uint32_t)x;
}
__device__ __forceinline__ int wave_incl_max_scan(int v) {      // v >= 0
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false));
    return v;
}

// Largest lane m with start[m] <= x, for per-lane non-decreasing `start` with start[0] <= x.  Every lane of
// the wave must call this (it shuffles).
__device__ __forceinline__ int seg_find(uint32_t start_mine, uint32_t x) {
    int lo = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const uint32_t s = __shfl(start_mine, lo + step);
        if (s <= x) lo += step;
    }
    return lo;
}

// Lanes of the wave whose `key` (low nbits) equals mine, among lanes with active == true.
__device__ __forceinline__ uint64_t match_lanes(uint32_t key, int nbits, bool active) {
    const uint64_t act = ballot(active);
    uint32_t lo = (uint32_t)act, hi = (uint32_t)(act >> 32);
    for (int b = 0; b < nbits; b++) {
        // per bit: m &= (my bit set ? lanes with the bit : lanes without) = m & ~(ballot ^ my bit spread over the word):
        // one v_bfe_i32, one compare, one v_bitop3 per half
        const int ext = __builtin_amdgcn_sbfe((int)key, (unsigned)b, 1u);      // 0 or -1
        const uint64_t bal = ballot(ext != 0);
        lo = __builtin_amdgcn_bitop3_b32(lo, (uint32_t)bal, (uint32_t)ext, 0x90);
        hi = __builtin_amdgcn_bitop3_b32(hi, (uint32_t)(bal >> 32), (uint32_t)ext, 0x90);
    }
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

__device__ __forceinline__ int highest_lane(uint64_t m) { return 63 - __clzll((long long)m); }

// Largest index in [lo, hi] whose value (base[idx * stride], non-decreasing, base[lo * stride] <= key) is <= key.
// The whole wavefront probes 64 evenly spaced elements per round: log64 instead of log2 dependent memory round trips.
__device__ __forceinline__ uint32_t wave_search_le(const uint32_t *base, uint32_t stride, uint32_t lo, uint32_t hi, uint32_t key) {
    const uint32_t lane = (uint32_t)lane_id();
    while (hi > lo) {
        const uint32_t span = hi - lo + 1;
        const uint32_t step = (span + 63u) / 64u;
        const uint32_t idx = lo + lane * step;
        const bool in = idx <= hi;
        const uint32_t v = in ? base[(size_t)idx * stride] : 0xFFFFFFFFu;
        const uint64_t le = ballot(in && v <= key);   // a prefix of the lanes
        const uint32_t k = (uint32_t)__popcll(le) - 1u;
        lo += k * step;
        hi = min(hi, lo + step - 1u);
    }
    return lo;
}

// XCD-aware order of a grid's workgroups.  The dispatcher places workgroup b on XCD b % 8 (observed, not a contract: a wrong guess
// only costs speed); each XCD has its own 4 MB L2.  swz gives XCD x the x-th CONTIGUOUS eighth of the work items, in order, so
// that items that are neighbours in the work order meet in one L2 (bijective for any grid size).
__device__ __forceinline__ uint32_t xcd_contiguous(uint32_t bid, uint32_t nwg) {
    const uint32_t xcd = bid & 7u, q = nwg >> 3, r = nwg & 7u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (bid >> 3);
}

// ---------------------------------------------------------------------------------------------------------
// Steps that several prefilter kernels share.  Everything is forced inline: a call site compiles to what it spelled out before.

// log2 of the number of bins (a power of two)
__device__ __forceinline__ int pf_bin_shift(uint32_t B) {
    int bshift = 0;
    while ((1u << bshift) < B) bshift++;
    return bshift;
}

__device__ __forceinline__ PfCand pf_cand_zero() { return PfCand{}; }      // every field zero

// The substitution matrix in LDS in rows of 32 (seg_cells_n), zero outside the alphabet.  The caller places the barrier.
template <int THREADS>
__device__ __forceinline__ void pf_load_smat32(int8_t *smat, const int8_t *mat, int alphabet) {
    for (int k = (int)threadIdx.x; k < 32 * 32; k += THREADS)
        smat[k] = ((k >> 5) < alphabet && (k & 31) < alphabet) ? mat[(k >> 5) * alphabet + (k & 31)] : (int8_t)0;
}

// Sum of `v` over the wavefront, added to *counter by one atomic (none when the sum is zero).  Every lane must call this.
__device__ __forceinline__ void wave_sum_to(unsigned long long *counter, unsigned long long v) {
    for (int dd = 1; dd < 64; dd <<= 1) v += __shfl_xor(v, dd);
    if (lane_id() == 0 && v) atomicAdd(counter, v);
}

// The (query, bin) bucket of this wavefront in a grid of `waves_per_block` wavefronts per workgroup over the buckets of the launch's
// queries; false when the grid's last workgroup reaches past them.
template <class Args>
__device__ __forceinline__ bool pf_wave_bucket(const Args &A, uint32_t waves_per_block, uint64_t *bucket) {
    *bucket = (uint64_t)A.q_first * A.bins + (uint64_t)blockIdx.x * waves_per_block + (uint32_t)(threadIdx.x >> 6);
    return *bucket < (uint64_t)(A.q_first + A.n_queries) * A.bins;
}

// keepMaxElement's table entry (CacheFriendlyOperations.cpp:354-384): the highest count wins, among equal counts the lowest candidate
// index.  `cnt` is the element's count - min(255, score), or pf_el_count(score) where counts were reassigned (pf_long_kernel).
__device__ __forceinline__ uint32_t keepmax_key(uint32_t cnt, uint32_t ci) { return (cnt << 24) | (0xFFFFFFu - min(ci, 0xFFFFFEu)); }

// The lanes with win == true take consecutive slots behind *counter (one atomic per wavefront) and store `value` there - those
// whose slot lies below `cap`, where the list has one (the counter goes on counting).  Returns the lane's slot (meaningless where
// win is false).  Every lane of the wavefront must call this.
constexpr uint32_t WAVE_APPEND_NO_CAP = 0xFFFFFFFFu;
template <class T>
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, T *dst, bool win, const T &value, uint32_t cap = WAVE_APPEND_NO_CAP) {
    const int lane = lane_id();
    const uint64_t wb = ballot(win);
    uint32_t slot = 0;
    if (wb) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll(wb));
        base = __shfl(base, 0);
        slot = base + (uint32_t)__popcll(wb & lanes_below(lane));
        if (win && (cap == WAVE_APPEND_NO_CAP || slot < cap)) dst[slot] = value;
    }
    return slot;
}

// Bitonic sorting network over n (a power of two) elements by a workgroup of THREADS threads: after it greater(i, j) is false for
// every i < j.  `greater` and `exchange` name the elements by index; padding up to n is the caller's.  FENCE: the elements live
// in global memory.  Ends with a barrier.
template <int THREADS, bool FENCE = false, class Greater, class Exchange>
__device__ __forceinline__ void block_bitonic_sort(uint32_t n, Greater greater, Exchange exchange) {
    for (uint32_t size = 2; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t k = threadIdx.x; k < n / 2; k += THREADS) {
                const uint32_t i = 2 * k - (k & (stride - 1));
                const uint32_t j = i + stride;
                const bool up = (i & size) == 0;
                if (greater(i, j) == up) exchange(i, j);
            }
            if (FENCE) __threadfence();
            __syncthreads();
        }
    }
}
template <class T>
__device__ __forceinline__ void exchange_at(T *v, uint32_t i, uint32_t j) {
    const T t = v[i];
    v[i] = v[j];
    v[j] = t;
}

// ---------------------------------------------------------------------------------------------------------
// a9, the end of the selection (pf_select_kernel; pf_xmerge_kernel over the union of the shards' records).

// computeScoreThreshold (QueryMatcher.h:211-221) over the histogram of the counts, not below min_diag_score.  One thread.
__device__ __forceinline__ uint32_t pf_score_threshold(const uint32_t *hist, uint32_t max_hits, uint32_t min_diag_score) {
    uint32_t found = 0, thr = 0;
    for (thr = 255; thr > 0; thr--) {
        found += hist[thr];
        if (found >= max_hits) break;
    }
    return max(min_diag_score, thr);
}

// maxSelfScore of rescoreHits: the query's self score above the saturation point, within [1, 65535]
__device__ __forceinline__ int pf_self_clamp(int self_score) {
    int ms = self_score - 255;
    ms = ms > 1 ? ms : 1;
    ms = ms < 65535 ? ms : 65535;
    return ms;
}

__device__ __forceinline__ uint32_t rescaled_count(uint32_t score, float fms) {
    // rescoreHits, QueryMatcher.cpp:576-581: (score - 255) / maxSelfScore * 255 + 0.5, float arithmetic, cut to a byte
    const uint32_t ns = score - 255u;
    const float sc = (float)min(ns, 65535u);
    const float r = __fmul_rn(__fdiv_rn(sc, fms), 255.0f);
    const double dd = (double)r + 0.5;
    return (uint32_t)(int)dd & 0xFFu;
}

// prefScore of a selected element (getResult, QueryMatcher.cpp:430-452): under a truncated threshold the rescaled count spread over
// the self score; else the exact score of a saturated element (not for getResult<KMER_SCORE>), the count of any other.
__device__ __forceinline__ uint32_t pf_pref_score(bool trunc, bool kmer_score, uint32_t cnt, uint32_t exact, int ms) {
    if (trunc) return 255u + (rescaled_count(exact, (float)ms) * (uint32_t)ms / 255u);
    return (cnt >= 255u && !kmer_score) ? exact : cnt;
}

// Sort key of hit_t::compareHitsByScoreAndId (QueryMatcher.h:38-49): score descending, id ascending
__device__ __forceinline__ uint64_t pf_hit_key(uint32_t score, uint32_t id) { return ((uint64_t)(0xFFFFFFFFu - score) << 32) | (uint64_t)id; }

// The hit list of a query from its n sorted keys - key(k) and diag(k) hand out the k-th - behind the self hit (getResult :408-424)
// when nself == 1.  Returns the list's length.
template <int THREADS, class Key, class Diag>
__device__ __forceinline__ uint32_t pf_write_hits(mmgpu_pf_hit *out, uint32_t nself, uint32_t ident, int32_t self_score, uint32_t n,
                                                  Key key, Diag diag) {
    for (uint32_t k = threadIdx.x; k < n; k += THREADS) {
        const uint64_t kk = key(k);
        mmgpu_pf_hit h;
        h.id = (uint32_t)kk;
        h.score = (int32_t)(0xFFFFFFFFu - (uint32_t)(kk >> 32));
        h.diagonal = diag(k);
        h.reserved = 0;
        out[nself + k] = h;
    }
    if (threadIdx.x == 0 && nself) {
        mmgpu_pf_hit h;
        h.id = ident;
        h.score = self_score;
        h.diagonal = 0;
        h.reserved = 0;
        out[0] = h;
    }
    return nself + n;
}

}  // namespace

}  // namespace mmgpu
