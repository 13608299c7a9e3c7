// Exhaustive gapped scan for gfx950 / CDNA4 (include/mmgpu.h, "exhaustive gapped scan"): what runs around the Gotoh kernels.  The
// pairs themselves are scored by the forward kernels of an alignment batch (sw_kernel.hip, sw_half_kernel.hip), untouched; this file
// holds the three small kernels that feed them and read their records:
//  * the planner writes a chunk's lists: the pairs of query q are positions [q_begin, q_begin + q_count) of the length-ordered id
//    list (longest first - the order the alignment kernels want), pair p of it takes slot q_slot + p of the chunk's arrays.
//  * the identity kernel: SmithWaterman::scoreIdentical's diagonal sum for the queries that have their own target in the window.
//  * the selection kernel, one workgroup per query: it spreads the chunk's records into the query's row of the [query][target]
//    score array (id order, 0 outside the window, the identity score over the aligned one), then builds the list out of the row:
//    keys k = 32767 - score in [0, 65535]; a 256-bin histogram of k >> 8 finds the bin the cut falls into, one of k & 255 inside that
//    bin the cut key; compaction in id order with ballot prefix sums takes every key below the cut and the first ids of the cut
//    class; at most GSCAN_MAX_HITS keys (k << 32 | id) are sorted in LDS.  The histograms' atomics only count.
#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

constexpr int PLAN_THREADS = 256;
constexpr int SELECT_THREADS = 1024;
static_assert(GSCAN_MAX_HITS == MMGPU_PF_MAX_FUSED_HITS, "the selection kernel sorts every list the C-ABI admits");

__global__ __launch_bounds__(PLAN_THREADS) void gscan_plan_kernel(GscanPlanArgs A) {
    for (uint32_t ql = blockIdx.y; ql < A.n_queries; ql += gridDim.y) {
        const uint32_t q = A.q_first + ql;
        const uint32_t n = A.q_count[q], begin = A.q_begin[q], slot = A.q_slot[q];
        for (uint32_t p = blockIdx.x * PLAN_THREADS + threadIdx.x; p < n; p += gridDim.x * PLAN_THREADS) {
            A.hit_target[slot + p] = A.order[begin + p];
            A.hit_out[slot + p] = slot + p;
        }
    }
}

// One wavefront per query.  The reference adds the terms one after the other into a short; addition modulo 2^16 is associative, so
// the int32 sum of all terms (at most 65535 x 255 in size), cut to its low 16 bits and read as int16, is the same number.
__global__ __launch_bounds__(64) void gscan_identity_kernel(GscanIdentArgs A) {
    const uint32_t q = blockIdx.x;
    const uint32_t id = A.q_ident[q];
    if (id == 0xFFFFFFFFu) {
        if (threadIdx.x == 0) A.ident_score[q] = 0;
        return;
    }
    const uint32_t qo = A.q_off[q], qlen = A.q_off[q + 1] - qo;
    const uint8_t *t = A.t_res + (size_t)A.t_off4[id] * 4u;
    const uint32_t po = A.q_prof ? A.q_prof_off[q] : 0xFFFFFFFFu;
    int sum = 0;
    for (uint32_t pos = threadIdx.x; pos < qlen; pos += 64) {
        const uint32_t letter = t[pos];
        if (po != 0xFFFFFFFFu) sum += (int)A.q_prof[(size_t)po + (size_t)letter * qlen + pos];
        else sum += (int)A.mat[letter * (uint32_t)A.alphabet + A.q_res[qo + pos]] + (int)A.q_cb[qo + pos];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (threadIdx.x == 0) A.ident_score[q] = (int)(short)(unsigned short)((unsigned)sum & 0xFFFFu);
}

__global__ __launch_bounds__(SELECT_THREADS) void gscan_select_kernel(GscanSelectArgs A) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long keys[GSCAN_MAX_HITS];
    __shared__ unsigned wsum[2][2][SELECT_THREADS / 64];
    __shared__ unsigned s_bin, s_above, s_cut, s_need;
    const uint32_t q = A.q_first + blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t n = A.n_targets;
    int32_t *row = A.scores + (size_t)q * n;
    const uint32_t ident = A.q_ident[q], lo = A.q_win[2 * q], hi = A.q_win[2 * q + 1];
    const uint32_t count = A.q_count[q], begin = A.q_begin[q], slot = A.q_slot[q];
    const int min_ev = A.q_min_ev[q];

    // the row: 0 outside the window, the records' scores inside, the identity score over its pair's
    if (count < n) {
        for (uint64_t i = tid; i < n; i += SELECT_THREADS) row[i] = 0;
        __syncthreads();
    }
    for (uint32_t p = tid; p < count; p += SELECT_THREADS) row[A.order[begin + p]] = A.out[(size_t)slot + p].score;
    __syncthreads();
    if (tid == 0 && ident != 0xFFFFFFFFu) row[ident] = A.ident_score[q];
    if (tid < 256) hist[tid] = 0;
    __syncthreads();

    // admitted: inside the window, and the query's own target or past both thresholds
    auto admitted = [&](uint64_t i, int s) {
        const uint32_t len = A.t_len[i];
        return len >= lo && len <= hi && ((uint32_t)i == ident || (s > A.min_score && s >= min_ev));
    };
    for (uint64_t i = tid; i < n; i += SELECT_THREADS) {
        const int s = row[i];
        if (admitted(i, s)) atomicAdd(&hist[(unsigned)(32767 - s) >> 8], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int b = 0; b < 256; b++) total += hist[b];
        unsigned bin = 256, above = 0;
        if (total > A.max_hits) {      // the high byte the cut falls into
            for (unsigned b = 0; b < 256; b++) {
                if (above + hist[b] >= A.max_hits) { bin = b; break; }
                above += hist[b];
            }
        }
        s_bin = bin;
        s_above = above;
        s_cut = 65536u;      // no cut: every admitted key is below it
        s_need = 0;
    }
    __syncthreads();
    const unsigned bin = s_bin;
    if (bin < 256u) {      // (uniform over the workgroup) the low byte inside that bin, and how many of the cut class's lowest ids are kept
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint64_t i = tid; i < n; i += SELECT_THREADS) {
            const int s = row[i];
            const unsigned k = (unsigned)(32767 - s);
            if ((k >> 8) == bin && admitted(i, s)) atomicAdd(&hist[k & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned above = s_above;
            for (unsigned b = 0; b < 256; b++) {
                if (above + hist[b] >= A.max_hits) { s_cut = (bin << 8) | b; s_need = A.max_hits - above; break; }
                above += hist[b];
            }
        }
        __syncthreads();
    }
    const unsigned cut = s_cut, need = s_need;

    // compaction in id order: everything below the cut key, the first `need` of the cut class
    unsigned cbase = 0, obase = 0;
    unsigned par = 0;
    for (uint64_t start = 0; start < n; start += SELECT_THREADS, par ^= 1u) {
        const uint64_t i = start + tid;
        unsigned k = 0;
        bool adm = false;
        if (i < n) {
            const int s = row[i];
            k = (unsigned)(32767 - s);
            adm = admitted(i, s);
        }
        const bool isA = adm && k < cut, isC = adm && k == cut;
        const unsigned long long bA = __ballot(isA), bC = __ballot(isC);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) { wsum[par][0][wv] = (unsigned)__popcll(bA); wsum[par][1][wv] = (unsigned)__popcll(bC); }
        __syncthreads();
        unsigned a_before = (unsigned)__popcll(bA & below), c_before = (unsigned)__popcll(bC & below), a_tot = 0, c_tot = 0;
        for (unsigned w = 0; w < SELECT_THREADS / 64; w++) {
            const unsigned a = wsum[par][0][w], c = wsum[par][1][w];
            if (w < wv) { a_before += a; c_before += c; }
            a_tot += a; c_tot += c;
        }
        const unsigned taken0 = min(need, cbase);
        const bool take = isA || (isC && cbase + c_before < need);
        if (take) {
            const unsigned pos = obase + a_before + (min(need, cbase + c_before) - taken0);
            keys[pos] = ((unsigned long long)k << 32) | (unsigned long long)(uint32_t)i;
        }
        obase += a_tot + (min(need, cbase + c_tot) - taken0);
        cbase += c_tot;
    }
    __syncthreads();
    const unsigned total = obase;      // <= max_hits <= GSCAN_MAX_HITS by the choice of the cut
    unsigned np2 = 1;
    while (np2 < total) np2 <<= 1;
    for (unsigned t = total + tid; t < np2; t += SELECT_THREADS) keys[t] = ~0ull;
    __syncthreads();
    for (unsigned kk = 2; kk <= np2; kk <<= 1) {
        for (unsigned j = kk >> 1; j > 0; j >>= 1) {
            for (unsigned t = tid; t < np2; t += SELECT_THREADS) {
                const unsigned x = t ^ j;
                if (x > t) {
                    const unsigned long long a = keys[t], b = keys[x];
                    if ((a > b) == ((t & kk) == 0)) { keys[t] = b; keys[x] = a; }
                }
            }
            __syncthreads();
        }
    }
    mmgpu_pf_hit *out = A.hits + (size_t)q * A.stride;
    for (unsigned t = tid; t < A.stride; t += SELECT_THREADS) {
        mmgpu_pf_hit h = {0, 0, 0, 0};
        if (t < total) {
            const unsigned long long key = keys[t];
            h.id = (uint32_t)key;
            h.score = 32767 - (int32_t)(key >> 32);
        }
        out[t] = h;
    }
    if (tid == 0) A.counts[q] = total;
}

}  // namespace

hipError_t launch_gscan_plan(const GscanPlanArgs &A, hipStream_t stream) {
    if (A.n_queries == 0) return hipSuccess;
    // (the grid's x covers the longest slice with a grid-stride loop; 256 workgroups of 256 threads per query keep the copies wide)
    hipLaunchKernelGGL(gscan_plan_kernel, dim3(256, std::min<uint32_t>(A.n_queries, 65535u)), dim3(PLAN_THREADS), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_gscan_identity(const GscanIdentArgs &A, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(gscan_identity_kernel, dim3(nq), dim3(64), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_gscan_select(const GscanSelectArgs &A, uint32_t n_queries, hipStream_t stream) {
    if (n_queries == 0) return hipSuccess;
    if (A.max_hits == 0 || A.max_hits > (uint32_t)GSCAN_MAX_HITS) return hipErrorInvalidValue;      // the key array must never be short
    hipLaunchKernelGGL(gscan_select_kernel, dim3(n_queries), dim3(SELECT_THREADS), 0, stream, A);
    return hipGetLastError();
}

void warm_gscan() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&gscan_select_kernel));
}

}  // namespace mmgpu
