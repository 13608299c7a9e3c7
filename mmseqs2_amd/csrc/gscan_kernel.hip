// Exhaustive gapped scan for gfx950 / CDNA4 (include/mmgpu.h, "exhaustive gapped scan"): what runs around the Gotoh kernels.  The
// pairs themselves are scored by the forward kernels of an alignment batch (sw_kernel.hip, sw_half_kernel.hip), untouched; this file
// holds the three small kernels that feed them and read their records:
//  * the planner writes a chunk's lists: the pairs of query q are positions [q_begin, q_begin + q_count) of the length-ordered id
//    list (longest first - the order the alignment kernels want), pair p of it takes slot q_slot + p of the chunk's arrays.
//  * the identity kernel: SmithWaterman::scoreIdentical's diagonal sum for the queries that have their own target in the window.
//  * the selection kernel, one workgroup per query: it spreads the chunk's records into the query's row of the [query][target]
//    score array (id order, 0 outside the window, the identity score over the aligned one), then builds the list out of the row:
//    keys k = 32767 - score in [0, 65535]; a 256-bin histogram of k >> 8 finds the bin the cut falls into, one of k & 255 inside that
//    bin the cut key; compaction, sort and the write of the list are select_device.h's, shared with scan_kernel.hip.  The
//    histograms' atomics only count.
#include "mmgpu_internal.h"
#include "select_device.h"

namespace mmgpu {

namespace {

constexpr int PLAN_THREADS = 256;

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
    __shared__ unsigned hist[SELECT_BINS];
    __shared__ SelectLds lds;
    __shared__ unsigned s_bin, s_above, s_cut, s_need;
    const uint32_t q = A.q_first + blockIdx.x;
    const unsigned tid = threadIdx.x;
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
    if (tid < SELECT_BINS) hist[tid] = 0;
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
        for (int b = 0; b < SELECT_BINS; b++) total += hist[b];
        SelectCut c = {SELECT_BINS, 0};
        if (total > A.max_hits) c = select_cut_walk(hist, 0, A.max_hits);      // the high byte the cut falls into
        s_bin = c.bin;
        s_above = c.above;
        s_cut = 65536u;      // no cut: every admitted key is below it
        s_need = 0;
    }
    __syncthreads();
    const unsigned bin = s_bin;
    if (bin < (unsigned)SELECT_BINS) {      // (uniform over the workgroup) the low byte inside that bin, and how many of the cut class's lowest ids are kept
        if (tid < SELECT_BINS) hist[tid] = 0;
        __syncthreads();
        for (uint64_t i = tid; i < n; i += SELECT_THREADS) {
            const int s = row[i];
            const unsigned k = (unsigned)(32767 - s);
            if ((k >> 8) == bin && admitted(i, s)) atomicAdd(&hist[k & 255u], 1u);      // (the lengths are read for that bin's targets only)
        }
        __syncthreads();
        if (tid == 0) {
            const SelectCut c = select_cut_walk(hist, s_above, A.max_hits);
            if (c.bin < (unsigned)SELECT_BINS) { s_cut = (bin << 8) | c.bin; s_need = A.max_hits - c.above; }
        }
        __syncthreads();
    }
    auto key_of = [&](uint64_t i, unsigned &k) {
        const int s = row[i];
        k = (unsigned)(32767 - s);
        return admitted(i, s);
    };
    select_emit(n, key_of, s_cut, s_need, lds, 32767, A.hits + (size_t)q * A.stride, A.stride, &A.counts[q]);
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
    if (A.max_hits == 0 || A.max_hits > (uint32_t)SELECT_MAX_HITS) return hipErrorInvalidValue;      // the key array must never be short
    hipLaunchKernelGGL(gscan_select_kernel, dim3(n_queries), dim3(SELECT_THREADS), 0, stream, A);
    return hipGetLastError();
}

void warm_gscan() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&gscan_select_kernel));
}

}  // namespace mmgpu
