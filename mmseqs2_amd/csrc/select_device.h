// Device-side steps of the list selection that the two exhaustive scans share (scan_kernel.hip, gscan_kernel.hip): one workgroup of
// SELECT_THREADS per query turns a row of scores into the query's list.  Each kernel keeps what is its own - how a score row becomes
// "admitted + key", and how many histogram levels find the cut - and calls these for the rest.  Device only; every function is
// forced inline and has internal linkage (the anonymous namespace: each of the including files is a code object of its own).
//
// Keys ascend: key = key_top - score with key_top the highest score of the scan (255 for the score bytes, 32767 for the int16
// Gotoh scores), so the best score has the smallest key.  The list is everything with key < cut plus the `need` lowest ids with
// key == cut, sorted by (key, id); "no cut" is a cut above every key (256, 65536) with need = 0.  key_top - score reverses the order
// of the scores and keeps their classes, so "score above the cut score, the first ids of the cut score's class, best score first,
// ties by id" - what the ungapped kernel did on the scores themselves, walking its histogram downwards - selects the same set in
// the same order: its histogram is now indexed by key and walked upwards, like the gapped kernel's.
#pragma once

#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

constexpr int SELECT_THREADS = 1024;
constexpr int SELECT_MAX_HITS = 4096;      // keys a selection kernel sorts in LDS
constexpr int SELECT_BINS = 256;
static_assert(SELECT_MAX_HITS == MMGPU_PF_MAX_FUSED_HITS, "the selection kernels sort every list the C-ABI admits");

// the LDS a selection kernel declares for select_emit (16-byte aligned: the per-wave sums are read four at a time)
struct alignas(16) SelectLds {
    unsigned long long keys[SELECT_MAX_HITS];
    unsigned wsum[2][2][SELECT_THREADS / 64];
};

// The first bin b at which above + hist[b] >= max_hits, and the count of the bins before it added to `above`; bin == SELECT_BINS if
// there is none.  One thread calls it.
struct SelectCut {
    unsigned bin, above;
};
__device__ __forceinline__ SelectCut select_cut_walk(const unsigned *hist, unsigned above, unsigned max_hits) {
    for (unsigned b = 0; b < (unsigned)SELECT_BINS; b++) {
        if (above + hist[b] >= max_hits) return {b, above};
        above += hist[b];
    }
    return {(unsigned)SELECT_BINS, above};
}

// Compaction in id order (everything below the cut key, the first `need` of the cut class), padding to a power of two, the bitonic
// sort of key << 32 | id, and the query's row of hits and its count.  key_of(i, key) -> admitted, for i < n.  The whole workgroup
// calls it; the choice of cut and need keeps the list within max_hits <= SELECT_MAX_HITS keys.
template <typename KeyOf>
__device__ __forceinline__ void select_emit(uint32_t n, KeyOf key_of, unsigned cut, unsigned need, SelectLds &lds, int key_top, mmgpu_pf_hit *out,
                                            uint32_t stride, uint32_t *count) {
    const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long *keys = lds.keys;
    unsigned cbase = 0, obase = 0;
    unsigned par = 0;
    for (uint64_t start = 0; start < n; start += SELECT_THREADS, par ^= 1u) {
        const uint64_t i = start + tid;
        unsigned k = 0;
        const bool adm = i < n && key_of(i, k);
        const bool isA = adm && k < cut, isC = adm && k == cut;
        const unsigned long long bA = __ballot(isA), bC = __ballot(isC);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) { lds.wsum[par][0][wv] = (unsigned)__popcll(bA); lds.wsum[par][1][wv] = (unsigned)__popcll(bC); }
        __syncthreads();
        unsigned a_before = (unsigned)__popcll(bA & below), c_before = (unsigned)__popcll(bC & below), a_tot = 0, c_tot = 0;
        for (unsigned w = 0; w < SELECT_THREADS / 64; w++) {
            const unsigned a = lds.wsum[par][0][w], c = lds.wsum[par][1][w];
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
    const unsigned total = obase;
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
    for (unsigned t = tid; t < stride; t += SELECT_THREADS) {
        mmgpu_pf_hit h = {0, 0, 0, 0};
        if (t < total) {
            const unsigned long long key = keys[t];
            h.id = (uint32_t)key;
            h.score = key_top - (int32_t)(key >> 32);
        }
        out[t] = h;
    }
    if (tid == 0) *count = total;
}

}  // namespace

}  // namespace mmgpu
