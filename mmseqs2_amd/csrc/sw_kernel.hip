// Gotoh Smith-Waterman (affine gaps, local) for gfx950 / CDNA4 - score, end position, start position.
//
// What it computes: exactly what SmithWaterman::alignScoreEndPos (src/alignment/
// StripedSmithWaterman.cpp:892-941; sw_sse2_byte :98-299, sw_sse2_word :301-476) and the reverse scan of
// alignStartPosBacktrace (:1129-1204) compute on the CPU, bit for bit:
//     H = max(sat16(Hdiag + P), E, F);  E' = max(E - ge, H - go);  F' = max(F - ge, H - go)   (E, F >= 0)
//     t_end = first column in which the running maximum reaches its final value (:232-248, :414-425)
//     q_end = smallest query index holding that maximum in that column           (:262-271, :438-447)
// The reference runs a uint8 pass and re-runs in int16 on overflow; the kernels of this file compute in int16 (exact for
// every score the uint8 pass can represent, and saturating at 32767 exactly like sw_sse2_word), and the
// `word` flag reports which pass the reference would have ended in (score + bias >= 255, :238-242).
// The single-tile groups have twins in sw_half_kernel.hip whose forward scan runs in packed f16 first and in int16 only for
// the pairs that score past 1792 - same results; launch_sw (below) picks.  The body of both is sw_body.h:
// sw_body runs a job as named steps (sw_query, sw_profiles / sw_build_profiles, sw_pack_live, sw_claim_chunk, then - inline - the
// pair setup, the tile scan with the column step, and the fold, then sw_write_result); the kernels here add the job prologue
// (sw_clip_job, sw_claim_scratch / sw_release_scratch) and pick the body with sw_dispatch_shape.
//
// How it is mapped to CDNA4 (this is not the striped/lazy-F formulation of the CPU code):
//  * integer DP => VALU, no MFMA.  All cell arithmetic is packed 2 x int16 (v_pk_add_i16 clamp,
//    v_pk_max_i16/u16, v_pk_sub_u16 clamp): the low half of every register belongs to target A, the
//    high half to target B, so one VALU lane-op advances two independent alignments.
//  * a group of 16 lanes (one DPP row) owns one pair of targets; lane g owns R consecutive query rows
//    (R = 1,2,..,32 -> 16..512 rows per tile) whose H/E state lives in registers for the whole scan.
//    Lanes run skewed by one column (anti-diagonal wavefront): at step s lane g works on column s - g.
//    The hand-off lane g -> g+1 (H of the strip's last row, the F leaving it, and the two target
//    letters) is three v_mov_b32_dpp row_shr:1 - no LDS, no bpermute.  The head lane takes zeros for H and F
//    (bound_ctrl) or the boundary row of the tile above, and its letters from a queue of four (a | b << 8) pairs
//    that is made once per four columns (two v_perm_b32; the padding letter of columns past a target's end is put
//    in there, under a scalar branch): what a column costs beside its rows is 11 VALU instructions single-tile,
//    16 multi-tile (profiles/sw_isa_audit.txt).
//  * the query profile P[letter][row] (int16, composition bias folded in) is built once per workgroup in
//    LDS; per step a lane fetches its R scores for letter a (target A) and for letter b (target B) with
//    ds_read_b128 and interleaves them with v_perm_b32.  The per-lane row stride is padded to an odd
//    number of 16-byte slots so the 16 lanes of a group hit 64 distinct banks.
//  * four groups per wave64, four waves per workgroup: 32 targets in flight per workgroup, all against
//    the same query (the prefilter list of one query, pre-sorted by target length so the groups of a
//    wave finish together).
//  * end positions: each lane keeps the packed running maximum of its strip, the column where it was
//    last raised and a snapshot of the strip's H values at that column (v_bfi under a rarely taken
//    branch); a 16-lane DPP/shuffle reduction at the end applies the reference's tie rules.
//  * queries longer than one tile loop over tiles inside the kernel; the H/F row leaving the last lane
//    is parked in a double-buffered global scratch line (lane 15 stores a column per step, under a scalar test) and
//    re-enters at the head lane of the next tile, loaded 16 columns at a time and rotated one lane per step.
//    Where the profiles of all tiles fit the workgroup's LDS (two tiles always, three up to R = 24 with 21 letters:
//    sw_multi_resident, mmgpu_internal.h) they are built once per job and the tile loop only moves the LDS base;
//    otherwise the one profile is rebuilt per tile, between two barriers.
//  * wide groups: a query of 16 * SW_MAX_R + 1 .. 32 * SW_MAX_R residues (449 .. 896) is not two tiles but ONE tile of a group of
//    32 lanes (two DPP rows, two groups and four pairs per wave64): lane g of 32 owns R = ceil(qlen / 32) rows, and the job is a
//    single-tile job - f16 forward scan, row prefetch, reverse scan in the workgroup, no scratch line, no slot, no tile loop.  The
//    hand-off crosses the row boundary with one more move per value, v_mov_b32_dpp wave_shr:1 row_mask:0xa bank_mask:0x1 behind the
//    row_shr:1 (lanes 16 - 19 and 48 - 51 are rewritten: lane 16 gets lane 15's value, the others what they had): 14 instead of 11
//    instructions beside the rows, still no LDS and no bpermute (profiles/sw_wide_isa_audit.txt).  Shape codes 64 + R - 1, served
//    by the grids of groups 1 and 2 by register need (sw_group_of, mmgpu_internal.h); MMGPU_SW_WIDE=0 in the environment restores the two tiles.
//
// Bytes per cell that ever touch HBM: (tlen + 28) / (qlen * tlen) ~ 0.003 - this kernel
// is bound by VALU issue, not by HBM.
#include "mmgpu_internal.h"
#include "pf_device.h"
#include "sw_body.h"   // sw_body and its steps, sw_passes, the job prologue and the shape dispatch: shared with sw_half_kernel.hip

namespace mmgpu {

namespace {

template <int G, bool BOTH>
__global__ __launch_bounds__(WAVES * 64)
__attribute__((amdgpu_waves_per_eu(sw_waves_floor(G, BOTH), sw_waves_cap(G, BOTH)))) void sw_kernel(SwLaunch L) {
    SwJob job = L.jobs[blockIdx.x];
    if (!sw_clip_job(L, job)) return;
    // multi-tile jobs (the last group only) run with a slot of the column-scratch pool
    const bool claims = G == SW_GROUPS - 1 && (job.shape & 0xFFu) >= SW_SHAPE_MULTI && (job.shape & 0xFFu) < SW_SHAPE_WIDE;
    if (claims) sw_claim_scratch(L, job);
    sw_dispatch_shape<G>(job.shape, [&](auto r, auto kind) __attribute__((always_inline)) {
        sw_passes<decltype(r)::value, decltype(kind)::value == SW_MULTI, BOTH, decltype(kind)::value == SW_WIDE ? 2 * GROUP : GROUP>(L, job);
    });
    if (claims) sw_release_scratch(L, job);
}

// Reverse scan of the multi-tile queries.  A forward job of a long query holds few hits (8 or 16 per workgroup for
// queries of 1024 residues or more, so that the batch has no long tail), of which one in six needs a reverse scan: done
// inside the forward job, one or two 16-lane groups of one wave worked while the workgroup held four waves' registers
// and a profile (measured: +19 ms on the 10k x 1M lists for 11 % of the pairs).  Here a job is up to SW_REV_JOB_HITS
// hits of one query - normally its whole list - whose live pairs are packed before they are dealt to the waves.
// Launched behind the group-2 kernel on the same stream (it reads that kernel's forward results).
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(SW_MIN_WAVES))) void sw_rev_multi_kernel(SwLaunch L) {
    SwJob job = L.jobs[blockIdx.x];
    if (!sw_clip_job(L, job)) return;
    sw_claim_scratch(L, job);
    sw_dispatch_shape<SW_GROUPS - 1>(job.shape, [&](auto r, auto kind) __attribute__((always_inline)) {
        if constexpr (decltype(kind)::value == SW_MULTI) sw_body<decltype(r)::value, true, true, false>(L, job);
    });
    sw_release_scratch(L, job);
}

// ---------------------------------------------------------------------------------------------------------
// Fused prefilter -> align hand-over: what mmgpu_sw_prepare does on the host for caller
// supplied lists, done on the device for the hit lists of a prefilter batch.  One workgroup per query: the list is
// sorted by target length (longest first, stable) so that the targets a wavefront runs together end together;
// hit_target / hit_out are written for the list's slots [q * stride, q * stride + count).
__global__ __launch_bounds__(256) void sw_from_pf_kernel(SwFromPfArgs A) {
    extern __shared__ uint32_t key[];      // next power of two >= the lists' stride (launch_sw_from_pf)
    const uint32_t q = blockIdx.x;
    unsigned long long *const stat = A.cells + (size_t)(blockIdx.x % (uint32_t)SW_FROM_PF_STAT_SLOTS) * 3;      // (cells, pairs, longest target)
    const uint32_t n = min(A.hit_count[q], A.stride);
    const mmgpu_pf_hit *hits = A.pf_hits + (size_t)q * A.pf_stride;
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    unsigned long long cells = 0;
    const uint32_t qlen = A.q_off[q + 1] - A.q_off[q];
    for (uint32_t k = threadIdx.x; k < np2; k += 256) {
        uint32_t v = 0xFFFFFFFFu;
        if (k < n) {
            const uint32_t len = A.t_len[hits[k].id];
            v = ((0xFFFFu - min(len, 0xFFFFu)) << 16) | k;      // length descending, list position ascending
            cells += (unsigned long long)qlen * len;
        }
        key[k] = v;
    }
    __syncthreads();
    const uint32_t base = q * A.stride;
    if (n <= 512) {
        // a list of --max-seqs 300: every element counts the keys below its own (the keys are distinct; all lanes read the same
        // word of LDS at a time) - one pass instead of the 45 barrier-separated steps of the network below
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            const uint32_t mine = key[i];
            uint32_t r = 0;
            for (uint32_t j = 0; j < n; j++) r += key[j] < mine ? 1u : 0u;
            A.hit_target[base + r] = hits[i].id;
            A.hit_out[base + r] = base + i;
            A.slot_target[base + i] = hits[i].id;
            if (r == 0) atomicMax(stat + 2, (unsigned long long)(0xFFFFu - (mine >> 16)));   // longest target of any list
        }
    } else {
    block_bitonic_sort<256>(np2, [&](uint32_t i, uint32_t j) { return key[i] > key[j]; }, [&](uint32_t i, uint32_t j) { exchange_at(key, i, j); });
    for (uint32_t r = threadIdx.x; r < n; r += 256) {
        const uint32_t k = key[r] & 0xFFFFu;
        A.hit_target[base + r] = hits[k].id;
        A.hit_out[base + r] = base + k;
        A.slot_target[base + r] = hits[r].id;
    }
    if (threadIdx.x == 0 && n) atomicMax(stat + 2, (unsigned long long)(0xFFFFu - (key[0] >> 16)));   // longest target of any list
    }
    for (uint32_t r = n + threadIdx.x; r < A.stride; r += 256) {   // unused slots: defined contents
        A.hit_target[base + r] = 0;
        A.hit_out[base + r] = base + r;
        A.slot_target[base + r] = 0;
    }
    if (threadIdx.x == 0) A.count_copy[q] = n;
    // statistics (cells = forward DP cells, Alignment.cpp:380,530 convention)
    wave_sum_to(stat, cells);
    if (threadIdx.x == 0 && n) atomicAdd(stat + 1, (unsigned long long)n);
}

}  // namespace

hipError_t launch_sw_from_pf(const SwFromPfArgs &A, uint32_t nq, hipStream_t stream) {
    // the kernel orders a list in np2 * 4 bytes of dynamic LDS: the longest list it is given must keep that within the 64 KB a
    // workgroup may ask for without the launch attribute that raises the ceiling
    static_assert((SW_PF_MAX_LIST & (SW_PF_MAX_LIST - 1)) == 0 && (size_t)SW_PF_MAX_LIST * sizeof(uint32_t) <= 65536,
                  "SW_PF_MAX_LIST: a power of two whose dwords fit 64 KB of dynamic LDS");
    if (A.stride > (uint32_t)SW_PF_MAX_LIST) return hipErrorInvalidValue;
    if (nq == 0) return hipSuccess;
    uint32_t np2 = 1;
    while (np2 < A.stride) np2 <<= 1;
    const size_t lds = (size_t)np2 * sizeof(uint32_t);
    if (lds > 65536) return hipErrorInvalidValue;      // (unreachable after the stride check; the kernel's LDS array must never be short)
    // strides 8193 - 16384 ask for the full 64 KB: say so to the runtime instead of relying on its default ceiling
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(sw_from_pf_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(sw_from_pf_kernel, dim3(nq), dim3(256), lds, stream, A);
    return hipGetLastError();
}

uint32_t sw_multi_resident_blocks(size_t lds_bytes, bool both_passes, int compute_units) {
    int per_cu = 0;
    const size_t lds = lds_bytes + SW_LDS_HEADER;
    hipError_t e = both_passes ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sw_kernel<SW_GROUPS - 1, true>, WAVES * 64, lds)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sw_kernel<SW_GROUPS - 1, false>, WAVES * 64, lds);
    if (e == hipSuccess && both_passes) {   // the reverse kernel of the multi-tile queries draws on the same pool
        int rev = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&rev, sw_rev_multi_kernel, WAVES * 64, lds) == hipSuccess) per_cu = std::max(per_cu, rev);
    }
    // a CU holds at most 32 wavefronts = 8 workgroups of 4; one more than the occupancy query says, as a margin
    if (e != hipSuccess || per_cu < 1) per_cu = 8;
    per_cu = per_cu + 1 > 8 ? 8 : per_cu + 1;
    return (uint32_t)per_cu * (uint32_t)(compute_units > 0 ? compute_units : 256);
}

hipError_t launch_sw_rev_multi(const SwLaunch &L, size_t lds_bytes, hipStream_t stream) {
    if (L.n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_rev_multi_kernel, dim3(L.n_jobs), dim3(WAVES * 64), lds_bytes + SW_LDS_HEADER, stream, L);
    return hipGetLastError();
}

// by register need (sw_group_of): the shape code is kind + R - 1
int sw_shape_group(uint32_t shape) {
    const uint32_t kind = shape >= SW_SHAPE_WIDE ? SW_SHAPE_WIDE : (shape >= SW_SHAPE_MULTI ? SW_SHAPE_MULTI : 0u);
    return sw_group_of(kind == SW_SHAPE_MULTI, (int)(shape - kind) + 1);
}

static bool env_switch(const char *name, bool unset) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) != 0 : unset;
}
bool sw_wide_enabled() {
    static const bool on = env_switch("MMGPU_SW_WIDE", true);
    return on;
}
bool sw_half_wide() {
    static const bool on = env_switch("MMGPU_SW_HALF_WIDE", true);
    return on;
}

// May this batch's single-tile forward scans run in f16 (sw_half_kernel.hip)?  The exactness rule of sw_body.h (at SW_HALF_LIMIT)
// assumes profile entries in [-256, 254] - true of every batch: they are sums of two int8, or int8 profile scores, whatever the
// alphabet - and gap costs that f16 holds exactly and whose subtraction from a value in [0, 2046] stays within +-2048:
// 0 <= gap_extend, gap_open <= 2048.  A launch that only runs reverse scans (rev_only) has no forward scan to gain from.
static bool sw_half_eligible(const SwLaunch &L) {
    return MMGPU_SW_HALF && !L.rev_only && L.gap_open >= 0 && L.gap_open <= SW_HALF_MAX_GAP && L.gap_extend >= 0 &&
           L.gap_extend <= SW_HALF_MAX_GAP;
}

hipError_t launch_sw(const SwLaunch &L, int group, size_t lds_bytes, bool both_passes, hipStream_t stream) {
    if (L.n_jobs == 0) return hipSuccess;
    if (sw_half_eligible(L) && launch_sw_half(L, group, lds_bytes, both_passes, stream)) return hipGetLastError();
    dim3 grid(L.n_jobs), block(WAVES * 64);
    const size_t lds = lds_bytes + SW_LDS_HEADER;
    switch (group * 2 + (both_passes ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((sw_kernel<0, false>), grid, block, lds, stream, L); break;
        case 1: hipLaunchKernelGGL((sw_kernel<0, true>), grid, block, lds, stream, L); break;
        case 2: hipLaunchKernelGGL((sw_kernel<1, false>), grid, block, lds, stream, L); break;
        case 3: hipLaunchKernelGGL((sw_kernel<1, true>), grid, block, lds, stream, L); break;
        case 4: hipLaunchKernelGGL((sw_kernel<2, false>), grid, block, lds, stream, L); break;
        case 5: hipLaunchKernelGGL((sw_kernel<2, true>), grid, block, lds, stream, L); break;
        case 6: hipLaunchKernelGGL((sw_kernel<SW_GROUPS - 1, false>), grid, block, lds, stream, L); break;      // (SW_GROUPS == 4 only)
        case 7: hipLaunchKernelGGL((sw_kernel<SW_GROUPS - 1, true>), grid, block, lds, stream, L); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// first use of any kernel of this file loads its code object (tens of milliseconds): mmgpu_warmup does it ahead of time
void warm_sw() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_rev_multi_kernel));
    if (MMGPU_SW_HALF) warm_sw_half();
}

}  // namespace mmgpu
