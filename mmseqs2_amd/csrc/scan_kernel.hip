// Exhaustive ungapped scan for gfx950 / CDNA4: the best ungapped diagonal score of every query against every resident target
// (SmithWaterman::ungapped_alignment, src/alignment/StripedSmithWaterman.cpp:1817-1876, behind runFilterOnCpu of
// src/prefiltering/ungappedprefilter.cpp:346-482), and the selection of each query's list out of the score bytes.
//
// What it computes, per pair:   U(i, j) = max(0, sat16(U(i-1, j-1) + p(i, t[j]))),   score = min(255 - B, max U)
// with p(i, x) = mat[x][q[i]] + comp_bias[i] for a sequence query and p(i, x) = prof[x][i] (x < profile_letters, else 0) for a
// profile query (B then comes from the profile alone; scan_api.hip).  The reference clamps every cell at 255 - B (unsigned bytes,
// adds then subs of the bias B); the capped and the uncapped recurrence agree until the cap first bites, and from there the capped
// maximum IS the cap, so one min at the end gives the same number.
//
// How it is mapped (sw_kernel.hip's mapping where it serves):
//  * packed 2 x int16: the low half of every register belongs to target A, the high half to target B of a pair taken from the
//    length-sorted id list; a group of 16 lanes (one DPP row) owns one pair, lane g owns R consecutive query rows.
//  * a cell depends on its diagonal neighbour only, so the lanes are NOT skewed: all 16 lanes work on the same column.  A register
//    follows one diagonal: in column c + 1 it stands one row lower.  Over a chunk of R columns (fully unrolled) the register that
//    leaves the strip's last row re-enters at row 0 with the value of the lane above - one v_mov_b32_dpp row_shr:1 per column -
//    and no register is ever moved.  Per row pair: v_perm_b32 (interleave the two letters' profile rows), v_pk_add_i16 clamp,
//    v_pk_max_i16 with 0, v_pk_max_i16 into the running maximum.
//  * the query profile P[letter][row] (int16, composition bias folded in, 0 for the rows past the query and for the pad letter)
//    is built once per workgroup in LDS in sw_kernel.hip's layout (odd number of 16-byte slots per lane).  A profile query's rows
//    are copied from its own int8 table instead; from there on the two kinds of query run the same code.
//  * four rows per wave64, four waves per workgroup: 32 targets per round, SCAN_JOB_TARGETS per job.  Target letters are read
//    a chunk ahead, four per dword; words past a target's end read as the pad letter, whose profile row is 0.
//  * queries longer than one tile (512 rows): the tile loop runs inside the kernel; the value leaving the last lane is parked in a
//    double-buffered global line per DPP row and re-enters at lane 0 of the next tile.  The profile is rebuilt per tile.
//  * the finished pair's score goes into the batch's [query][target] byte array with plain byte stores; the selection kernel
//    (one workgroup per query) builds a 256-bin histogram of the admitted targets' keys 255 - score and finds the cut key in it;
//    compaction, sort and the write of the list are select_device.h's, shared with gscan_kernel.hip.  The histogram's atomics only
//    count.
#include "mmgpu_internal.h"
#include "select_device.h"

namespace mmgpu {

namespace {

constexpr int GROUP = 16;            // lanes per target pair (one DPP row)
constexpr int WAVES = 4;             // waves per workgroup
static_assert(SCAN_ROUND == WAVES * (64 / GROUP) * 2, "targets per workgroup round");

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk_add_sat(unsigned a, unsigned b) {   // v_pk_add_i16 ... clamp
    return __builtin_bit_cast(unsigned, __builtin_elementwise_add_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned pk_max_s(unsigned a, unsigned b) {     // v_pk_max_i16
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

template <int R>
struct Tile {
    static constexpr int ROWS = GROUP * R;
    static constexpr int LANE_STRIDE = lane_stride_bytes(R);
    static constexpr int ROW_STRIDE = GROUP * LANE_STRIDE;   // bytes per letter
};

// where a job's profile rows come from: a sequence query (prof == nullptr) or a profile query's own table
struct ScanSource {
    const uint8_t *q;
    const int8_t *cb;
    const int8_t *prof;      // [prof_letters][qlen], letter-major
    int prof_letters;
    int qlen;
};

__device__ __forceinline__ ScanSource scan_source(const ScanLaunch &L, uint32_t query) {
    const uint32_t qo = L.q_off[query];
    const uint64_t po = L.q_prof_off[query];
    ScanSource S;
    S.q = L.q_res + qo;
    S.cb = L.q_cb + qo;
    S.prof = po == SCAN_NO_PROFILE ? nullptr : L.q_prof + po;
    S.prof_letters = (int)L.q_prof_letters[query];
    S.qlen = (int)(L.q_off[query + 1] - qo);
    return S;
}

// P[letter][row] for rows [tile_base, tile_base + ROWS): 0 past the query's end and for the pad letter `alphabet`; for a profile
// query also for the letters it has no row for.  Consecutive threads take consecutive rows of one letter, so a profile query's reads
// are contiguous bytes; the source is the job's, hence uniform over the workgroup.
template <int R>
__device__ __forceinline__ void build_profile(unsigned char *lds, const ScanSource &S, int tile_base, const int8_t *mat, int alphabet) {
    using T = Tile<R>;
    const int total = (alphabet + 1) * T::ROWS;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int letter = idx / T::ROWS;
        const int row = idx - letter * T::ROWS;
        const int rg = tile_base + row;
        short v = 0;
        if (S.prof) {
            if (letter < S.prof_letters && rg < S.qlen) v = (short)S.prof[(size_t)letter * (size_t)S.qlen + (size_t)rg];
        } else if (letter < alphabet && rg < S.qlen) {
            v = (short)((int)mat[letter * alphabet + S.q[rg]] + (int)S.cb[rg]);
        }
        const int lane = row / R, r = row - lane * R;
        *reinterpret_cast<short *>(lds + letter * T::ROW_STRIDE + lane * T::LANE_STRIDE + r * 2) = v;
    }
}

// R columns of one pair: wA / wB hold the chunk's letters (four per dword), H[d] the diagonals the lane's strip holds.  In column
// k of the chunk register d stands in row (d + k) % R of the strip.
template <int R, bool MULTI>
__device__ __forceinline__ void scan_chunk(unsigned (&H)[R], unsigned &vmax, const unsigned char *prof_lane, const unsigned (&wA)[R / 4],
                                           const unsigned (&wB)[R / 4], const unsigned (&inc)[(R + 15) / 16], unsigned (&outv)[(R + 15) / 16], int l16) {
    using T = Tile<R>;
#pragma unroll
    for (int k = 0; k < R; k++) {
        const unsigned la = __builtin_amdgcn_ubfe(wA[k / 4], (unsigned)(k & 3) * 8u, 8u);
        const unsigned lb = __builtin_amdgcn_ubfe(wB[k / 4], (unsigned)(k & 3) * 8u, 8u);
        const uint4 *pa = reinterpret_cast<const uint4 *>(prof_lane + la * T::ROW_STRIDE);
        const uint4 *pb = reinterpret_cast<const uint4 *>(prof_lane + lb * T::ROW_STRIDE);
        unsigned pav[R / 2], pbv[R / 2];
#pragma unroll
        for (int v = 0; v < R / 8; v++) {
            const uint4 a = pa[v], b = pb[v];
            pav[4 * v] = a.x; pav[4 * v + 1] = a.y; pav[4 * v + 2] = a.z; pav[4 * v + 3] = a.w;
            pbv[4 * v] = b.x; pbv[4 * v + 1] = b.y; pbv[4 * v + 2] = b.z; pbv[4 * v + 3] = b.w;
        }
        // the register that left the last row of the strip above enters row 0: lane 0 of the row takes the tile's incoming value
        const int d0 = (R - k) % R;
        // (multi-tile: lane k % 16 of the row fetched the value for column k of the chunk)
        const unsigned head = MULTI ? (unsigned)__shfl((int)inc[k / 16], k % 16, GROUP) : 0u;
        H[d0] = __builtin_amdgcn_update_dpp(head, H[d0], 0x111 /*row_shr:1*/, 0xF, 0xF, false);
#pragma unroll
        for (int d = 0; d < R; d++) {
            const int r = (d + k) % R;
            const unsigned P = __builtin_amdgcn_perm(pbv[r / 2], pav[r / 2], (r & 1) ? 0x07060302u : 0x05040100u);
            H[d] = pk_max_s(pk_add_sat(H[d], P), 0u);
            vmax = pk_max_s(vmax, H[d]);
        }
        if (MULTI) {
            // the strip's last row of the tile's last lane: what the next tile's lane 0 adds to in the next column; lane k % 16 keeps
            // it, so that the row stores a chunk's values with one coalesced store per 16 columns
            const unsigned leaving = (unsigned)__shfl((int)H[R - 1 - k], GROUP - 1, GROUP);
            if (l16 == k % 16) outv[k / 16] = leaving;
        }
    }
}

// the chunk's letters of one target: words past its end (and every word of an absent target, len 0) read as the pad letter
template <int R>
__device__ __forceinline__ void load_words(unsigned (&w)[R / 4], const uint32_t *t, uint32_t len, uint32_t c0, unsigned padw) {
#pragma unroll
    for (int j = 0; j < R / 4; j++) {
        const uint32_t ci = c0 / 4u + (uint32_t)j;
        const bool in = ci * 4u < len;
        const unsigned v = t[in ? ci : 0u];
        w[j] = in ? v : padw;
    }
}

template <int R, bool MULTI>
__global__ __launch_bounds__(WAVES * 64) void scan_kernel(ScanLaunch L) {
    using T = Tile<R>;
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l16 = lane & 15, grp = lane >> 4;
    const unsigned padw = (unsigned)L.alphabet * 0x01010101u;
    const uint32_t *t_words = reinterpret_cast<const uint32_t *>(L.t_res);
    const unsigned char *prof_lane = scan_lds + l16 * T::LANE_STRIDE;

    for (uint32_t job = blockIdx.x; job < L.n_jobs; job += gridDim.x) {
        const ScanJob J = L.jobs[job];
        const ScanSource S = scan_source(L, J.query);
        const int qlen = S.qlen;
        const int cap = L.q_cap[J.query];
        const int n_tiles = MULTI ? (qlen + T::ROWS - 1) / T::ROWS : 1;
        if (!MULTI) {
            __syncthreads();
            build_profile<R>(scan_lds, S, 0, L.mat, L.alphabet);
            __syncthreads();
        }
        // multi-tile: this DPP row's two boundary lines in the workgroup's slot (the slot was sized for its longest job)
        uint32_t *park = nullptr;
        uint32_t park_half = 0;
        if (MULTI) {
            const uint32_t row_words = scan_park_row_words(L.t_len[L.order[J.begin]]);
            park = L.park + L.park_off[blockIdx.x] + (size_t)(wave * 4 + grp) * row_words;
            park_half = row_words / 2u;
        }
        for (uint32_t round = J.begin; round < J.end; round += SCAN_ROUND) {
            const uint32_t wave_first = round + (uint32_t)wave * 8u;
            const uint32_t pos = wave_first + (uint32_t)grp * 2u;
            const bool validA = pos < J.end, validB = pos + 1u < J.end;
            const uint32_t idA = validA ? L.order[pos] : 0u;
            const uint32_t idB = validB ? L.order[pos + 1u] : idA;
            const uint32_t lenA = validA ? L.t_len[idA] : 0u;
            const uint32_t lenB = validB ? L.t_len[idB] : 0u;
            const uint32_t *tA = t_words + L.t_off4[idA];
            const uint32_t *tB = t_words + L.t_off4[idB];
            // the wave's first target is its longest (the list is sorted longest first): one column count for the four rows
            uint32_t ncols = wave_first < J.end ? scan_cols(L.t_len[L.order[wave_first]], R) : 0u;
            ncols = __builtin_amdgcn_readfirstlane(ncols);
            unsigned vmax = 0;
            for (int tile = 0; tile < n_tiles; tile++) {
                if (MULTI) {
                    __syncthreads();
                    build_profile<R>(scan_lds, S, tile * T::ROWS, L.mat, L.alphabet);
                    __syncthreads();
                }
                uint32_t *park_out = MULTI ? park + (uint32_t)(tile & 1) * park_half : nullptr;
                const uint32_t *park_in = MULTI ? park + (uint32_t)((tile & 1) ^ 1) * park_half : nullptr;
                unsigned H[R];
#pragma unroll
                for (int d = 0; d < R; d++) H[d] = 0;
                unsigned wA[R / 4], wB[R / 4], nA[R / 4], nB[R / 4];
                load_words<R>(wA, tA, lenA, 0, padw);
                load_words<R>(wB, tB, lenB, 0, padw);
                for (uint32_t c0 = 0; c0 < ncols; c0 += R) {
                    load_words<R>(nA, tA, lenA, c0 + R, padw);      // (a chunk ahead; past the end it reads word 0 and keeps the pad)
                    load_words<R>(nB, tB, lenB, c0 + R, padw);
                    // multi-tile: entry c of a boundary line is what column c's row 0 adds to (entry 0: nothing, the matrix's edge)
                    unsigned inc[(R + 15) / 16], outv[(R + 15) / 16];
#pragma unroll
                    for (int j = 0; j < (R + 15) / 16; j++) {
                        const uint32_t col = c0 + 16u * (uint32_t)j + (uint32_t)l16;
                        inc[j] = (MULTI && tile > 0 && col > 0u) ? park_in[col] : 0u;
                        outv[j] = 0;
                    }
                    scan_chunk<R, MULTI>(H, vmax, prof_lane, wA, wB, inc, outv, l16);
                    if (MULTI) {
#pragma unroll
                        for (int j = 0; j < (R + 15) / 16; j++) park_out[c0 + 1u + 16u * (uint32_t)j + (uint32_t)l16] = outv[j];
                    }
#pragma unroll
                    for (int j = 0; j < R / 4; j++) { wA[j] = nA[j]; wB[j] = nB[j]; }
                }
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) vmax = pk_max_s(vmax, (unsigned)__shfl_xor((int)vmax, off, GROUP));
            if (l16 == 0) {
                const int sa = min(cap, (int)(vmax & 0xFFFFu)), sb = min(cap, (int)(vmax >> 16));
                uint8_t *row = L.scores + (size_t)J.query * L.n_targets;
                if (validA) row[idA] = (uint8_t)sa;
                if (validB) row[idB] = (uint8_t)sb;
            }
        }
    }
}

// One workgroup per query: the list out of the score bytes.  Keys are 255 - score; one histogram level finds the cut.
__global__ __launch_bounds__(SELECT_THREADS) void scan_select_kernel(ScanSelectArgs A) {
    __shared__ unsigned hist[SELECT_BINS];
    __shared__ SelectLds lds;
    __shared__ unsigned s_cut, s_need;
    const uint32_t q = blockIdx.x;
    const unsigned tid = threadIdx.x;
    const uint32_t n = A.n_targets;
    const uint8_t *scores = A.scores + (size_t)q * n;
    const uint32_t ident = A.q_ident[q], lo = A.q_win[2 * q], hi = A.q_win[2 * q + 1];
    if (tid < SELECT_BINS) hist[tid] = 0;
    __syncthreads();
    // admitted: inside the window, and above the threshold or the query's own target
    auto key_of = [&](uint64_t i, unsigned &k) {
        const int s = scores[i];
        const uint32_t len = A.t_len[i];
        k = (unsigned)(255 - s);
        return len >= lo && len <= hi && (s > A.min_score || (uint32_t)i == ident);
    };
    for (uint64_t i = tid; i < n; i += SELECT_THREADS) {
        unsigned k;
        if (key_of(i, k)) atomicAdd(&hist[k], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int b = 0; b < SELECT_BINS; b++) total += hist[b];
        unsigned cut = SELECT_BINS, need = 0;      // no cut: every admitted key is below it
        if (total > A.max_hits) {      // the class the cut falls into, and how many of its lowest ids are kept
            const SelectCut c = select_cut_walk(hist, 0, A.max_hits);
            cut = c.bin;
            need = A.max_hits - c.above;
        }
        s_cut = cut;
        s_need = need;
    }
    __syncthreads();
    select_emit(n, key_of, s_cut, s_need, lds, 255, A.hits + (size_t)q * A.stride, A.stride, &A.counts[q]);
}

}  // namespace

hipError_t launch_scan(const ScanLaunch &L, int cls, uint32_t grid, hipStream_t stream) {
    if (L.n_jobs == 0 || grid == 0) return hipSuccess;
    const size_t lds = sw_profile_bytes(scan_class_rows(cls), L.alphabet);
    if (lds > 65536) return hipErrorInvalidValue;
    const dim3 g(grid), block(WAVES * 64);
    switch (cls) {
        case 0: hipLaunchKernelGGL((scan_kernel<8, false>), g, block, lds, stream, L); break;
        case 1: hipLaunchKernelGGL((scan_kernel<16, false>), g, block, lds, stream, L); break;
        case 2: hipLaunchKernelGGL((scan_kernel<24, false>), g, block, lds, stream, L); break;
        case 3: hipLaunchKernelGGL((scan_kernel<32, false>), g, block, lds, stream, L); break;
        case SCAN_MULTI: hipLaunchKernelGGL((scan_kernel<SCAN_MAX_R, true>), g, block, lds, stream, L); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_select(const ScanSelectArgs &A, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (A.max_hits > (uint32_t)SELECT_MAX_HITS) return hipErrorInvalidValue;      // the key array must never be short
    hipLaunchKernelGGL(scan_select_kernel, dim3(nq), dim3(SELECT_THREADS), 0, stream, A);
    return hipGetLastError();
}

void warm_scan() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&scan_select_kernel));
}

}  // namespace mmgpu
