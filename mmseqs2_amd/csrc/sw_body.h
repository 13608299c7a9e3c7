// The Smith-Waterman column loop and what it needs, shared by the kernels of sw_kernel.hip (packed int16) and of
// sw_half_kernel.hip (packed f16 first pass of the single-tile forward scan).  How the scan is mapped to the chip is
// described at the top of sw_kernel.hip; the f16 arithmetic and its exactness rule below, at SW_HALF_LIMIT.
#pragma once
#include "mmgpu_internal.h"
#include "pf_device.h"

namespace mmgpu {

namespace {

constexpr int GROUP = 16;            // lanes per target pair (one DPP row); the wide bodies (W = 32) give a pair two rows
constexpr int WAVES = 4;             // waves per workgroup
constexpr int GROUPS_PER_WAVE = 64 / GROUP;
constexpr int HITS_PER_WAVE = 2 * GROUPS_PER_WAVE;   // two targets per group (lo/hi halves); 2 * 64 / W in a body of W-lane groups
constexpr unsigned NEG2 = 0x80008000u;               // packed (-32768, -32768)

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk_add_sat(unsigned a, unsigned b) {   // v_pk_add_i16 ... clamp
    return __builtin_bit_cast(unsigned, __builtin_elementwise_add_sat(__builtin_bit_cast(s16x2, a),
                                                                      __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned pk_max_s(unsigned a, unsigned b) {     // v_pk_max_i16
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a),
                                                                  __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned pk_max_u(unsigned a, unsigned b) {     // v_pk_max_u16
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned pk_sub_sat_u(unsigned a, unsigned b) { // v_pk_sub_u16 ... clamp
    return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a),
                                                                      __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned bfi(unsigned mask, unsigned a, unsigned b) {   // v_bfi_b32
    return (a & mask) | (b & ~mask);
}

// ---- packed 2 x f16 cell arithmetic (sw_body<.., HALF = true>: the first pass of sw_half_kernel.hip) -------------------------
// gfx950 has a packed three-way maximum for f16 (v_pk_maximum3_f16) and none for int16, and the recurrence is three pairs of maxima:
//     H = max3(Hd + P, E, F);  E' = max3(E - ge, H - go, 0);  F' = max3(F - ge, H - go, 0);  cmax = max3(cmax, H[r], H[r + 1])
// - 8.5 packed ops and a v_perm per row of two cells instead of 10.  All of them issue at the rate of the int16 ops
// (profiles/sw_half_valu_rate_probe.txt).  Plain C++ on _Float16 vectors: the compiler selects v_pk_maximum3_f16 (with the inline
// constant 0) and v_pk_add_f16 with neg_lo / neg_hi for the subtractions; no asm, whose boundaries cost the column loop wait states.
//
// Exactness.  A profile entry is an int8 matrix entry plus an int8 composition bias, or an int8 profile score: it lies in
// [-256, 254], or is -32768 (rows past the query end, the padding letter), and f16 holds all of these exactly.  f16 holds every
// integer of magnitude <= 2048 exactly.  While the running maximum of a pair is at most SW_HALF_LIMIT = 2048 - 256, every H, E and F
// of the columns done so far lies in [0, 1792], so in the next column Hd + P lies in [-256, 2046] (or is negative: P = -32768,
// whose rounded sum never survives the maximum with E, F >= 0), H in [0, 2046], H - go and E - ge in [-2048, 2046] (the kernel is
// used for 0 <= ge, go <= 2048 only, sw_half_eligible): every intermediate is an integer f16 holds, every operation is exact, and the
// column equals the int16 column value for value.  So the first column whose maximum exceeds the limit is itself exact, and the
// running maximum never falls: "final maximum > SW_HALF_LIMIT" is decided identically by the f16 and the int16 recurrence.  A pair
// with that flag is scanned again in int16 by the same workgroup (MARKED); every other pair's result is the int16 result.
// Past the limit values may round, and beyond 65504 become +inf; nothing here subtracts two infinities, so no NaN arises,
// and x + (-x) is +0 in round-to-nearest: no -0 either.  Non-negative f16 values order like their bit patterns and equal values
// have equal bits, so the bookkeeping on bit patterns (running maximum, snapshot compare, the 16-lane fold) is shared with int16.
constexpr int SW_HALF_LIMIT = 2048 - 256;
constexpr int SW_HALF_MAX_GAP = 2048;
constexpr int SW_HALF_MARK = -1;     // score field of a pair the f16 pass leaves to the int16 pass (no finished result holds it)
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h16x2 as_h(unsigned a) { return __builtin_bit_cast(h16x2, a); }
__device__ __forceinline__ unsigned as_u(h16x2 a) { return __builtin_bit_cast(unsigned, a); }
__device__ __forceinline__ unsigned h_add(unsigned a, unsigned b) { return as_u(as_h(a) + as_h(b)); }   // v_pk_add_f16
__device__ __forceinline__ unsigned h_sub(unsigned a, unsigned b) { return as_u(as_h(a) - as_h(b)); }   // v_pk_add_f16 neg_lo neg_hi
__device__ __forceinline__ unsigned h_max(unsigned a, unsigned b) {
    return as_u(__builtin_elementwise_maximum(as_h(a), as_h(b)));
}
__device__ __forceinline__ unsigned h_max3(unsigned a, unsigned b, unsigned c) {                         // v_pk_maximum3_f16
    return as_u(__builtin_elementwise_maximum(__builtin_elementwise_maximum(as_h(a), as_h(b)), as_h(c)));
}
__device__ __forceinline__ unsigned short h_bits(int v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
__device__ __forceinline__ int h_value(unsigned bits) { return (int)(float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
// A group of W = 32 lanes is two DPP rows, and row_shr stops at the row boundary: a second move, wave_shr:1 restricted to the
// first bank of the odd rows (row_mask 0xA, bank_mask 0x1: lanes 16 - 19 and 48 - 51), gives lane 16 of the group the value of lane
// 15 - lanes 17 - 19 get once more what row_shr gave them, the group's head lane (0, 32) keeps what the first move left there.
// One VALU op more per hand-off, no LDS, no bpermute.
template <int W>
__device__ __forceinline__ unsigned across_rows(unsigned x, unsigned v) {
    static_assert(W == 16 || W == 32, "groups of one or two DPP rows");
    if constexpr (W == 32) x = __builtin_amdgcn_update_dpp(x, v, 0x138 /*wave_shr:1*/, 0xA, 0x1, false);
    return x;
}
// value of the lane one below inside the W-lane group; lane 0 of each group keeps `head`
template <int W = GROUP>
__device__ __forceinline__ unsigned from_lane_above(unsigned head, unsigned v) {
    return across_rows<W>(__builtin_amdgcn_update_dpp(head, v, 0x111 /*row_shr:1*/, 0xF, 0xF, false), v);
}
// ... lane 0 of each group gets 0 (bound_ctrl): no register has to hold the zero
template <int W = GROUP>
__device__ __forceinline__ unsigned from_lane_above_or_zero(unsigned v) {
    return across_rows<W>(__builtin_amdgcn_update_dpp(0u, v, 0x111 /*row_shr:1*/, 0xF, 0xF, true), v);
}

// Build knob for A/B measurements (no test builds with 0; the default is what the suite and the bench run):
// MMGPU_SW_PREFETCH=0 fetches the profile rows in the column that uses them, as before the prefetch.
#ifndef MMGPU_SW_PREFETCH
#define MMGPU_SW_PREFETCH 1
#endif
// Empty asm that takes a value in and out of a VGPR: the instruction producing it has to stand where the source has it.
// Used on the E update in phase 2 of the column loop - see there.
#define SW_KEEP_IN_ROW(x) asm volatile("" : "+v"(x))

// (lane_stride_bytes and the size of a tile's profile: mmgpu_internal.h, shared with the host's LDS sizing)
template <int R, int W = GROUP>
struct Tile {
    static constexpr int ROWS = W * R;
    static constexpr int LANE_STRIDE = lane_stride_bytes(R);
    static constexpr int ROW_STRIDE = W * LANE_STRIDE;   // bytes per letter
};
static_assert(GROUP == 16, "sw_profile_bytes' default and sw_tiles (mmgpu_internal.h) assume 16-lane groups for all but the wide shapes");

// Build P[letter][row] for rows [tile_base, tile_base + ROWS) of the query (or of the reversed query).
// Rows past the query end and the extra letter `alphabet` (padding column of a finished target) are
// -32768, which keeps H at max(E, F) there and can never raise a running maximum.  HALF: the same values as f16.
template <int R, bool REV, bool HALF = false, int W = GROUP>
__device__ __forceinline__ void build_profile(unsigned char *lds, const uint8_t *q, const int8_t *cb, int qlen,
                                              int tile_base, const int8_t *mat, int alphabet, const int8_t *prof) {
    using T = Tile<R, W>;
    const int total = (alphabet + 1) * T::ROWS;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int letter = idx / T::ROWS;
        const int row = idx - letter * T::ROWS;
        const int rg = tile_base + row;
        short v = (short)-32768;
        if (letter < alphabet && rg < qlen) {
            const int qi = REV ? (qlen - 1 - rg) : rg;
            // profile query: the score row of the letter (createQueryProfile<PROFILE>, StripedSmithWaterman.cpp:773-776)
            v = prof ? (short)prof[letter * qlen + qi] : (short)((int)mat[letter * alphabet + q[qi]] + (int)cb[qi]);
        }
        const int lane = row / R, r = row - lane * R;
        if constexpr (HALF) v = (short)h_bits(v);
        *reinterpret_cast<short *>(lds + letter * T::ROW_STRIDE + lane * T::LANE_STRIDE + r * 2) = v;
    }
}

// Does the pair whose forward result sits in out[slot] get a reverse scan?  ssw_align_private scans backwards for the start
// position when the score passes the E-value gate (StripedSmithWaterman.cpp:857-863) - and, in the reference's alignment modes with a
// start position, only for hits of the uint8 pass: an int16-range hit (word == 1) takes its start from the block aligner (:865-882),
// falling back to the reverse scan when that declines (rev_mode 2: the caller names those pairs afterwards).
__device__ __forceinline__ bool sw_rev_wanted(const SwLaunch &L, uint32_t slot, int min_start) {
    const mmgpu_sw_hit &f = L.out[slot];
    const int s = f.score;
    if (L.rev_mode == 2) return s > 0 && L.rev_force[slot] != 0;
    return s > 0 && s >= min_start && !(L.rev_mode == 1 && f.word != 0);
}

constexpr int SW_REV_JOB_HITS = 1024;   // most hits a reverse-scan job may hold (mmgpu_internal.h: SW_REV_JOB_MAX)
static_assert(SW_REV_JOB_HITS == SW_REV_JOB_MAX, "host and kernel disagree on the reverse job size");
// dynamic LDS of an alignment workgroup: a 1 KB header (job-local scheduling state) followed by the query profiles of the tiles held
struct SwLds {
    uint16_t live[SW_REV_JOB_HITS];   // packed live hits (reverse pass, MARKED)
    uint32_t live_wave[WAVES];
    uint32_t next_chunk;              // next 8-hit chunk to hand to a wave
    uint32_t half_flag;               // HALF: some pair of the job is marked
    uint32_t unused[10];
    __device__ unsigned char *profiles() { return reinterpret_cast<unsigned char *>(this + 1); }   // (as many bytes as the launch asked for)
};
constexpr int SW_HALF_FLAG_AT = offsetof(SwLds, half_flag);   // byte offset in the header of the f16 pass's "some pair is marked" word
static_assert(SW_LDS_HEADER == SW_REV_JOB_HITS * 2 + 64 && sizeof(SwLds) == SW_LDS_HEADER && SW_HALF_FLAG_AT == SW_REV_JOB_HITS * 2 + 20 &&
              offsetof(SwLds, next_chunk) == SW_REV_JOB_HITS * 2 + 16, "the header holds the live hits and the scheduling words");
// (every `extern __shared__` array of a kernel is the one dynamic LDS block: this is sw_body's header)
__device__ __forceinline__ SwLds &sw_lds() {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
    return *reinterpret_cast<SwLds *>(lds_all);
}
__device__ __forceinline__ uint32_t sw_half_any_marked() { return sw_lds().half_flag; }

// the query of a job
struct SwQuery {
    const uint8_t *q;
    const int8_t *cb;
    int qlen, qbias;
    const int8_t *prof;   // profile query: its score rows, else nullptr
};
__device__ __forceinline__ SwQuery sw_query(const SwLaunch &L, uint32_t query) {
    const uint32_t qbeg = L.q_off[query];
    SwQuery Q;
    Q.qlen = (int)(L.q_off[query + 1] - qbeg);
    Q.q = L.q_res + qbeg;
    Q.cb = L.q_cb + qbeg;
    Q.qbias = L.q_bias[query];
    Q.prof = nullptr;
    if (L.q_prof_off) {
        const uint32_t po = L.q_prof_off[query];
        if (po != 0xFFFFFFFFu) Q.prof = L.q_prof + po;
    }
    return Q;
}

// The profiles a job holds, and when which is built.  A single-tile job has the one.  A multi-tile job whose tiles all fit the LDS
// the host granted by the same rule (sw_multi_resident) keeps every tile's profile: built once, in front of the chunk loop, which
// then runs without a barrier - its wavefronts take chunks as they finish, like the single-tile bodies.  The other jobs rebuild
// the one profile they have room for per tile and round.  (workgroup-uniform)
struct SwProfiles {
    unsigned char *lds;    // where the profiles start (behind the header)
    int n_tiles;
    uint32_t tile_bytes;
    bool resident;         // MULTI: all tiles held
    bool dynamic;          // all profiles held: chunks handed out through next_chunk, no barrier in the loop
};
template <int R, bool MULTI>
__device__ __forceinline__ SwProfiles sw_profiles(const SwLaunch &L, int qlen) {
    SwProfiles P;
    P.lds = sw_lds().profiles();
    P.n_tiles = MULTI ? (int)sw_tiles((uint32_t)qlen, R) : 1;
    P.tile_bytes = sw_profile_bytes(R, L.alphabet);
    P.resident = MULTI && sw_multi_resident((uint32_t)P.n_tiles, R, L.alphabet, L.resident_lds);
    P.dynamic = !MULTI || P.resident;
    return P;
}
enum SwBuildAt { SW_AT_JOB_START, SW_AT_PACKED, SW_AT_TILE };
// The one place profiles are built from.  A job that holds all its profiles builds them once, all threads, a barrier behind them: at
// the start of the job, or (PACKED: the reverse scan and the re-run of the marked pairs) behind the packing, which may leave nothing
// to scan.  The other jobs build the profile of `tile` at the top of that tile, between two barriers.
template <SwBuildAt AT, int R, bool REV, bool HALF, bool PACKED, int W>
__device__ __forceinline__ void sw_build_profiles(const SwLaunch &L, const SwQuery &Q, const SwProfiles &P, int tile = 0) {
    using T = Tile<R, W>;
    if (AT == SW_AT_TILE) {
        if (!P.dynamic) {
            __syncthreads();   // everyone is done reading the previous tile's profile
            build_profile<R, REV, HALF, W>(P.lds, Q.q, Q.cb, Q.qlen, tile * T::ROWS, L.mat, L.alphabet, Q.prof);
            __syncthreads();
        }
    } else if ((AT == SW_AT_PACKED) == PACKED && P.dynamic) {
        for (int t = 0; t < P.n_tiles; ++t)
            build_profile<R, REV, HALF, W>(P.lds + (uint32_t)t * P.tile_bytes, Q.q, Q.cb, Q.qlen, t * T::ROWS, L.mat, L.alphabet, Q.prof);
        __syncthreads();
    }
}

// Reverse pass: only the pairs whose forward score reaches the query's start-score threshold are scanned
// (ssw_align_private, StripedSmithWaterman.cpp:857-863) - typically one hit in six, scattered over the
// length-sorted list.  They are packed to the front (order kept), so that the waves run full instead of every
// wave waiting for its one or two live targets.
// MARKED packs the pairs the f16 pass marked in the same way (their int16 profile replaces the f16 one: the caller's barrier
// stands between the last read of that and this).
// Returns how many pairs `live` lists.
template <bool REV, bool MARKED>
__device__ __forceinline__ uint32_t sw_pack_live(const SwLaunch &L, const SwJob &job, SwLds &H, uint32_t n_hits) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int min_start = REV ? L.q_minstart[job.query] : 0;
    uint32_t total = 0;
    for (uint32_t base = 0; base < n_hits; base += WAVES * 64) {   // a job of the BOTH kernels holds at most 256 hits: one round
        const uint32_t idx = base + threadIdx.x;
        bool pass = false;
        if (idx < n_hits) {
            const uint32_t slot = L.hit_out[job.hit_begin + idx];
            pass = MARKED ? L.out[slot].score == SW_HALF_MARK : sw_rev_wanted(L, slot, min_start);
        }
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) H.live_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, round_total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = H.live_wave[w];
            before += w < wave ? c : 0u;
            round_total += c;
        }
        if (pass) H.live[total + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)idx;
        total += round_total;
        __syncthreads();
    }
    return total;
}

// Single-tile and resident jobs: a wave takes the next chunk of 8 hits (4 in a wide body) when it is done with its last one (the hits
// are sorted by length, so fixed wave <-> chunk striping would give wave 0 the longest chunk of every round).
// The other multi-tile jobs rebuild the profile per tile with all threads, so their waves stay in step.
// Returns the first slot of the wavefront's chunk in round `it` (wave-uniform).
template <int W>
__device__ __forceinline__ uint32_t sw_claim_chunk(SwLds &H, bool dynamic, uint32_t it) {
    constexpr int HITS_PER_WAVE = 2 * 64 / W;   // (W = 16: the file's constant)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t chunk = it * WAVES + wave;
    if (dynamic) {
        if (lane == 0) chunk = atomicAdd(&H.next_chunk, 1u);
        chunk = __builtin_amdgcn_readfirstlane(chunk);
    }
    return chunk * HITS_PER_WAVE;
}

// ---- write the result of one pair (its group's head lane) ----
// end, cols: the pair's forward t_end and its columns (REV)
template <bool REV, bool HALF>
__device__ __forceinline__ void sw_write_result(const SwLaunch &L, const SwQuery &Q, unsigned long long key, uint32_t h, int end, int cols) {
    // HALF: the key holds the score's f16 bits (ordered like the value); past the limit the pair is left to the int16 pass
    const bool marked = HALF && (unsigned)(key >> 32) > (unsigned)h_bits(SW_HALF_LIMIT);
    const int score = HALF ? (marked ? SW_HALF_MARK : h_value((unsigned)(key >> 32))) : (int)(key >> 32);
    const int col = 0xFFFF - (int)((key >> 16) & 0xFFFFu);
    const int row = 0xFFFF - (int)(key & 0xFFFFu);
    mmgpu_sw_hit *o = L.out + L.hit_out[h];
    if (!REV) {
        mmgpu_sw_hit res;
        res.score = score;
        res.q_end = score ? row : 0;       // all-zero saved column matches at index 0 (:263-271)
        res.t_end = score ? col : -1;      // byte pass initialises end_db = -1 (:118)
        res.q_start = -1;
        res.t_start = -1;
        res.word = (score + Q.qbias >= 255) ? 1 : 0;
        *o = res;
        if (marked) sw_lds().half_flag = 1;
    } else {
        if (cols > 0) {
            // column index counts backwards from t_end; row is an index into the reversed query
            // score 0: no strip reached the forward score - "Score of forward/backward SW differ" (:1191-1201)
            o->t_start = (score == o->score) ? end - col : -2;
            o->q_start = (score == o->score) ? Q.qlen - 1 - row : -2;
        }
    }
}

// One job: the pairs of its hit list against its query, eight (W = 32: four) per wavefront at a time.  The steps around the scan are
// the functions above.  Three steps stay inline, under their banners: the pair setup, the tile scan and the fold of a tile.  What the
// compiler makes of the column loop depends on them standing in one function with it - a function is simplified on its own before it is
// inlined, and what it settles there stays.  Tried as functions (scripts/sw_isa_audit.py against the inline form): the tile scan
// with its results by reference turns the selects of the rare `nm != vmax` block into branches; the pair setup changes the row
// search of the reverse bodies' rare block (rev_target's halves are opaque to the column step) and costs the wide bodies of R = 15, 16
// a wait state per column; the fold costs the multi-tile reverse body of R = 10 a wait state, and with its inputs as plain values
// the multi-tile bodies of R = 13, 14 two ds_reads.
// PF: the profile rows of a column are fetched one column ahead (see the column loop)
// HALF: the cells are computed in packed f16 (above, at SW_HALF_LIMIT); a pair whose score exceeds SW_HALF_LIMIT gets SW_HALF_MARK
//   for a result and raises the workgroup's flag in the LDS header.
// MARKED: the int16 forward scan of the pairs so marked, packed to the front like the live pairs of the reverse scan.
// W: lanes of a group, 16 or 32 (wide: a single tile of up to 32 R rows, four pairs per wavefront; the hand-off crosses the DPP row
//   boundary in the middle of the group, across_rows above).  Multi-tile bodies are 16 lanes wide.
template <int R, bool MULTI, bool REV, bool PF, bool HALF = false, bool MARKED = false, int W = GROUP>
__device__ __forceinline__ void sw_body(const SwLaunch &L, const SwJob job) {
    static_assert(!(HALF || MARKED) || (!MULTI && !REV && !(HALF && MARKED)), "f16 and its int16 re-run: single-tile forward scans");
    static_assert(W == GROUP || (W == 2 * GROUP && !MULTI), "the boundary row of a multi-tile body rotates inside one DPP row");
    constexpr bool PACKED = REV || MARKED;   // the job's pairs to scan are the ones listed in `live`
    constexpr int HITS_PER_WAVE = 2 * 64 / W;   // (W = 16: the file's constant)
    using T = Tile<R, W>;
    SwLds &H = sw_lds();
    // A multi-tile job is one long dependent chain (tiles x columns) however few targets it holds, and the batch ends
    // with the longest of them: those waves take the issue slots first, the short jobs sharing the SIMD fill the gaps.
    if (MULTI) __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane & (W - 1);
    const int grp = lane / W;
    const SwQuery Q = sw_query(L, job.query);
    const SwProfiles prof = sw_profiles<R, MULTI>(L, Q.qlen);
    const unsigned go2 = (HALF ? (unsigned)h_bits(L.gap_open) : (unsigned)L.gap_open) * 0x10001u;
    const unsigned ge2 = (HALF ? (unsigned)h_bits(L.gap_extend) : (unsigned)L.gap_extend) * 0x10001u;
    const unsigned pad_letter = (unsigned)L.alphabet;

    if (threadIdx.x == 0) H.next_chunk = 0;
    if (HALF && threadIdx.x == 0) H.half_flag = 0;
    sw_build_profiles<SW_AT_JOB_START, R, REV, HALF, PACKED, W>(L, Q, prof);
    uint32_t n_hits = job.hit_end - job.hit_begin;
    if (PACKED) {
        n_hits = sw_pack_live<REV, MARKED>(L, job, H, n_hits);
        if (n_hits == 0) return;      // (workgroup-uniform) no pair of this job needs a start position: no profile either
    }
    sw_build_profiles<SW_AT_PACKED, R, REV, HALF, PACKED, W>(L, Q, prof);
    const uint32_t n_iter = (n_hits + WAVES * HITS_PER_WAVE - 1) / (WAVES * HITS_PER_WAVE);

    for (uint32_t it = 0; prof.dynamic || it < n_iter; ++it) {
        const uint32_t slot0 = sw_claim_chunk<W>(H, prof.dynamic, it);
        if (prof.dynamic && slot0 >= n_hits) break;   // wave-uniform; the jobs in step keep every wave in the barrier loop

        // ---- the two targets of this group ------------------------------------------------------
        const uint32_t sA = slot0 + grp * 2, sB = sA + 1;
        const bool vA = sA < n_hits, vB = sB < n_hits;
        const uint32_t hA = job.hit_begin + (PACKED ? (uint32_t)H.live[vA ? sA : 0] : sA);
        const uint32_t hB = job.hit_begin + (PACKED ? (uint32_t)H.live[vB ? sB : 0] : sB);
        const uint32_t tA = vA ? L.hit_target[hA] : 0u, tB = vB ? L.hit_target[hB] : 0u;
        const uint8_t *pA = L.t_res + (size_t)L.t_off4[tA] * 4;
        const uint8_t *pB = L.t_res + (size_t)L.t_off4[tB] * 4;
        int colsA = vA ? (int)L.t_len[tA] : 0, colsB = vB ? (int)L.t_len[tB] : 0;
        int r0A = 0, r0B = 0;       // REV: first live row of the reversed query
        int endA = 0, endB = 0;     // REV: forward t_end
        unsigned rev_target = 0xFFFFFFFFu;
        if (REV) {
            // reverse scan over q[0..q_end] x t[0..t_end], both walked backwards (:1143-1175)
            // Lanes without a live pair must not take positions from a result slot: slot 0 may still be unwritten
            // (another workgroup's forward pass), and an arbitrary t_end there becomes a wild target address below.
            mmgpu_sw_hit fa, fb;
            fa.score = 0; fa.q_end = 0; fa.t_end = 0;
            fb = fa;
            if (vA) fa = L.out[L.hit_out[hA]];
            if (vB) fb = L.out[L.hit_out[hB]];
            // (every packed hit passed sw_rev_wanted above)
            colsA = vA ? fa.t_end + 1 : 0;
            colsB = vB ? fb.t_end + 1 : 0;
            endA = colsA > 0 ? fa.t_end : 0;
            endB = colsB > 0 ? fb.t_end : 0;
            r0A = colsA > 0 ? Q.qlen - 1 - fa.q_end : 0;
            r0B = colsB > 0 ? Q.qlen - 1 - fb.q_end : 0;
            // the score the reverse scan has to reach (terminate = r.score1, :1159-1175); 0xFFFF can never be reached
            rev_target = (colsA > 0 ? (unsigned)fa.score & 0xFFFFu : 0xFFFFu) | ((colsB > 0 ? (unsigned)fb.score & 0xFFFFu : 0xFFFFu) << 16);
        }
        int ncols = colsA > colsB ? colsA : colsB;
        ncols = max(ncols, __shfl_xor(ncols, 16));
        ncols = max(ncols, __shfl_xor(ncols, 32));
        ncols = __builtin_amdgcn_readfirstlane(ncols);
        const int nsteps = ncols + W - 1;
        // the shortest target of the wavefront (a half without a pair counts as 0 columns): letter blocks that end at or
        // before it hold no padding column in any group
        int mincols = colsA < colsB ? colsA : colsB;
        mincols = min(mincols, __shfl_xor(mincols, 16));
        mincols = min(mincols, __shfl_xor(mincols, 32));
        mincols = __builtin_amdgcn_readfirstlane(mincols);

        unsigned long long bestA = 0, bestB = 0;   // (score << 32) | (~col << 16) | ~row, maximised

        // the scratch lines of this wavefront (a wave-uniform address) and where the group's two start in them
        uint2 *scr = nullptr;
        unsigned scr_grp = 0;
        if (MULTI) {
            scr = L.scratch + (size_t)((job.shape >> 8) * WAVES + wave) * GROUPS_PER_WAVE * 2 * L.scratch_cols;
            scr_grp = (unsigned)grp * 2u * L.scratch_cols;
        }

        // ---- tile scan: one tile of the query against the two targets of every group, column by column ----
        for (int tile = 0; tile < prof.n_tiles; ++tile) {
            const int tile_base = tile * T::ROWS;
            sw_build_profiles<SW_AT_TILE, R, REV, HALF, PACKED, W>(L, Q, prof, tile);
            // the profile of this tile: the one there is, or this tile's of the resident ones (no barrier: nobody writes them).
            // Without the barriers nothing but program order stands between tile t's stores to its scratch line (lane 15 of a
            // group) and tile t + 1's loads from it (the group's head lane): the hand-over of the boundary row relies on both
            // being lanes of ONE wavefront, whose vector memory operations on the same addresses complete in order.  A group
            // spread over two wavefronts would need a fence and a barrier here again.
            const unsigned char *const lds_tile = MULTI && prof.resident ? prof.lds + (uint32_t)tile * prof.tile_bytes : prof.lds;
            const uint2 *scr_in = MULTI ? scr + (size_t)((tile + 1) & 1) * L.scratch_cols : nullptr;
            uint2 *scr_out = MULTI ? scr + (size_t)(tile & 1) * L.scratch_cols : nullptr;
            const bool has_above = MULTI && tile > 0;
            const bool has_below = MULTI && tile + 1 < prof.n_tiles;

            // forward: snap[] = the strip's H values in the column where the running maximum last rose (q_end);
            // reverse: rmask[] = rows of the reversed query that lie inside q[0..q_end] - the reverse scan needs no
            // snapshot, it ends in the first column that reaches the forward score (see below), so the two bodies of a
            // kernel need the same number of registers and the forward scan keeps its own occupancy
            unsigned Hp[R], E[R], aux[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { Hp[r] = 0; E[r] = 0; aux[r] = 0; }
            if (REV) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int rg = tile_base + g * R + r;
                    aux[r] = (rg >= r0A ? 0xFFFFu : 0u) | (rg >= r0B ? 0xFFFF0000u : 0u);
                }
            }
            unsigned vmax = 0, bestcol = 0xFFFFFFFFu;
            unsigned rev_rowA = 0, rev_rowB = 0;   // REV: first row holding the forward score in the column that reached it
            unsigned Hup_prev = 0;
            unsigned out_H = 0, out_F = 0;

            // Four columns' letters per dword load (every lane of the group loads the same word).  Forward: targets
            // start 4-byte aligned and the residue buffer ends with max_len + 64 bytes of slack (mmgpu_load_targets), so
            // no clamping is needed: columns past a target's end are replaced by the padding letter below.  Reverse:
            // column c is byte t[t_end - c], block k = the (unaligned) word at t_end - 3 - 4k read from its top byte down;
            // words wholly before the target are clamped to offset -3 (the buffer starts with 64 bytes of padding).
            // One v_bfe per target and column instead of an address computation and a byte load: 16-18 fewer
            // instructions per column (R = 12: 194 -> 177).
            auto letters4 = [&](const uint8_t *p, int end, int k) -> unsigned {
                if (!REV) return reinterpret_cast<const unsigned *>(p)[k];
                int o = end - 3 - 4 * k;
                o = o < -3 ? -3 : o;
                unsigned w;
                __builtin_memcpy(&w, p + o, 4);
                return w;
            };
            unsigned wA = letters4(pA, endA, 0), wB = letters4(pB, endB, 0);
            unsigned wA_next = letters4(pA, endA, 1), wB_next = letters4(pB, endB, 1);
            // Boundary row of the tile above, 16 columns (a stretch) at a time: the lanes of the group load one column each -
            // one coalesced load per 16 steps, issued a stretch ahead - and the live stretch is rotated by one lane per step,
            // so that the head lane holds column s at step s.  A stretch changes where a block of four steps begins (below):
            // stretch 0 is the columns 0 .. 15, of which the steps 0 .. 14 use 15, stretch m >= 1 the columns 16 m - 1 .. 16 m + 14.
            // The index is clamped to the last column of the wavefront: the steps past a group's (or the wavefront's) end read
            // that column again, as harmless as it was.
            // Boundary row for the tile below: lane 15 stores its hand-off in every step from its first column on (see there).
            uint2 bnd = make_uint2(0, 0), bnd_next = make_uint2(0, 0);   // (H, F) of the live stretch and of the one after it
            auto boundary16 = [&](int m) -> uint2 {   // m is wave-uniform
                const int last = ncols - 1 < 0 ? 0 : ncols - 1;
                return scr_in[scr_grp + (unsigned)min(16 * m + g - (m > 0 ? 1 : 0), last)];
            };
            if (has_above) {
                bnd = boundary16(0);
                bnd_next = boundary16(1);
            }

            // R scores per target as ND = ceil(R / 2) packed dwords (odd R: the high half of the last one is row padding
            // nobody selects): ds_read_b128 for whole 16-byte slots, b64 / b32 for the tail
            constexpr int ND = (R + 1) / 2;
            unsigned pav_next[PF ? ND : 1], pbv_next[PF ? ND : 1];   // PF: the rows fetched for the next step
            auto load_rows = [&](unsigned letters, unsigned *pav, unsigned *pbv) {
                const unsigned a = letters & 0xFFu, b = (letters >> 8) & 0xFFu;
                const uint4 *rowA = reinterpret_cast<const uint4 *>(lds_tile + a * T::ROW_STRIDE + g * T::LANE_STRIDE);
                const uint4 *rowB = reinterpret_cast<const uint4 *>(lds_tile + b * T::ROW_STRIDE + g * T::LANE_STRIDE);
#pragma unroll
                for (int k = 0; k < ND / 4; ++k) {
                    const uint4 pa = rowA[k], pb = rowB[k];
                    pav[4 * k] = pa.x; pav[4 * k + 1] = pa.y; pav[4 * k + 2] = pa.z; pav[4 * k + 3] = pa.w;
                    pbv[4 * k] = pb.x; pbv[4 * k + 1] = pb.y; pbv[4 * k + 2] = pb.z; pbv[4 * k + 3] = pb.w;
                }
                if constexpr (ND % 4 >= 2) {
                    const uint2 pa = *reinterpret_cast<const uint2 *>(rowA + ND / 4);
                    const uint2 pb = *reinterpret_cast<const uint2 *>(rowB + ND / 4);
                    pav[(ND / 4) * 4] = pa.x; pav[(ND / 4) * 4 + 1] = pa.y;
                    pbv[(ND / 4) * 4] = pb.x; pbv[(ND / 4) * 4 + 1] = pb.y;
                }
                if constexpr (ND % 2 == 1) {
                    pav[ND - 1] = reinterpret_cast<const unsigned *>(rowA)[ND - 1];
                    pbv[ND - 1] = reinterpret_cast<const unsigned *>(rowB)[ND - 1];
                }
            };
            // The letters lane g needs in step s + 1 are the letters lane g - 1 holds in step s (the head lane's come from the
            // letter words): every body hands them on in step s, between the two phases, where the DPP move has the packed ops
            // of the rows around it - at the top of a column it stood behind the instruction that made the head lane's letters,
            // and short columns paid wait states for that.  `let` is carried from step to step; the prologue takes column 0.
            // PF: the profile rows of a column are fetched one column ahead as well: the ds_reads of step s + 1 are issued in
            // step s behind the hand-off, that is behind the last use of the rows of step s (phase 1) and in front of the
            // serial chain (phase 2): the LDS round trip is covered by the wavefront's own instructions instead of standing
            // at the top of every column.  pav / pbv are carried from step to step too; the prologue fetches column 0.
            // The step after the last one fetches the padding letter's row (s + 1 >= cols), which every tile has: nothing
            // is read past the profile.  The rows stay in the same registers (the reads stand behind their last use), but
            // the compiler moves some reads up, which costs 6 - 24 registers per kernel.
            unsigned let = pad_letter * 0x101u;   // what a lane holds before its first column
            // The head lane's letters, prepared once per block of four columns: wA / wB are interleaved into the queue
            // `lq` of four (a | b << 8) pairs in the order the columns consume them (two v_perm_b32), and a column shifts
            // its pair out (the consumers read the low 16 bits of `let` only).  Columns past a target's end get the padding
            // letter here, per block and only in the blocks that reach past the wavefront's shortest target (a scalar
            // branch): the column loop holds no compare and no select for them.
            // The single-tile bodies of R <= 6 have too few instructions per column to take this form without wait states they
            // did not have (profiles/sw_isa_audit.txt): forward they select per column as before (LETTER_BLOCKS
            // false), in reverse the column shifts the queue itself instead of indexing it (LETTER_QUEUE), one instruction more.
            constexpr bool LETTER_BLOCKS = MULTI || REV || R >= 7;
            constexpr bool LETTER_QUEUE = !MULTI && R < 7;
            unsigned long long lq = 0;
            auto letter_block = [&](int k) {   // block k = columns 4k .. 4k + 3, from wA / wB
                if (!LETTER_BLOCKS) return;
                unsigned a = wA, b = wB;
                if (4 * k + 4 > mincols) {   // wave-uniform
                    const unsigned pad4 = pad_letter * 0x01010101u;
                    const int na = min(max(colsA - 4 * k, 0), 4), nb = min(max(colsB - 4 * k, 0), 4);   // live columns of the block
                    // forward: column 4k + i is byte i; reverse: byte 3 - i
                    const unsigned ma = REV ? ~(unsigned)(0xFFFFFFFFull >> (8 * na)) : (unsigned)((1ull << (8 * na)) - 1ull);
                    const unsigned mb = REV ? ~(unsigned)(0xFFFFFFFFull >> (8 * nb)) : (unsigned)((1ull << (8 * nb)) - 1ull);
                    a = bfi(ma, a, pad4);
                    b = bfi(mb, b, pad4);
                }
                const unsigned lo = __builtin_amdgcn_perm(b, a, REV ? 0x06020703u : 0x05010400u);
                const unsigned hi = __builtin_amdgcn_perm(b, a, REV ? 0x04000501u : 0x07030602u);
                lq = ((unsigned long long)hi << 32) | lo;
            };
            auto head_letters = [&](int c, int j) -> unsigned {   // column c of the head lane = pair j of the block; j is wave-uniform
                if (LETTER_BLOCKS && LETTER_QUEUE) { const unsigned v = (unsigned)lq; lq >>= 16; return v; }
                if (LETTER_BLOCKS) return (unsigned)(lq >> (16 * j));   // (plus bits nobody reads)
                const unsigned sh = (unsigned)(REV ? 3 - j : j) * 8u;
                const unsigned la0 = __builtin_amdgcn_ubfe(wA, sh, 8u);
                const unsigned lb0 = __builtin_amdgcn_ubfe(wB, sh, 8u);
                return (c < colsA ? la0 : pad_letter) | ((c < colsB ? lb0 : pad_letter) << 8);
            };
            letter_block(0);
            let = from_lane_above<W>(head_letters(0, 0), let);
            if (PF) load_rows(let, pav_next, pbv_next);

            // blocks of four steps, one dword of letters per target and block.  Step s hands on the letters of column
            // s + 1, so a block is the steps 4k - 1 .. 4k + 2 (the first one the steps 0 .. 2).
            // Invariant: in block s0 = 4k - 1, wA / wB hold the k-th letter word (lq its four pairs), and step j of the block
            // fetches column 4k + j = byte j of it (reverse: byte 3 - j).
            for (int s0 = -1; s0 < nsteps; s0 += 4) {
            if (MULTI && s0 > 0 && ((s0 + 1) & 15) == 0) {   // every fourth block (s0 = 16 m - 1): stretch m of the boundary row
                bnd = bnd_next;
                if (has_above) bnd_next = boundary16(((s0 + 1) >> 4) + 1);
            }
            const int jn = min(4, nsteps - s0);
#pragma nounroll
            for (int j = s0 < 0 ? 1 : 0; j < jn; ++j) {
                const int s = s0 + j;
                // ---- inputs of this step: from the lane above, or the tile boundary for the head lane ----
                // Lane 15 works on column s - 15, which lies inside [0, ncols) from step 15 to the last one: what it handed off
                // in the step before is stored here, under a scalar test - the lane mask is the same in every step, and the
                // address is the line's (wave-uniform) plus a fixed lane offset.  (The last column: behind the loop.)
                if (has_below && s >= GROUP) {
                    if (g == GROUP - 1) (scr_out + (s - GROUP))[scr_grp] = make_uint2(out_H, out_F);
                }
                const unsigned Hup = MULTI ? from_lane_above<W>(bnd.x, out_H) : from_lane_above_or_zero<W>(out_H);
                unsigned f = MULTI ? from_lane_above<W>(bnd.y, out_F) : from_lane_above_or_zero<W>(out_F);
                if (MULTI) {
                    // the live stretch moves up one lane (row_ror:15)
                    bnd.x = __builtin_amdgcn_update_dpp(bnd.x, bnd.x, 0x12F, 0xF, 0xF, false);
                    bnd.y = __builtin_amdgcn_update_dpp(bnd.y, bnd.y, 0x12F, 0xF, 0xF, false);
                }
                unsigned pav[ND], pbv[ND];
                if (PF) {
#pragma unroll
                    for (int k = 0; k < ND; ++k) { pav[k] = pav_next[k]; pbv[k] = pbv_next[k]; }
                } else {
                    load_rows(let, pav, pbv);
                }

                unsigned hd = Hup_prev;
                Hup_prev = Hup;
                unsigned cmax = 0;
                // Phase 1 (no dependencies between rows): everything that only needs the previous column -
                // diagonal + score, max with E, and E - ge.  Phase 2 is the serial F chain down the strip
                // (max -> sub -> max per row) with the off-chain ops of the row (f - ge, column maximum, E
                // update) available to sit behind each dependent VOP3P op.  Compared with the single-loop form
                // the compiler needs 23 fewer register moves and 10 fewer wait states per column at R = 24
                // (346 -> 313 instructions).
                //
                // A packed op that reads the result of the packed op right in front of it costs a wait state (s_nop).  A row
                // of phase 2 is six ops, three of them the chain h -> t -> f'; with the other three between the links
                // (h, f - ge, t, cmax, f', E[r]) no op reads its predecessor.  Left alone, the compiler sinks all R updates of
                // E out of the rows, past the `nm != vmax` branch, into a block of their own: five ops per row and a wait state
                // in each, 1.75 R + 2 per column, one issue slot in seven.  SW_KEEP_IN_ROW is an EMPTY asm on the value: it emits nothing (so the
                // hazard recognizer still sees real neighbours), but the update has to be done where the row is.  What was
                // tried and does not work on this toolchain: an asm per op or two-operand asms that chain the ops (the
                // recognizer pads around every asm boundary: 44 -> 73 and -> 97 wait states at R = 24),
                // __builtin_amdgcn_sched_barrier after each row (no effect: the sinking happens before scheduling), an
                // anchor on cmax as well (the multi-tile bodies had one while their boundary store stood behind phase 2; with the
                // store at the top of the step it puts `t` right in front of `f'` in every second row from R = 17 on).  If a later compiler
                // stops honouring the anchor (tests/test_sw_isa_audit.py notices), the structural alternatives are: rotate
                // the body so that the `nm != vmax` bookkeeping of column s runs at the top of step s + 1 (Hp[] and col are
                // still there; the tail of the step is then straight-line code with no join block to sink into), or fold
                // the E update into the chain's data flow.
                // The schedule is sensitive to the shape of the source around it: with pav / pbv declared outside the column
                // loop the multi-tile bodies get a wait state per row back (scripts/sw_isa_audit.py after every change here).
                unsigned pre[R], es[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // (score of target A's letter, score of target B's letter) for query row r
                    unsigned P = __builtin_amdgcn_perm(pbv[r / 2], pav[r / 2], (r & 1) ? 0x07060302u : 0x05040100u);
                    // v_bitop3 (a ? b : c, table 0xCA) as an intrinsic: written as and/or the compiler hoists NEG2 & ~mask
                    // out of the column loop - R more live registers
                    if (REV) P = __builtin_amdgcn_bitop3_b32(aux[r], P, NEG2, 0xCA);
                    if constexpr (HALF) {   // the maximum with E[r] is the three-way maximum of phase 2
                        pre[r] = h_add(r == 0 ? hd : Hp[r - 1], P);
                        es[r] = h_sub(E[r], ge2);
                    } else {
                        pre[r] = pk_max_s(pk_add_sat(r == 0 ? hd : Hp[r - 1], P), E[r]);
                        es[r] = pk_sub_sat_u(E[r], ge2);
                    }
                }
                let = from_lane_above<W>(head_letters(s + 1, j), let);   // the next column's letters (PF: and profile rows)
                if (PF) load_rows(let, pav_next, pbv_next);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    unsigned h;
                    if constexpr (HALF) {
                        // max3(x, y, 0) for the unsigned saturating subtraction; the two-way maxima of cmax fold in pairs of rows
                        h = h_max3(pre[r], E[r], f);
                        const unsigned fs = h_sub(f, ge2);
                        const unsigned t = h_sub(h, go2);
                        cmax = r == 0 ? h : h_max(cmax, h);   // (max(0, h) is not h to the compiler: h might be a NaN)
                        f = h_max3(fs, t, 0u);
                        E[r] = h_max3(es[r], t, 0u);
                    } else {
                        h = pk_max_s(pre[r], f);
                        const unsigned fs = pk_sub_sat_u(f, ge2);
                        const unsigned t = pk_sub_sat_u(h, go2);
                        cmax = pk_max_u(cmax, h);
                        f = pk_max_u(fs, t);
                        E[r] = pk_max_u(es[r], t);
                    }
                    SW_KEEP_IN_ROW(E[r]);
                    Hp[r] = h;
                }
                out_H = Hp[R - 1];
                out_F = f;

                const int col = s - g;

                // ---- running maximum / column / snapshot (rarely taken once the scores have grown) ----
                const unsigned nm = pk_max_u(vmax, cmax);
                if (nm != vmax) {
                    const unsigned diff = nm ^ vmax;
                    if (!REV) {
                        const unsigned mask = ((diff & 0xFFFFu) ? 0xFFFFu : 0u) | ((diff >> 16) ? 0xFFFF0000u : 0u);
                        bestcol = bfi(mask, ((unsigned)col & 0xFFFFu) * 0x10001u, bestcol);
#pragma unroll
                        for (int r = 0; r < R; ++r) aux[r] = bfi(mask, Hp[r], aux[r]);
                    } else {
                        // Reverse scan: nothing in q[0..q_end] x t[0..t_end] scores above the forward score, and the
                        // reference stops in the first column whose maximum equals it (terminate, :232-248 / :414-425 with
                        // :1159-1175): the column in which this strip's maximum rises TO that score is the strip's candidate,
                        // its first row holding it the row - found once per pair, no snapshot of the strip is kept.
                        const unsigned x = nm ^ rev_target;
                        const bool hitA = (diff & 0xFFFFu) && !(x & 0xFFFFu), hitB = (diff >> 16) && !(x >> 16);
                        if (hitA | hitB) {
                            asm volatile("" ::: "memory");   // a real branch: if-converted, the row search below runs in every column
                            unsigned ra = 0, rb = 0;
#pragma unroll
                            for (int r = R - 1; r >= 0; --r) {
                                if ((Hp[r] & 0xFFFFu) == (rev_target & 0xFFFFu)) ra = (unsigned)r;
                                if ((Hp[r] >> 16) == (rev_target >> 16)) rb = (unsigned)r;
                            }
                            if (hitA) { bestcol = (bestcol & 0xFFFF0000u) | ((unsigned)col & 0xFFFFu); rev_rowA = ra; }
                            if (hitB) { bestcol = (bestcol & 0xFFFFu) | ((unsigned)col << 16); rev_rowB = rb; }
                        }
                    }
                    vmax = nm;
                }
            }
            {   // the next four columns' letters; the load after that is in flight for four steps
                wA = wA_next; wB = wB_next;
                const int k = ((s0 + 1) >> 2) + 2;
                wA_next = letters4(pA, endA, k); wB_next = letters4(pB, endB, k);
                letter_block(k - 1);
            }
            }
            if (has_below && ncols > 0 && g == GROUP - 1) (scr_out + (ncols - 1))[scr_grp] = make_uint2(out_H, out_F);

            // ---- fold this tile's lanes into the pair's running best (tie rules in the key order) ----
            unsigned rowA_first = rev_rowA, rowB_first = rev_rowB;
            unsigned sA = vmax & 0xFFFFu, sB = vmax >> 16;
            if (!REV) {
#pragma unroll
                for (int r = R - 1; r >= 0; --r) {
                    if ((aux[r] & 0xFFFFu) == sA) rowA_first = (unsigned)r;
                    if ((aux[r] >> 16) == sB) rowB_first = (unsigned)r;
                }
            } else {   // a strip that never reached the forward score has no candidate
                sA = sA == (rev_target & 0xFFFFu) ? sA : 0u;
                sB = sB == (rev_target >> 16) ? sB : 0u;
            }
            const unsigned rgA = (unsigned)(tile_base + g * R) + rowA_first;
            const unsigned rgB = (unsigned)(tile_base + g * R) + rowB_first;
            unsigned long long keyA = sA ? ((unsigned long long)sA << 32) | ((0xFFFFu - (bestcol & 0xFFFFu)) << 16) | (0xFFFFu - rgA) : 0ull;
            unsigned long long keyB = sB ? ((unsigned long long)sB << 32) | ((0xFFFFu - (bestcol >> 16)) << 16) | (0xFFFFu - rgB) : 0ull;
#pragma unroll
            for (int m = 1; m < W; m <<= 1) {
                const unsigned long long oa = __shfl_xor(keyA, m), ob = __shfl_xor(keyB, m);
                keyA = oa > keyA ? oa : keyA;
                keyB = ob > keyB ? ob : keyB;
            }
            bestA = keyA > bestA ? keyA : bestA;
            bestB = keyB > bestB ? keyB : bestB;
        }

        // ---- write results -----------------------------------------------------------------------
        if (g == 0) {
            if (vA) sw_write_result<REV, HALF>(L, Q, bestA, hA, endA, colsA);
            if (vB) sw_write_result<REV, HALF>(L, Q, bestB, hB, endB, colsB);
        }
    }
}

// Three launches per pass for the whole batch.  The tile shape (rows per lane R, single / multi tile) is a property
// of the job: every shape is its own instantiation of sw_body, picked per workgroup.  A launch per shape (32 kernels
// with grids from 50 to 3000 workgroups on side streams) left the chip underfilled - the runtime maps streams onto
// four hardware queues, and the long multi-tile jobs of the few long queries ran nearly alone at the end.  Shapes
// are grouped by register need instead (a kernel gets the registers of its largest body, which sets the occupancy of
// all of them): S (forward 80 / reverse 119 VGPRs), M (140 / 212), L and every multi-tile shape (212 / 256) - sw_group_of,
// mmgpu_internal.h, has the bounds.  Each group is one grid, longest job first; the three run concurrently.
// BOTH = false: forward scan only (MMGPU_SW_SCORE_END).  BOTH = true: the workgroup runs the reverse scan of its own
// pairs right after their forward scan - no grid-wide barrier between the passes, so the batch has one tail, not two.
// W = 32: the wide single-tile bodies (queries of 16 * SW_MAX_R + 1 .. 32 * SW_MAX_R residues); only the R such a query can have exist.
// the prefetch goes where it costs no wavefront and no wait states: not into the forward-only kernel of the largest single tiles,
// R = 25 .. 28 (183 registers, two wavefronts instead of three) and not into the multi-tile bodies (with it the compiler puts a
// wait state into every row of phase 2 again, profiles/sw_isa_audit.txt)
template <int R, bool MULTI, bool BOTH>
constexpr bool SW_PREFETCHES = MMGPU_SW_PREFETCH && !MULTI && (BOTH || sw_group_of(false, R) < 2);
template <int R, bool MULTI, bool BOTH, int W = GROUP>
__device__ __forceinline__ void sw_passes(const SwLaunch &L, const SwJob &job) {
    constexpr bool PF = SW_PREFETCHES<R, MULTI, BOTH>;
    if (!(BOTH && L.rev_only)) sw_body<R, MULTI, false, PF, false, false, W>(L, job);
    // multi-tile queries get their reverse scan from sw_rev_multi_kernel (sw_kernel.hip), per query instead of per job
    if constexpr (BOTH && !MULTI) {
        __threadfence_block();   // the forward results of this job, written by other waves of the workgroup
        __syncthreads();
        sw_body<R, MULTI, true, PF, false, false, W>(L, job);
    }
}

// occupancy floor (waves per SIMD; 512 registers per lane and SIMD) per group and kernel kind: what the compiler is told to
// fit.  Measured on the 10k x 1M lists (profiles/r03_exp_sw_occupancy_floors.txt): the floor changes the schedule even
// where the register count already fits.
#ifndef MMGPU_SW_WAVES_G0F
#define MMGPU_SW_WAVES_G0F 4
#endif
#ifndef MMGPU_SW_WAVES_G0B
#define MMGPU_SW_WAVES_G0B 2
#endif
#ifndef MMGPU_SW_WAVES_G1F
#define MMGPU_SW_WAVES_G1F 3
#endif
#ifndef MMGPU_SW_WAVES_G1B
#define MMGPU_SW_WAVES_G1B 2
#endif
// the two arguments of amdgpu_waves_per_eu of sw_kernel<G, BOTH> and its f16 twin sw_half_kernel<G, BOTH>
constexpr int sw_waves_floor(int G, bool BOTH) {
    return G == 0 ? (BOTH ? MMGPU_SW_WAVES_G0B : MMGPU_SW_WAVES_G0F) : (G == 1 ? (BOTH ? MMGPU_SW_WAVES_G1B : MMGPU_SW_WAVES_G1F) : SW_MIN_WAVES);
}
// upper bound: the forward + reverse kernel of the middle group is at the edge of a third wavefront per
// SIMD (168 - 170 registers) and runs slower with it (83.4 against 78.7 ms for the stage, round 6) - pinned.
// Re-measured with the wait states out of phase 2 and the rows fetched a column ahead (183 registers at
// two wavefronts): 75.41 ms for the stage at 2, 74.57 ms at 3 (profiles/sw_column_loop_bench.txt) - but at 3
// the compiler fits 168 registers only with 44 bytes of scratch per lane (spills around, not inside, the
// column loops).  Kept at 2: no kernel of this file uses scratch (tests/test_sw_isa_audit.py); the 0.8 ms
// are there for whoever gets this kernel to 168 registers without spilling.
constexpr int sw_waves_cap(int G, bool BOTH) { return G == 1 && BOTH ? MMGPU_SW_WAVES_G1B : 8; }

// ---- what the kernels do around the bodies: job, scratch slot, shape dispatch ------------------------------------------------
// fused prefilter -> align hand-over: the list length of the query is only known on the device.  False: nothing left of the job.
__device__ __forceinline__ bool sw_clip_job(const SwLaunch &L, SwJob &job) {
    if (L.q_hit_count) {
        const uint32_t lim = job.query * L.hit_stride + L.q_hit_count[job.query];
        job.hit_end = job.hit_end < lim ? job.hit_end : lim;
        if (job.hit_end <= job.hit_begin) return false;
    }
    return true;
}

// multi-tile jobs: claim a slot of the column-scratch pool.  The pool has at least as many slots as workgroups of the claiming
// kernels can be resident at once, so the search always ends; a slot is only ever read after its owner wrote it (tile t writes
// what tile t + 1 reads), so stale content is harmless.  The slot rides in the job's shape word above the shape code.
__device__ __forceinline__ void sw_claim_scratch(const SwLaunch &L, SwJob &job) {
    __shared__ uint32_t scratch_slot;
    if (threadIdx.x == 0) {
        uint32_t s = blockIdx.x % L.scratch_slots;
        while (atomicCAS(&L.scratch_busy[s], 0u, 1u) != 0u) s = s + 1 == L.scratch_slots ? 0u : s + 1;
        scratch_slot = s;
    }
    __syncthreads();
    job.shape = (job.shape & 0xFFu) | (scratch_slot << 8);
}
__device__ __forceinline__ void sw_release_scratch(const SwLaunch &L, const SwJob &job) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        atomicExch(&L.scratch_busy[job.shape >> 8], 0u);
    }
}

// The one list of rows per lane, and the one switch over a job's shape code: f(R, kind) for the shapes of kernel group G, both
// as compile-time values (std::integral_constant).  A shape exists for R <= SW_MAX_R; multi-tile from R = 8 (a query cut into
// tiles gets at least ceil(SW_MAX_R / 2) rows per lane: 8 .. 32 covers every SW_MAX_R the header allows), wide from the R of the
// shortest wide query.  Workgroup-uniform.
enum SwKind { SW_SINGLE, SW_MULTI, SW_WIDE };
constexpr bool sw_shape_exists(SwKind kind, int R) {
    return R <= SW_MAX_R && (kind != SW_MULTI || R >= 8) && (kind != SW_WIDE || R >= SW_WIDE_MIN_R);
}
#define MMGPU_SW_EACH_R(X)                                                                                                          \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) \
    X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
template <int G, typename F>
__device__ __forceinline__ void sw_dispatch_shape(uint32_t shape, F f) {
    static_assert(GROUP == 16 && SW_SHAPE_MULTI == 32 && SW_SHAPE_WIDE == 64, "the shape codes of the dispatch: 16-lane groups, + 32 multi-tile, + 64 wide");
#define MMGPU_SW_CASE(R, KIND, BASE)                                                                                                \
    case BASE + (R) - 1:                                                                                                            \
        if constexpr (sw_shape_exists(KIND, R) && sw_group_of(KIND == SW_MULTI, R) == G)                                            \
            f(std::integral_constant<int, R>(), std::integral_constant<SwKind, KIND>());                                            \
        break;
#define MMGPU_SW_CASES(R) MMGPU_SW_CASE(R, SW_SINGLE, 0) MMGPU_SW_CASE(R, SW_MULTI, SW_SHAPE_MULTI) MMGPU_SW_CASE(R, SW_WIDE, SW_SHAPE_WIDE)
    switch (shape & 0xFFu) {
        MMGPU_SW_EACH_R(MMGPU_SW_CASES)
        default: break;
    }
#undef MMGPU_SW_CASES
#undef MMGPU_SW_CASE
}

}  // namespace

}  // namespace mmgpu
