// linclust's k-mer matching stage on the device (include/mmgpu.h, "linclust's k-mer matching stage"): the kernels.
//
//   extraction   one wavefront per sequence (a protein of ~300 residues has ~290 windows, i.e. four to five rounds of
//                64 lanes; a 16-lane row would walk 18 rounds and leave three quarters of a wavefront to the longest of its four
//                sequences).  The selection needs the kmerConsidered-th smallest 16-bit score t and the surplus of its bin: a two-level
//                radix histogram in LDS (high byte, then the low byte within the high bin found) gives both - the reference's 65 536
//                bins do not fit.  Scores are recomputed per pass (a hash is ~25 integer instructions; a score array of a 32 766-residue
//                sequence would be 64 KB of LDS).  The reference's selection loop (:287-323) reduces to: every window with score < t is
//                taken; of the windows with score == t all are taken when the surplus is 0, else only the first `surplus` in position
//                order (its threshold drops by one when the surplus is used up - the quirk); the loop stops after kmerConsidered
//                windows.  Both ranks are ballots and population counts, so the records leave in position order.
//   scans        a three-kernel scan over uint32 (tile sums, scan of the tile sums by one workgroup, tile rescan) with the element
//                read through a functor, for the record offsets, the group starts (a maximum scan) and the three compactions.
//   group, vote  one thread per record / per (representative, member) run.
// The two sorts are rocprim::radix_sort_pairs (kmermatch_api.hip), each as two stable passes over parts of the key.
#include "kmm_device.h"

namespace mmgpu {

namespace {

// What one wavefront holds of its sequence while it walks the windows in rounds of 64 (the Walk of kmm_device.h)
struct KmmWalk {
    const uint8_t *res;      // the sequence's residues
    uint32_t L, n_win;       // n_win: windows with or without X
    int k;
    uint32_t base, x;        // alph_size - 1: the radix of the index and the reduced X
    unsigned long long seed;
    const uint8_t *red_tab;  // LDS: the reduction table
    uint8_t *st;             // LDS [96]: the staged round

    // st[0 .. 64 + k - 1): the reduced residues of round `c` and of the k - 1 behind it (KMM_MAX_K <= 32), X behind the sequence's end
    __device__ __forceinline__ void stage(uint32_t c, uint32_t lane) {
        const uint32_t p = c * 64u + lane;
        st[lane] = p < L ? red_tab[res[p] < 21u ? res[p] : 20u] : (uint8_t)x;
        if (lane < 32u) {
            const uint32_t q = c * 64u + 64u + lane;
            st[64u + lane] = q < L ? red_tab[res[q] < 21u ? res[q] : 20u] : (uint8_t)x;
        }
    }

    // the window at position c * 64 + lane: false when there is none or it holds an X
    __device__ __forceinline__ bool window(uint32_t c, uint32_t lane, unsigned long long &idx, uint32_t &pos, uint32_t &score) const {
        pos = c * 64u + lane;
        bool ok = pos < n_win;
        unsigned long long v = 0;
        for (int i = k - 1; i >= 0; i--) {      // Indexer::int2index: sum r[i] * base^i
            const uint32_t r = st[lane + i];
            ok = ok && r != x;
            v = v * base + r;
        }
        idx = v;
        score = (uint32_t)(xxh64_u64(v, seed) & 0xFFFFull);
        return ok;
    }

    __device__ __forceinline__ uint32_t residue(uint32_t lane) const { return st[lane]; }
};

__device__ __forceinline__ KmmWalk kmm_walk_of(const KmmExtractArgs &A, uint32_t sid, const uint8_t *red_tab, uint8_t *stage) {
    KmmWalk W;
    W.res = A.res + (size_t)A.off4[sid] * 4u;
    W.L = A.len[sid];
    W.k = A.k;
    W.n_win = W.L >= (uint32_t)A.k ? W.L - (uint32_t)A.k + 1u : 0u;
    W.base = (uint32_t)A.alph_size - 1u;
    W.x = W.base;
    W.seed = A.seed;
    W.red_tab = red_tab;
    W.st = stage;
    return W;
}

// Pass 1 of the extraction: per sequence the selection rule {t, surplus, considered} and the number of records it will write
__global__ __launch_bounds__(64) void kmm_count_kernel(KmmExtractArgs A) {
    __shared__ uint32_t hist[256];
    __shared__ uint8_t red_tab[32];
    __shared__ uint8_t stage[96];
    const uint32_t sid = blockIdx.x, lane = threadIdx.x;
    if (sid >= A.n) return;
    KmmWalk W = kmm_walk_of(A, sid, red_tab, stage);
    if (lane < 21u) red_tab[lane] = A.reduce[lane];
    kmm_count_body(W, hist, A.kmers_per_seq, A.kmers_per_seq_scale, lane, &A.rule[sid], &A.count[sid]);
}

// Pass 2: the records, at rec_off[sid]: the identity record, then the selected windows in position order
__global__ __launch_bounds__(64) void kmm_write_kernel(KmmExtractArgs A) {
    __shared__ uint8_t red_tab[32];
    __shared__ uint8_t stage[96];
    const uint32_t sid = blockIdx.x, lane = threadIdx.x;
    if (sid >= A.n) return;
    KmmWalk W = kmm_walk_of(A, sid, red_tab, stage);
    if (lane < 21u) red_tab[lane] = A.reduce[lane];
    __syncthreads();
    kmm_write_body(W, A.rule[sid], sid, A.rec_off[sid], lane, A.rec_kmer, A.rec_val);
}

// ---- scans ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

struct OpSum { __device__ static uint32_t op(uint32_t a, uint32_t b) { return a + b; } };
struct OpMax { __device__ static uint32_t op(uint32_t a, uint32_t b) { return a > b ? a : b; } };

// inclusive scan of one value per thread over a workgroup of SCAN_THREADS; `total` = the last
template <class Op>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *lds, uint32_t &total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {
        const uint32_t other = t >= d ? lds[t - d] : 0u;
        __syncthreads();
        if (t >= d) lds[t] = Op::op(lds[t], other);
        __syncthreads();
    }
    const uint32_t r = lds[t];
    total = lds[SCAN_THREADS - 1];
    __syncthreads();
    return r;
}

template <class F, class Op>
__global__ __launch_bounds__(256) void scan_tiles_kernel(F f, uint32_t n, uint32_t *tile_sum) {
    __shared__ uint32_t lds[SCAN_THREADS];
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; i++)
        if (first + i < n) v = Op::op(v, f((uint32_t)(first + i)));
    uint32_t total;
    block_scan<Op>(v, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum[n_tiles] -> its exclusive scan in place, by one workgroup
template <class Op>
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(uint32_t *tile_sum, uint32_t n_tiles) {
    __shared__ uint32_t lds[SCAN_THREADS];
    uint32_t carry = 0;
    for (uint32_t at = 0; at < n_tiles; at += SCAN_THREADS) {
        const uint32_t i = at + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_sum[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_scan<Op>(v, lds, total);
        // exclusive = carry op (everything before v in this round): for the sum incl - v, for the maximum the neighbour's inclusive
        lds[threadIdx.x] = incl;
        __syncthreads();
        const uint32_t before = threadIdx.x ? lds[threadIdx.x - 1] : 0u;
        __syncthreads();
        if (i < n_tiles) tile_sum[i] = Op::op(carry, before);
        carry = Op::op(carry, total);
    }
}

// out[i] = scan of f over [0, i) (EXCLUSIVE; out[n] = the total) or over [0, i] (inclusive)
template <class F, class Op, bool EXCLUSIVE>
__global__ __launch_bounds__(256) void scan_apply_kernel(F f, uint32_t n, const uint32_t *tile_sum, uint32_t *out) {
    __shared__ uint32_t lds[SCAN_THREADS];
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t item[SCAN_ITEMS];
    uint32_t v = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; i++) {
        item[i] = first + i < n ? f((uint32_t)(first + i)) : 0u;
        v = Op::op(v, item[i]);
    }
    uint32_t total;
    const uint32_t incl = block_scan<Op>(v, lds, total);
    lds[threadIdx.x] = incl;      // (block_scan has left lds free): the threads before this one are the neighbour's inclusive value
    __syncthreads();
    const uint32_t before = threadIdx.x ? lds[threadIdx.x - 1] : 0u;
    uint32_t run = Op::op(tile_sum[blockIdx.x], before);
    for (uint32_t i = 0; i < SCAN_ITEMS; i++) {
        if (first + i >= n) break;
        if (EXCLUSIVE) out[first + i] = run;
        run = Op::op(run, item[i]);
        if (!EXCLUSIVE) out[first + i] = run;
    }
    if (EXCLUSIVE && first < n && first + SCAN_ITEMS >= n) out[n] = run;      // the thread that holds element n - 1
}

template <class F, class Op, bool EXCLUSIVE>
hipError_t scan_u32(F f, uint32_t n, uint32_t *tile_sum, uint32_t *out, hipStream_t s) {
    if (n == 0) {
        if (EXCLUSIVE) return hipMemsetAsync(out, 0, sizeof(uint32_t), s);
        return hipSuccess;
    }
    const uint32_t tiles = (uint32_t)(((uint64_t)n + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL((scan_tiles_kernel<F, Op>), dim3(tiles), dim3(SCAN_THREADS), 0, s, f, n, tile_sum);
    hipLaunchKernelGGL((scan_tile_sums_kernel<Op>), dim3(1), dim3(SCAN_THREADS), 0, s, tile_sum, tiles);
    hipLaunchKernelGGL((scan_apply_kernel<F, Op, EXCLUSIVE>), dim3(tiles), dim3(SCAN_THREADS), 0, s, f, n, tile_sum, out);
    return hipGetLastError();
}

struct LoadU32 {
    const uint32_t *p;
    __device__ uint32_t operator()(uint32_t i) const { return p[i]; }
};

// ---- group -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t val_len(unsigned long long v) { return KMM_LEN_MASK - ((uint32_t)(v >> KMM_LEN_SHIFT) & KMM_LEN_MASK); }
__device__ __forceinline__ uint32_t val_id(unsigned long long v) { return (uint32_t)(v >> KMM_ID_SHIFT); }
__device__ __forceinline__ int val_pos(unsigned long long v) { return (int)(v & KMM_LEN_MASK); }

// NUCL (nuclmatch_api.hip): bit 63 of a k-mer is the strand its window was taken on and bit 63 of an emitted pair says whether the
// representative is aligned as it stands; neither takes part in a comparison
constexpr unsigned long long KMM_STRAND = 1ull << 63;
template <bool NUCL>
__device__ __forceinline__ bool same_key(unsigned long long a, unsigned long long b) { return NUCL ? ((a ^ b) & ~KMM_STRAND) == 0 : a == b; }

template <bool NUCL>
struct GroupHead {      // i where a k-mer's records begin, else 0: its maximum scan is every record's group start
    const unsigned long long *kmer;
    __device__ uint32_t operator()(uint32_t i) const { return i > 0 && !same_key<NUCL>(kmer[i], kmer[i - 1]) ? i : 0u; }
};

// the diagonal of member record `me` against its representative's (kmermatcher.cpp:636-663).  NUCL: a window taken as its reverse
// complement stores its position on the reverse strand, so both positions are counted from the far end when the member's is one;
// the representative stays as it is when both windows were taken on the same strand.  The reference computes in `short`: lengths
// and positions are below 32 767 here and nothing wraps
template <bool NUCL>
__device__ __forceinline__ int kmm_diagonal(const KmmGroupArgs &A, uint32_t g, uint32_t i, bool &as_it_is) {
    const unsigned long long rep = A.val[g], me = A.val[i];
    as_it_is = true;
    if (NUCL) {
        const bool rep_reverse = !(A.kmer[g] & KMM_STRAND), me_reverse = !(A.kmer[i] & KMM_STRAND);
        as_it_is = rep_reverse == me_reverse;
        if (me_reverse) return ((int)val_len(rep) - 1 - val_pos(rep)) - ((int)val_len(me) - 1 - val_pos(me));
    }
    return val_pos(rep) - val_pos(me);
}

// Util::canBeCovered (Util.cpp:542-559), float32 with IEEE division
__device__ __forceinline__ bool can_be_covered(float thr, int mode, float q, float t) {
    switch (mode) {
    case 0: return __fdiv_rn(q, t) >= thr && __fdiv_rn(t, q) >= thr;
    case 1: return __fdiv_rn(q, t) >= thr;
    case 2: return __fdiv_rn(t, q) >= thr;
    case 3: return __fdiv_rn(t, q) >= thr && __fdiv_rn(t, q) <= 1.0f;
    case 4: return __fdiv_rn(q, t) >= thr && __fdiv_rn(q, t) <= 1.0f;
    case 5: return __fdiv_rn(fminf(q, t), fmaxf(q, t)) >= thr;
    default: return true;
    }
}

template <bool NUCL>
struct GroupEmit {      // 1 when record i emits a (representative, member, diagonal), kmermatcher.cpp:633-672
    KmmGroupArgs A;
    __device__ uint32_t operator()(uint32_t i) const {
        const uint32_t g = A.group_start[i];
        if (g == i && (i + 1u == A.n_records || !same_key<NUCL>(A.kmer[i + 1u], A.kmer[i]))) return 0u;      // a group of one
        const int q_len = (int)val_len(A.val[g]), t_len = (int)val_len(A.val[i]);
        bool as_it_is;
        const int diagonal = kmm_diagonal<NUCL>(A, g, i, as_it_is);
        const bool extendable = diagonal < 0 || diagonal > q_len - t_len;
        const bool coverable = can_be_covered(A.cov_thr, A.cov_mode, (float)q_len, (float)t_len);
        return ((!A.only_extendable && coverable) || (A.only_extendable && extendable)) ? 1u : 0u;
    }
};

template <bool NUCL>
__global__ __launch_bounds__(256) void kmm_emit_kernel(KmmGroupArgs A, const uint32_t *emit_at, unsigned long long *pair, uint16_t *diag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_records) return;
    const GroupEmit<NUCL> E{A};
    if (!E(i)) return;
    const unsigned long long rep = A.val[A.group_start[i]], me = A.val[i];
    bool as_it_is;
    int diagonal = kmm_diagonal<NUCL>(A, A.group_start[i], i, as_it_is);
    uint32_t a = val_id(rep), b = val_id(me);
    if (!NUCL && val_len(rep) < val_len(me) && A.cov_mode == 1) {      // :679-683 (refused on nucleotides: the swap loses the strand)
        const uint32_t s = a; a = b; b = s;
        diagonal = -diagonal;
    }
    const uint32_t at = emit_at[i];
    pair[at] = ((unsigned long long)a << 32) | b | (NUCL && as_it_is ? KMM_STRAND : 0ull);      // (ids are below 2^31: a sequence has a record)
    diag[at] = (uint16_t)((uint32_t)diagonal ^ 0x8000u);      // the short, biased: the radix sort orders it as a signed value
}

// ---- vote --------------------------------------------------------------------------------------------------------------------------
template <bool NUCL>
struct PairKept {      // 1 where a (representative, member) run with member != representative begins
    const unsigned long long *pair;
    __device__ uint32_t operator()(uint32_t i) const {
        const unsigned long long p = NUCL ? pair[i] & ~KMM_STRAND : pair[i];
        return (i == 0 || !same_key<NUCL>(pair[i - 1], p)) && (uint32_t)(p >> 32) != (uint32_t)p ? 1u : 0u;
    }
};

// writeKmerMatcherResult (:1614-1655) per kept run: score = its length, diagonal = the value with the longest run, the last on a tie.
// NUCL: the reference's walk compares every entry with the representative's id, whose bit 63 it has cleared, so it covers the run's
// leading entries with a reverse-complemented representative only and the score is minus their number; a run that begins with an
// as-it-is entry is not walked at all: score 0 and that entry's diagonal, the smallest
template <bool NUCL>
__global__ __launch_bounds__(256) void kmm_vote_kernel(const unsigned long long *pair, const uint16_t *diag, uint32_t n_pairs, const uint32_t *kept_at,
                                                        mmgpu_pf_hit *records, uint32_t *kept_rep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pairs) return;
    const PairKept<NUCL> K{pair};
    if (!K(i)) return;
    const unsigned long long p = NUCL ? pair[i] & ~KMM_STRAND : pair[i];
    uint32_t score = 0, best_cnt = 0, cnt = 0;
    uint16_t best = diag[i], prev = diag[i];
    for (uint32_t j = i; j < n_pairs && pair[j] == p; j++) {
        const uint16_t d = diag[j];
        cnt = d == prev ? cnt + 1u : 1u;
        if (cnt >= best_cnt) { best = d; best_cnt = cnt; }
        prev = d;
        score++;
    }
    const uint32_t rep = (uint32_t)(p >> 32), at = kept_at[i];
    mmgpu_pf_hit h;
    h.id = (uint32_t)p;
    h.score = NUCL ? -(int32_t)score : (int32_t)score;
    h.diagonal = (uint16_t)(best ^ 0x8000u);
    h.reserved = 0;
    records[(size_t)rep + 1u + at] = h;      // `rep + 1` lists' first entries and `at` kept runs lie before it
    kept_rep[at] = rep;
}

// offsets[s] = s + (kept runs of representatives below s); the {s, 0, 0} entry of every list
__global__ __launch_bounds__(256) void kmm_offsets_kernel(const uint32_t *kept_rep, uint32_t n_kept, uint32_t n, unsigned long long *offsets,
                                                           mmgpu_pf_hit *records) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > n) return;
    uint32_t lo = 0, hi = n_kept;
    while (lo < hi) {      // the first kept run whose representative is >= s
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (kept_rep[mid] < s) lo = mid + 1u; else hi = mid;
    }
    const unsigned long long off = (unsigned long long)s + lo;
    offsets[s] = off;
    if (s < n) {
        mmgpu_pf_hit h;
        h.id = s;
        h.score = 0;
        h.diagonal = 0;
        h.reserved = 0;
        records[off] = h;
    }
}

// the hand-over to the rescoring: entry e of the CSR -> hit_query[e] = its list, pairs[e] = (target, diagonal)
__global__ __launch_bounds__(256) void kmm_handover_kernel(const unsigned long long *offsets, uint32_t n, const mmgpu_pf_hit *records, uint32_t n_entries,
                                                            uint32_t *hit_query, mmgpu_rescore_pair *pairs) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n_entries) return;
    uint32_t lo = 0, hi = n;      // the last list whose offset is <= e (offsets[0] == 0, every list holds an entry)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= e) lo = mid; else hi = mid;
    }
    hit_query[e] = lo;
    mmgpu_rescore_pair p;
    p.target = records[e].id;
    p.diagonal = records[e].diagonal;
    p.reserved = 0;
    pairs[e] = p;
}

}  // namespace

hipError_t launch_kmm_extract_count(const KmmExtractArgs &A, hipStream_t s) {
    if (A.n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmm_count_kernel, dim3(A.n), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_kmm_record_offsets(const uint32_t *count, uint32_t n, uint32_t *tile_sum, uint32_t *rec_off, hipStream_t s) {
    return scan_u32<LoadU32, OpSum, true>(LoadU32{count}, n, tile_sum, rec_off, s);
}

hipError_t launch_kmm_extract_write(const KmmExtractArgs &A, hipStream_t s) {
    if (A.n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmm_write_kernel, dim3(A.n), dim3(64), 0, s, A);
    return hipGetLastError();
}

// group_start[n_records], emit_at[n_records + 1] (emit_at[n_records] = the number of emitted records)
hipError_t launch_kmm_group_scan(const KmmGroupArgs &A, uint32_t *tile_sum, uint32_t *emit_at, hipStream_t s) {
    hipError_t e = A.nucl ? scan_u32<GroupHead<true>, OpMax, false>(GroupHead<true>{A.kmer}, A.n_records, tile_sum, A.group_start, s)
                          : scan_u32<GroupHead<false>, OpMax, false>(GroupHead<false>{A.kmer}, A.n_records, tile_sum, A.group_start, s);
    if (e != hipSuccess) return e;
    return A.nucl ? scan_u32<GroupEmit<true>, OpSum, true>(GroupEmit<true>{A}, A.n_records, tile_sum, emit_at, s)
                  : scan_u32<GroupEmit<false>, OpSum, true>(GroupEmit<false>{A}, A.n_records, tile_sum, emit_at, s);
}

hipError_t launch_kmm_emit(const KmmGroupArgs &A, const uint32_t *emit_at, unsigned long long *pair, uint16_t *diag, hipStream_t s) {
    if (A.n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(A.nucl ? kmm_emit_kernel<true> : kmm_emit_kernel<false>, dim3((A.n_records + 255u) / 256u), dim3(256), 0, s, A, emit_at, pair, diag);
    return hipGetLastError();
}

// kept_at[n_pairs + 1] (kept_at[n_pairs] = the number of kept runs)
hipError_t launch_kmm_vote_scan(const unsigned long long *pair, uint32_t n_pairs, bool nucl, uint32_t *tile_sum, uint32_t *kept_at, hipStream_t s) {
    return nucl ? scan_u32<PairKept<true>, OpSum, true>(PairKept<true>{pair}, n_pairs, tile_sum, kept_at, s)
                : scan_u32<PairKept<false>, OpSum, true>(PairKept<false>{pair}, n_pairs, tile_sum, kept_at, s);
}

hipError_t launch_kmm_vote(const unsigned long long *pair, const uint16_t *diag, uint32_t n_pairs, bool nucl, const uint32_t *kept_at, uint32_t n_kept, uint32_t n,
                           uint32_t *kept_rep, unsigned long long *offsets, mmgpu_pf_hit *records, hipStream_t s) {
    if (n_pairs) hipLaunchKernelGGL(nucl ? kmm_vote_kernel<true> : kmm_vote_kernel<false>, dim3((n_pairs + 255u) / 256u), dim3(256), 0, s, pair, diag, n_pairs, kept_at, records, kept_rep);
    hipLaunchKernelGGL(kmm_offsets_kernel, dim3((n + 1u + 255u) / 256u), dim3(256), 0, s, kept_rep, n_kept, n, offsets, records);
    return hipGetLastError();
}

hipError_t launch_kmm_handover(const unsigned long long *offsets, uint32_t n, const mmgpu_pf_hit *records, uint32_t n_entries, uint32_t *hit_query,
                               mmgpu_rescore_pair *pairs, hipStream_t s) {
    if (n_entries == 0) return hipSuccess;
    hipLaunchKernelGGL(kmm_handover_kernel, dim3((n_entries + 255u) / 256u), dim3(256), 0, s, offsets, n, records, n_entries, hit_query, pairs);
    return hipGetLastError();
}

}  // namespace mmgpu
