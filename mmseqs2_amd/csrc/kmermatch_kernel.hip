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
#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

constexpr unsigned long long XXH_P1 = 11400714785074694791ull, XXH_P2 = 14029467366897019727ull, XXH_P3 = 1609587929392839161ull,
                             XXH_P4 = 9650029242287828579ull, XXH_P5 = 2870177450012600261ull;

__device__ __forceinline__ unsigned long long rotl64(unsigned long long x, int r) { return (x << r) | (x >> (64 - r)); }

// XXH64 of one 8-byte little-endian word (xxHash specification: inputs below 32 bytes start from seed + PRIME5, one 8-byte lane,
// the avalanche)
__device__ __forceinline__ unsigned long long xxh64_u64(unsigned long long v, unsigned long long seed) {
    unsigned long long h = seed + XXH_P5 + 8ull;
    h ^= rotl64(v * XXH_P2, 31) * XXH_P1;
    h = rotl64(h, 27) * XXH_P1 + XXH_P4;
    h ^= h >> 33;
    h *= XXH_P2;
    h ^= h >> 29;
    h *= XXH_P3;
    h ^= h >> 32;
    return h;
}

__device__ __forceinline__ unsigned long long pow31(uint32_t e) {
    unsigned long long r = 1, b = 31;
    for (; e; e >>= 1, b *= b)
        if (e & 1u) r *= b;
    return r;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask, uint32_t lane) {
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// What one wavefront holds of its sequence while it walks the windows in rounds of 64
struct KmmWalk {
    const uint8_t *res;      // the sequence's residues
    uint32_t L, n_win;       // n_win: windows with or without X
    int k;
    uint32_t base, x;        // alph_size - 1: the radix of the index and the reduced X
    unsigned long long seed;
};

// stage[0 .. 64 + k - 1): the reduced residues of round `c` and of the k - 1 behind it (KMM_MAX_K <= 32), X behind the sequence's end
__device__ __forceinline__ void kmm_stage(const KmmWalk &W, uint32_t c, const uint8_t *red_tab, uint8_t *stage, uint32_t lane) {
    const uint32_t p = c * 64u + lane;
    stage[lane] = p < W.L ? red_tab[W.res[p] < 21u ? W.res[p] : 20u] : (uint8_t)W.x;
    if (lane < 32u) {
        const uint32_t q = c * 64u + 64u + lane;
        stage[64u + lane] = q < W.L ? red_tab[W.res[q] < 21u ? W.res[q] : 20u] : (uint8_t)W.x;
    }
}

// the window at position c * 64 + lane: false when there is none or it holds an X
__device__ __forceinline__ bool kmm_window(const KmmWalk &W, uint32_t c, const uint8_t *stage, uint32_t lane, unsigned long long &idx, uint32_t &score) {
    const uint32_t p = c * 64u + lane;
    bool ok = p < W.n_win;
    unsigned long long v = 0;
    for (int i = W.k - 1; i >= 0; i--) {      // Indexer::int2index: sum r[i] * base^i
        const uint32_t r = stage[lane + i];
        ok = ok && r != W.x;
        v = v * W.base + r;
    }
    idx = v;
    score = (uint32_t)(xxh64_u64(v, W.seed) & 0xFFFFull);
    return ok;
}

// hist[256] (LDS, complete): the bin that holds the `want`-th smallest element (1-based, want <= sum of hist) and the elements below
// that bin.  Uniform over the wavefront.
__device__ __forceinline__ uint32_t kmm_find_bin(const uint32_t *hist, uint32_t want, uint32_t lane, uint32_t &below) {
    const uint32_t h0 = hist[4u * lane], h1 = hist[4u * lane + 1u], h2 = hist[4u * lane + 2u], h3 = hist[4u * lane + 3u];
    uint32_t incl = h0 + h1 + h2 + h3;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d) incl += up;
    }
    const unsigned long long reached = __ballot(incl >= want);
    const uint32_t first = (uint32_t)__ffsll((long long)reached) - 1u;      // (reached != 0: want <= the total)
    const uint32_t excl = incl - (h0 + h1 + h2 + h3);
    uint32_t b = __shfl(excl, first);
    const uint32_t g0 = __shfl(h0, first), g1 = __shfl(h1, first), g2 = __shfl(h2, first);
    uint32_t bin = 4u * first;
    if (b + g0 < want) { b += g0; bin++;
        if (b + g1 < want) { b += g1; bin++;
            if (b + g2 < want) { b += g2; bin++; } } }
    below = b;
    return bin;
}

__device__ __forceinline__ KmmWalk kmm_walk_of(const KmmExtractArgs &A, uint32_t sid) {
    KmmWalk W;
    W.res = A.res + (size_t)A.off4[sid] * 4u;
    W.L = A.len[sid];
    W.k = A.k;
    W.n_win = W.L >= (uint32_t)A.k ? W.L - (uint32_t)A.k + 1u : 0u;
    W.base = (uint32_t)A.alph_size - 1u;
    W.x = W.base;
    W.seed = A.seed;
    return W;
}

// Pass 1 of the extraction: per sequence the selection rule {t, surplus, considered} and the number of records it will write
__global__ __launch_bounds__(64) void kmm_count_kernel(KmmExtractArgs A) {
    __shared__ uint32_t hist[256];
    __shared__ uint8_t red_tab[32];
    __shared__ uint8_t stage[96];
    const uint32_t sid = blockIdx.x, lane = threadIdx.x;
    if (sid >= A.n) return;
    const KmmWalk W = kmm_walk_of(A, sid);
    if (lane < 21u) red_tab[lane] = A.reduce[lane];
    for (uint32_t i = lane; i < 256u; i += 64u) hist[i] = 0;
    __syncthreads();
    const uint32_t rounds = (W.n_win + 63u) / 64u;
    uint32_t count = 0;
    unsigned long long idx;
    uint32_t score;
    for (uint32_t c = 0; c < rounds; c++) {
        kmm_stage(W, c, red_tab, stage, lane);
        __syncthreads();
        const bool ok = kmm_window(W, c, stage, lane, idx, score);
        if (ok) atomicAdd(&hist[score >> 8], 1u);
        count += (uint32_t)__popcll(__ballot(ok));
        __syncthreads();
    }
    // kmermatcher.cpp:239: an int plus a float product, in float (no fused multiply-add), cut to a size_t
    const float want_f = __fadd_rn((float)(A.kmers_per_seq - 1), __fmul_rn(A.kmers_per_seq_scale, (float)W.L));
    const unsigned long long want_ll = (unsigned long long)want_f;
    const uint32_t considered = want_ll < (unsigned long long)count ? (uint32_t)want_ll : count;
    uint32_t t = 0, surplus = 0, n_sel = 0;
    if (considered == count) {      // every window is taken: the largest score is the threshold bin and it has no surplus
        t = 0xFFFFu;
        n_sel = count;
    } else if (considered > 0) {
        uint32_t below_hi = 0, below_lo = 0;
        const uint32_t hi = kmm_find_bin(hist, considered, lane, below_hi);
        __syncthreads();
        for (uint32_t i = lane; i < 256u; i += 64u) hist[i] = 0;
        __syncthreads();
        for (uint32_t c = 0; c < rounds; c++) {
            kmm_stage(W, c, red_tab, stage, lane);
            __syncthreads();
            const bool ok = kmm_window(W, c, stage, lane, idx, score);
            if (ok && (score >> 8) == hi) atomicAdd(&hist[score & 255u], 1u);
            __syncthreads();
        }
        const uint32_t lo = kmm_find_bin(hist, considered - below_hi, lane, below_lo);
        const uint32_t in_bin = hist[lo];
        t = (hi << 8) | lo;
        surplus = below_hi + below_lo + in_bin - considered;      // tooMuchElemInLastBin
        // windows below t, plus the first `surplus` of bin t (all of it without a surplus), cut at `considered`
        const uint32_t flagged = surplus == 0 ? considered : considered + 2u * surplus - in_bin;
        n_sel = flagged < considered ? flagged : considered;
    }
    if (lane == 0) {
        A.rule[sid] = make_uint4(t, surplus, considered, 0u);
        A.count[sid] = 1u + n_sel;      // the identity record
    }
}

// Pass 2: the records, at rec_off[sid]: the identity record, then the selected windows in position order
__global__ __launch_bounds__(64) void kmm_write_kernel(KmmExtractArgs A) {
    __shared__ uint8_t red_tab[32];
    __shared__ uint8_t stage[96];
    const uint32_t sid = blockIdx.x, lane = threadIdx.x;
    if (sid >= A.n) return;
    const KmmWalk W = kmm_walk_of(A, sid);
    if (lane < 21u) red_tab[lane] = A.reduce[lane];
    __syncthreads();
    const uint4 rule = A.rule[sid];
    const uint32_t t = rule.x, surplus = rule.y, considered = rule.z;
    const uint32_t base = A.rec_off[sid];
    const unsigned long long tag = ((unsigned long long)(KMM_LEN_MASK - W.L) << KMM_LEN_SHIFT) | ((unsigned long long)sid << KMM_ID_SHIFT);
    const uint32_t rounds = (W.L + 63u) / 64u;      // every residue passes through stage[lane] once: the sequence hash rides along
    unsigned long long seq_hash = 0;
    uint32_t eq_seen = 0, sel_seen = 0;
    for (uint32_t c = 0; c < rounds; c++) {
        kmm_stage(W, c, red_tab, stage, lane);
        __syncthreads();
        // Util::hash: h = h * 31 + r over the residues of this round
        const uint32_t m = W.L - c * 64u < 64u ? W.L - c * 64u : 64u;
        unsigned long long part = lane < m ? (unsigned long long)stage[lane] * pow31(m - 1u - lane) : 0ull;
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
        seq_hash = seq_hash * pow31(m) + part;
        if (sel_seen < considered) {
            unsigned long long idx;
            uint32_t score;
            const bool ok = kmm_window(W, c, stage, lane, idx, score);
            const bool eq = ok && score == t;
            const unsigned long long eq_mask = __ballot(eq);
            const bool take = ok && (score < t || (eq && (surplus == 0 || eq_seen + lanes_below(eq_mask, lane) < surplus)));
            const unsigned long long take_mask = __ballot(take);
            const uint32_t rank = sel_seen + lanes_below(take_mask, lane);
            if (take && rank < considered) {
                A.rec_kmer[base + 1u + rank] = idx;
                A.rec_val[base + 1u + rank] = tag | (unsigned long long)(c * 64u + lane);
            }
            eq_seen += (uint32_t)__popcll(eq_mask);
            sel_seen += (uint32_t)__popcll(take_mask);
        }
        __syncthreads();
    }
    if (lane == 0) {
        A.rec_kmer[base] = xxh64_u64(seq_hash, W.seed);
        A.rec_val[base] = tag;
    }
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

struct GroupHead {      // i where a k-mer's records begin, else 0: its maximum scan is every record's group start
    const unsigned long long *kmer;
    __device__ uint32_t operator()(uint32_t i) const { return i > 0 && kmer[i] != kmer[i - 1] ? i : 0u; }
};

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

struct GroupEmit {      // 1 when record i emits a (representative, member, diagonal), kmermatcher.cpp:633-672
    KmmGroupArgs A;
    __device__ uint32_t operator()(uint32_t i) const {
        const uint32_t g = A.group_start[i];
        if (g == i && (i + 1u == A.n_records || A.kmer[i + 1u] != A.kmer[i])) return 0u;      // a group of one
        const unsigned long long rep = A.val[g], me = A.val[i];
        const int q_len = (int)val_len(rep), t_len = (int)val_len(me);
        const int diagonal = val_pos(rep) - val_pos(me);
        const bool extendable = diagonal < 0 || diagonal > q_len - t_len;
        const bool coverable = can_be_covered(A.cov_thr, A.cov_mode, (float)q_len, (float)t_len);
        return ((!A.only_extendable && coverable) || (A.only_extendable && extendable)) ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void kmm_emit_kernel(KmmGroupArgs A, const uint32_t *emit_at, unsigned long long *pair, uint16_t *diag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_records) return;
    const GroupEmit E{A};
    if (!E(i)) return;
    const unsigned long long rep = A.val[A.group_start[i]], me = A.val[i];
    int diagonal = val_pos(rep) - val_pos(me);
    uint32_t a = val_id(rep), b = val_id(me);
    if (val_len(rep) < val_len(me) && A.cov_mode == 1) {      // :679-683
        const uint32_t s = a; a = b; b = s;
        diagonal = -diagonal;
    }
    const uint32_t at = emit_at[i];
    pair[at] = ((unsigned long long)a << 32) | b;
    diag[at] = (uint16_t)((uint32_t)diagonal ^ 0x8000u);      // the short, biased: the radix sort orders it as a signed value
}

// ---- vote --------------------------------------------------------------------------------------------------------------------------
struct PairKept {      // 1 where a (representative, member) run with member != representative begins
    const unsigned long long *pair;
    __device__ uint32_t operator()(uint32_t i) const {
        const unsigned long long p = pair[i];
        return (i == 0 || pair[i - 1] != p) && (uint32_t)(p >> 32) != (uint32_t)p ? 1u : 0u;
    }
};

// writeKmerMatcherResult (:1614-1655) per kept run: score = its length, diagonal = the value with the longest run, the last on a tie
__global__ __launch_bounds__(256) void kmm_vote_kernel(const unsigned long long *pair, const uint16_t *diag, uint32_t n_pairs, const uint32_t *kept_at,
                                                        mmgpu_pf_hit *records, uint32_t *kept_rep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pairs) return;
    const PairKept K{pair};
    if (!K(i)) return;
    const unsigned long long p = pair[i];
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
    h.score = (int32_t)score;
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
    hipError_t e = scan_u32<GroupHead, OpMax, false>(GroupHead{A.kmer}, A.n_records, tile_sum, A.group_start, s);
    if (e != hipSuccess) return e;
    return scan_u32<GroupEmit, OpSum, true>(GroupEmit{A}, A.n_records, tile_sum, emit_at, s);
}

hipError_t launch_kmm_emit(const KmmGroupArgs &A, const uint32_t *emit_at, unsigned long long *pair, uint16_t *diag, hipStream_t s) {
    if (A.n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(kmm_emit_kernel, dim3((A.n_records + 255u) / 256u), dim3(256), 0, s, A, emit_at, pair, diag);
    return hipGetLastError();
}

// kept_at[n_pairs + 1] (kept_at[n_pairs] = the number of kept runs)
hipError_t launch_kmm_vote_scan(const unsigned long long *pair, uint32_t n_pairs, uint32_t *tile_sum, uint32_t *kept_at, hipStream_t s) {
    return scan_u32<PairKept, OpSum, true>(PairKept{pair}, n_pairs, tile_sum, kept_at, s);
}

hipError_t launch_kmm_vote(const unsigned long long *pair, const uint16_t *diag, uint32_t n_pairs, const uint32_t *kept_at, uint32_t n_kept, uint32_t n,
                           uint32_t *kept_rep, unsigned long long *offsets, mmgpu_pf_hit *records, hipStream_t s) {
    if (n_pairs) hipLaunchKernelGGL(kmm_vote_kernel, dim3((n_pairs + 255u) / 256u), dim3(256), 0, s, pair, diag, n_pairs, kept_at, records, kept_rep);
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
