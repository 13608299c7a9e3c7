// What the two extractions of linclust's k-mer matching stage share (kmermatch_kernel.hip: amino acids, nuclmatch_kernel.hip:
// nucleotides): the hash, the search in a 256-bin histogram, and the bodies of the count and the write kernel over a `Walk` - what
// one wavefront holds of its sequence while it walks the windows in rounds of 64:
//     uint32_t L, n_win; unsigned long long seed;
//     void stage(c, lane)                                  round c's residues into LDS (the body synchronises behind it)
//     bool window(c, lane, kmer, pos, score)               the window at position c * 64 + lane: false when it does not count; the
//                                                          k-mer and the position as the record stores them, the 16-bit score
//     uint32_t residue(lane)                               the staged residue at position c * 64 + lane as Util::hash reads it
#ifndef MMGPU_KMM_DEVICE_H
#define MMGPU_KMM_DEVICE_H
#include "mmgpu_internal.h"

namespace mmgpu {

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

// Pass 1 of an extraction, one wavefront: the selection rule {t, surplus, considered} of the sequence and the number of records it
// will write.  hist[256] is LDS.  Both histogram levels walk the sequence: keeping the first walk's scores in LDS for the second was
// built and measured for the nucleotide walk and lost.
template <class Walk>
__device__ __forceinline__ void kmm_count_body(Walk &W, uint32_t *hist, int kmers_per_seq, float kmers_per_seq_scale, uint32_t lane, uint4 *rule,
                                               uint32_t *n_records) {
    for (uint32_t i = lane; i < 256u; i += 64u) hist[i] = 0;
    __syncthreads();
    const uint32_t rounds = (W.n_win + 63u) / 64u;
    uint32_t count = 0;
    unsigned long long kmer;
    uint32_t pos, score;
    for (uint32_t c = 0; c < rounds; c++) {
        W.stage(c, lane);
        __syncthreads();
        const bool ok = W.window(c, lane, kmer, pos, score);
        if (ok) atomicAdd(&hist[score >> 8], 1u);
        count += (uint32_t)__popcll(__ballot(ok));
        __syncthreads();
    }
    // kmermatcher.cpp:239: an int plus a float product, in float (no fused multiply-add), cut to a size_t
    const float want_f = __fadd_rn((float)(kmers_per_seq - 1), __fmul_rn(kmers_per_seq_scale, (float)W.L));
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
            W.stage(c, lane);
            __syncthreads();
            const bool ok = W.window(c, lane, kmer, pos, score);
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
        *rule = make_uint4(t, surplus, considered, 0u);
        *n_records = 1u + n_sel;      // the identity record
    }
}

// Pass 2: the records of sequence `sid` at rec_kmer / rec_val[base ..]: the identity record, then the selected windows in position order
template <class Walk>
__device__ __forceinline__ void kmm_write_body(Walk &W, uint4 rule, uint32_t sid, uint32_t base, uint32_t lane, unsigned long long *rec_kmer,
                                               unsigned long long *rec_val) {
    const uint32_t t = rule.x, surplus = rule.y, considered = rule.z;
    const unsigned long long tag = ((unsigned long long)(KMM_LEN_MASK - W.L) << KMM_LEN_SHIFT) | ((unsigned long long)sid << KMM_ID_SHIFT);
    const uint32_t rounds = (W.L + 63u) / 64u;      // every residue passes through the staging once: the sequence hash rides along
    unsigned long long seq_hash = 0;
    uint32_t eq_seen = 0, sel_seen = 0;
    for (uint32_t c = 0; c < rounds; c++) {
        W.stage(c, lane);
        __syncthreads();
        // Util::hash: h = h * 31 + r over the residues of this round
        const uint32_t m = W.L - c * 64u < 64u ? W.L - c * 64u : 64u;
        unsigned long long part = lane < m ? (unsigned long long)W.residue(lane) * pow31(m - 1u - lane) : 0ull;
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
        seq_hash = seq_hash * pow31(m) + part;
        if (sel_seen < considered) {
            unsigned long long kmer;
            uint32_t pos, score;
            const bool ok = W.window(c, lane, kmer, pos, score);
            const bool eq = ok && score == t;
            const unsigned long long eq_mask = __ballot(eq);
            const bool take = ok && (score < t || (eq && (surplus == 0 || eq_seen + lanes_below(eq_mask, lane) < surplus)));
            const unsigned long long take_mask = __ballot(take);
            const uint32_t rank = sel_seen + lanes_below(take_mask, lane);
            if (take && rank < considered) {
                rec_kmer[base + 1u + rank] = kmer;
                rec_val[base + 1u + rank] = tag | (unsigned long long)pos;
            }
            eq_seen += (uint32_t)__popcll(eq_mask);
            sel_seen += (uint32_t)__popcll(take_mask);
        }
        __syncthreads();
    }
    if (lane == 0) {
        rec_kmer[base] = xxh64_u64(seq_hash, W.seed);
        rec_val[base] = tag;
    }
}

}  // namespace mmgpu
#endif
