// linclust's k-mer matching stage over a nucleotide database (include/mmgpu.h, "linclust's k-mer matching stage, nucleotides"): the
// extraction.  One wavefront per sequence, the count and the write pass of kmm_device.h over the walk below; everything behind the
// extraction is kmermatch_kernel.hip's, with its strand flag set.
//
//   staging      a round is 64 windows, i.e. 64 + k - 1 <= 94 residues.  Lanes 0 .. 23 read a dword of four residues each and leave
//                them in LDS packed: 2 bits a residue (residue i of the round at bits 2i of a 192-bit string) and beside it a bit a
//                residue that is set for N and behind the sequence's end.
//   window       a lane reads the two 64-bit words its window lies in and shifts: v = sum r[i] << 2i.  That is the reverse
//                complement but for the complement itself (A<->T, C<->G are code ^ 2, i.e. an XOR with 0xAAAA...), and the index
//                proper (first residue in the highest bits) is v with its 2-bit groups in reverse order: a 64-bit bit reversal, a
//                swap of the two bits of each pair, a shift by 64 - 2k.  The N test is a mask of k flag bits.  No loop over k.
//   strand       the smaller of index and reverse complement is hashed and stored, bit 63 set when it is the index itself; the stored
//                position of a window taken as its reverse complement is its position on the other strand, L - p - k.  A window that
//                equals its reverse complement (even k only) does not count.
// Scores are recomputed per pass, as the protein extraction does: the count pass that kept them in LDS for its second histogram level
// (a launch per length class) measured 0.86 ms against 0.75 ms of this one on the benchmark database.
#include "kmm_device.h"

namespace mmgpu {

namespace {

constexpr uint32_t NM_DWORDS = 24;      // dwords of residues a round stages: 96 residues >= 64 + KMM_MAX_K - 1

struct NuclWalk {
    const uint8_t *res;      // the sequence's residues (4-byte aligned)
    uint32_t L, n_win;
    int k;
    unsigned long long seed;
    unsigned long long *bits;      // LDS [3]: the staged round, 2 bits a residue
    unsigned long long *flag;      // LDS [2]: a bit a residue: N, or behind the sequence's end

    __device__ __forceinline__ void stage(uint32_t c, uint32_t lane) {
        const uint32_t at = c * 64u + 4u * lane;
        uint32_t code = 0, nib = 0;
        if (lane < NM_DWORDS) {
            const uint32_t d = at < L ? *reinterpret_cast<const uint32_t *>(res + at) : 0u;      // (a sequence's storage ends on a dword)
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t r = (d >> (8u * i)) & 255u;
                code |= (r & 3u) << (2u * i);
                nib |= (r >= 4u || at + i >= L ? 1u : 0u) << i;
            }
        }
        const uint32_t pair = nib | ((uint32_t)__shfl_down((int)nib, 1) << 4);      // two lanes' flags make a byte
        if (lane < NM_DWORDS) {
            reinterpret_cast<uint8_t *>(bits)[lane] = (uint8_t)code;
            if (!(lane & 1u)) reinterpret_cast<uint8_t *>(flag)[lane >> 1] = (uint8_t)pair;
        }
    }

    // the window at position c * 64 + lane: false when there is none, it holds an N or it is its own reverse complement
    __device__ __forceinline__ bool window(uint32_t c, uint32_t lane, unsigned long long &kmer, uint32_t &pos, uint32_t &score) const {
        const uint32_t s = 2u * lane, w = s >> 6, sh = s & 63u;
        unsigned long long v = bits[w] >> sh, nv = flag[0] >> lane;
        if (sh) v |= bits[w + 1u] << (64u - sh);
        if (lane) nv |= flag[1] << (64u - lane);
        const unsigned long long mask = (1ull << (2 * k)) - 1ull;      // k <= 31: bit 63 stays free for the strand
        v &= mask;
        const unsigned long long rev = v ^ (0xAAAAAAAAAAAAAAAAull & mask);      // Util::revComplement
        unsigned long long idx = __brevll(v);
        idx = ((idx >> 1) & 0x5555555555555555ull) | ((idx & 0x5555555555555555ull) << 1);
        idx >>= 64 - 2 * k;                                                     // Indexer::computeKmerIdx
        const bool pick_reverse = rev < idx;
        const unsigned long long canonical = pick_reverse ? rev : idx;
        const uint32_t p = c * 64u + lane;
        kmer = pick_reverse ? canonical : canonical | (1ull << 63);
        pos = pick_reverse ? L - p - (uint32_t)k : p;
        score = (uint32_t)(xxh64_u64(canonical, seed) & 0xFFFFull);
        return !(nv & ((1ull << k) - 1ull)) && rev != idx;      // (a window that reaches behind the end holds a flagged residue)
    }

    __device__ __forceinline__ uint32_t residue(uint32_t lane) const {
        return (flag[0] >> lane) & 1ull ? 4u : (uint32_t)(bits[lane >> 5] >> (2u * (lane & 31u))) & 3u;
    }
};

__device__ __forceinline__ NuclWalk nm_walk_of(const NuclExtractArgs &A, uint32_t sid, unsigned long long *bits, unsigned long long *flag) {
    NuclWalk W;
    W.res = A.res + (size_t)A.off4[sid] * 4u;
    W.L = A.len[sid];
    W.k = A.k;
    W.n_win = W.L >= (uint32_t)A.k ? W.L - (uint32_t)A.k + 1u : 0u;
    W.seed = A.seed;
    W.bits = bits;
    W.flag = flag;
    return W;
}

__global__ __launch_bounds__(64) void nm_count_kernel(NuclExtractArgs A) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long bits[3], flag[2];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= A.n) return;
    const uint32_t sid = A.order[blockIdx.x];
    if (lane < 2u) flag[lane] = 0;
    NuclWalk W = nm_walk_of(A, sid, bits, flag);
    kmm_count_body(W, hist, A.kmers_per_seq, A.kmers_per_seq_scale, lane, &A.rule[sid], &A.count[sid]);
}

__global__ __launch_bounds__(64) void nm_write_kernel(NuclExtractArgs A) {
    __shared__ unsigned long long bits[3], flag[2];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= A.n) return;
    const uint32_t sid = A.order[blockIdx.x];
    if (lane < 2u) flag[lane] = 0;
    __syncthreads();
    NuclWalk W = nm_walk_of(A, sid, bits, flag);
    kmm_write_body(W, A.rule[sid], sid, A.rec_off[sid], lane, A.rec_kmer, A.rec_val);
}

}  // namespace

hipError_t launch_nuclmatch_extract_count(const NuclExtractArgs &A, hipStream_t s) {
    if (A.n == 0) return hipSuccess;
    hipLaunchKernelGGL(nm_count_kernel, dim3(A.n), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_nuclmatch_extract_write(const NuclExtractArgs &A, hipStream_t s) {
    if (A.n == 0) return hipSuccess;
    hipLaunchKernelGGL(nm_write_kernel, dim3(A.n), dim3(64), 0, s, A);
    return hipGetLastError();
}

}  // namespace mmgpu
