// The targets of a masked alignment batch (mmgpu_sw_prepare_masked): every pair's private copy of its target, gathered out of the
// resident database with the pair's spans overwritten by the mask letter.
//
// Alignment::computeAlternativeAlignment (Alignment.cpp:569-601) overwrites [dbStartPos, dbEndPos) of the target with X and calls
// Matcher::getSWResult again, up to --alt-ali times per accepted hit.  Here the targets stay resident and unchanged: a batch of such
// second alignments gets an arena of copies in the layout the alignment kernels read (mmgpu_load_targets: every copy at a 4-byte
// boundary, pad letters behind its last residue), and the kernels are handed the arena in place of the database.
//
// sw_mask_gather_kernel: one wavefront per pair, four per workgroup.  The lanes stride over the dwords of the copy; a dword is
// loaded from the resident target, the bytes of [t_from, t_to) that fall into it are replaced through one mask, and it is stored.
// The span list is the same for all lanes: each lane loads one span, the loop over the spans broadcasts them lane by lane
// (v_readlane), 64 per pass; a longer list takes further passes over the copy itself.  The pad bytes of the last dword are the
// resident target's own (spans end at the target's length at the latest), the arena's padding is the memset before the launch.
//
// Not measured: lists beyond 64 spans.  Every further 64 spans re-read and re-store the whole copy, and inside a trip every span of
// the pass costs two v_readlane and a scalar branch whether it touches the trip's 256 residues or not - hundreds of spans on a
// 65 535-residue target make that many passes of 256 trips.  --alt-ali accumulates one span per round (N <= ~10 in practice), which
// is the case this form is written for; spans staged in LDS and filtered per trip would be the form for long lists.
#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

// the bytes [0, k) of a dword, k = 0 .. 4 (no shift by 32)
__device__ __forceinline__ uint32_t below_byte(int k) { return k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u; }

__global__ __launch_bounds__(256) void sw_mask_gather_kernel(SwMaskGatherArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (pair >= A.n_pairs) return;
    const uint32_t t = A.src_id[pair];
    const uint32_t len = A.src_len[t];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.src_res) + A.src_off4[t];
    uint32_t *dst = reinterpret_cast<uint32_t *>(A.dst_res) + A.dst_off4[pair];
    const uint32_t n_dw = (len + 3u) >> 2, trips = (n_dw + 63u) >> 6;      // a 65 535-residue target: 256 trips
    const uint32_t s_end = A.span_off[pair + 1];
    const uint32_t fill = A.mask_letter * 0x01010101u;
    uint32_t s0 = A.span_off[pair];
    const uint32_t *from = src;
    do {
        const uint32_t cnt = min(s_end - s0, 64u);
        int my_from = 0, my_to = 0;
        if (lane < cnt) {
            const mmgpu_sw_span sp = A.spans[s0 - A.span_base + lane];
            my_from = (int)sp.t_from;
            my_to = (int)min(sp.t_to, len);
        }
        for (uint32_t trip = 0; trip < trips; trip++) {
            const uint32_t i = trip * 64u + lane;
            const bool live = i < n_dw;
            uint32_t v = live ? from[i] : 0u;
            const uint32_t first = trip * 256u, base = i * 4u;      // residues [first, first + 256) are this trip's
            uint32_t m = 0;
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane(my_from, (int)k), e = (uint32_t)__builtin_amdgcn_readlane(my_to, (int)k);
                if (e <= first || f >= first + 256u || e <= f) continue;      // (the same for all lanes)
                // bytes [lo, hi) of the dword (positions are below 2^16: signed differences)
                const int lo = max(0, min((int)f - (int)base, 4)), hi = max(0, min((int)e - (int)base, 4));
                m |= below_byte(hi) & ~below_byte(lo);      // (nothing where hi <= lo)
            }
            v = (v & ~m) | (fill & m);
            if (live) dst[i] = v;
        }
        from = dst;      // a list beyond 64 spans: the next pass masks the copy (every lane re-reads what it stored itself)
        s0 += cnt;
    } while (s0 < s_end);
}

}  // namespace

hipError_t launch_sw_mask_gather(const SwMaskGatherArgs &A, hipStream_t stream) {
    if (A.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_mask_gather_kernel, dim3((A.n_pairs + 3u) / 4u), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace mmgpu
