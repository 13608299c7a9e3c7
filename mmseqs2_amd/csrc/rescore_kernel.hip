// Ungapped diagonal rescoring for gfx950 / CDNA4 (include/mmgpu.h, "ungapped diagonal rescoring"): one record per hit of a
// prefilter result list, as DistanceCalculator::computeUngappedAlignment computes it (DistanceCalculator.h:93-200).
//
// Mapping.  RESCORE_GROUP = 16 lanes (one DPP row) share a hit, four hits a wavefront: a diagonal of a few hundred cells gives every
// lane a run of a dozen or two.  Lane l walks cells [l * run, (l + 1) * run) of the diagonal, run = ceil(len / 16) rounded up to
// RESCORE_STEP = 4, so that a run starts on a dword of the side that is aligned at cell 0 (the target for D >= 0, the query for
// D < 0: both are stored on 4-byte boundaries); the other side is read as two neighbouring dwords and shifted.  A run is folded cell
// by cell into a RescoreSummary, the 16 summaries are combined in diagonal order with four xor exchanges inside the row, and every
// lane then holds the summary of the whole diagonal.  The loop over the candidate diagonals of a hit is uniform over its group.
//
// The summary of a run of cells [s, e) with P[i] = c[s] + .. + c[i] and P[s - 1] = 0:
//     sum                      P[e - 1]
//     mn, mn_pos               min of P over s - 1 .. e - 1, the LATEST position that attains it   (the reference resets on score <= 0)
//     mx, mx_pos               max of P over s .. e - 1, the EARLIEST position                       (it updates on a greater score only)
//     best, best_end/_start    max over i in s .. e - 1 of P[i] - min(P[s - 1 .. i]), the earliest i, 1 + the latest argmin before it
//     matches                  cells with equal residues
// rescore_combine(A, B) is the summary of A's run followed by B's; every mode's fold and the exchange between lanes call it.  For
// an i in B the running score is max(A.sum - A.mn + P_B[i], P_B[i] - min_B(.. i)): its maximum over B is max(A.sum - A.mn + B.mx,
// B.best).  When the first term wins strictly the minimum lies in A (start = A.mn_pos + 1) and the end is B.mx_pos; when the second
// wins strictly it is B's own segment; when they tie the earlier end wins, and at the same end the minimum is attained in A and in
// B alike, so the latest - B's - starts the segment.  A.best wins a tie against anything in B: it ends earlier.
// Positions are offsets along the diagonal, so no summary is shifted when runs are joined.  No atomics; records leave with plain
// vector stores.
#include "mmgpu_internal.h"

namespace mmgpu {

namespace {

constexpr int RESCORE_NONE = -(1 << 30);      // the maximum over no position (far below any sum of int8 cells; adding a sum does not wrap)

struct RescoreSummary {
    int sum;
    int mn, mn_pos;
    int mx, mx_pos;
    int best, best_end, best_start;
    int matches;
};

// the run [pos, pos)
__device__ __forceinline__ RescoreSummary rescore_empty(int pos) { return {0, 0, pos - 1, RESCORE_NONE, pos, RESCORE_NONE, pos, pos, 0}; }

// the run of the one cell at pos
__device__ __forceinline__ RescoreSummary rescore_cell(int c, int pos, int equal) {
    const bool low = c <= 0;
    const int mn = low ? c : 0, mn_pos = low ? pos : pos - 1;
    return {c, mn, mn_pos, c, pos, c - mn, pos, mn_pos + 1, equal};
}

__device__ __forceinline__ RescoreSummary rescore_combine(const RescoreSummary &A, const RescoreSummary &B) {
    RescoreSummary R;
    R.sum = A.sum + B.sum;
    R.matches = A.matches + B.matches;
    const int b_mn = A.sum + B.mn, b_mx = A.sum + B.mx;
    const bool mn_in_b = b_mn <= A.mn;      // the latest minimum
    R.mn = mn_in_b ? b_mn : A.mn;
    R.mn_pos = mn_in_b ? B.mn_pos : A.mn_pos;
    const bool mx_in_b = b_mx > A.mx;       // the earliest maximum
    R.mx = mx_in_b ? b_mx : A.mx;
    R.mx_pos = mx_in_b ? B.mx_pos : A.mx_pos;
    const int cross = A.sum - A.mn + B.mx;
    const bool crossing = cross > B.best || (cross == B.best && B.mx_pos < B.best_end);
    const int in_b = crossing ? cross : B.best;
    const int in_b_end = crossing ? B.mx_pos : B.best_end;
    const int in_b_start = crossing ? A.mn_pos + 1 : B.best_start;
    const bool keep_a = A.best >= in_b;
    R.best = keep_a ? A.best : in_b;
    R.best_end = keep_a ? A.best_end : in_b_end;
    R.best_start = keep_a ? A.best_start : in_b_start;
    return R;
}

__device__ __forceinline__ RescoreSummary rescore_exchange(const RescoreSummary &S, int off) {
    RescoreSummary O;
    O.sum = __shfl_xor(S.sum, off, RESCORE_GROUP);
    O.mn = __shfl_xor(S.mn, off, RESCORE_GROUP);
    O.mn_pos = __shfl_xor(S.mn_pos, off, RESCORE_GROUP);
    O.mx = __shfl_xor(S.mx, off, RESCORE_GROUP);
    O.mx_pos = __shfl_xor(S.mx_pos, off, RESCORE_GROUP);
    O.best = __shfl_xor(S.best, off, RESCORE_GROUP);
    O.best_end = __shfl_xor(S.best_end, off, RESCORE_GROUP);
    O.best_start = __shfl_xor(S.best_start, off, RESCORE_GROUP);
    O.matches = __shfl_xor(S.matches, off, RESCORE_GROUP);
    return O;
}

// the four residues from byte `at` of a sequence stored on a 4-byte boundary; an unaligned `at` reads the next dword as well
__device__ __forceinline__ uint32_t rescore_load4(const uint32_t *seq, uint32_t at) {
    const uint32_t w = at >> 2, m = at & 3u;
    const uint32_t lo = seq[w];
    if (m == 0) return lo;
    const uint32_t hi = seq[w + 1];
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * m));
}

// one diagonal of one hit over the group's 16 lanes -> its summary in every lane.  q_at / t_at: where cell 0 lies in each sequence
template <int MODE>
__device__ __forceinline__ RescoreSummary rescore_diagonal(const uint32_t *q, uint32_t q_at, const uint32_t *t, uint32_t t_at, uint32_t len,
                                                           const int8_t *s_mat, int alphabet, uint32_t lane) {
    const uint32_t per = (len + RESCORE_GROUP - 1) / RESCORE_GROUP;
    const uint32_t run = (per + RESCORE_STEP - 1) / RESCORE_STEP * RESCORE_STEP;
    const uint32_t lo = min(lane * run, len), hi = min(lo + run, len);
    RescoreSummary S = rescore_empty((int)lo);
    for (uint32_t c4 = lo; c4 < hi; c4 += RESCORE_STEP) {
        const uint32_t qw = rescore_load4(q, q_at + c4), tw = rescore_load4(t, t_at + c4);
#pragma unroll
        for (int j = 0; j < RESCORE_STEP; j++) {
            if (c4 + j < hi) {
                const uint32_t ql = (qw >> (8 * j)) & 255u, tl = (tw >> (8 * j)) & 255u;
                const int c = MODE == MMGPU_RESCORE_HAMMING ? 0 : (int)s_mat[ql * (uint32_t)alphabet + tl];
                S = rescore_combine(S, rescore_cell(c, (int)(c4 + j), ql == tl));
            }
        }
    }
#pragma unroll
    for (int off = 1; off < RESCORE_GROUP; off <<= 1) {
        const RescoreSummary O = rescore_exchange(S, off);
        S = (lane & off) ? rescore_combine(O, S) : rescore_combine(S, O);
    }
    return S;
}

// equal residues in cells [start, end] of a diagonal, summed over the group
__device__ __forceinline__ uint32_t rescore_identities(const uint32_t *q, uint32_t q_at, const uint32_t *t, uint32_t t_at, uint32_t start,
                                                       uint32_t end, uint32_t lane) {
    uint32_t n = 0;
    for (uint32_t c4 = (start & ~(uint32_t)(RESCORE_STEP - 1)) + lane * RESCORE_STEP; c4 <= end; c4 += RESCORE_GROUP * RESCORE_STEP) {
        const uint32_t qw = rescore_load4(q, q_at + c4), tw = rescore_load4(t, t_at + c4);
#pragma unroll
        for (int j = 0; j < RESCORE_STEP; j++) {
            const uint32_t pos = c4 + j;
            n += (pos >= start && pos <= end && ((qw >> (8 * j)) & 255u) == ((tw >> (8 * j)) & 255u)) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = 1; off < RESCORE_GROUP; off <<= 1) n += __shfl_xor(n, off, RESCORE_GROUP);
    return n;
}

template <int MODE>
__global__ __launch_bounds__(RESCORE_THREADS) void rescore_kernel(RescoreArgs A) {
    __shared__ int8_t s_mat[32 * 32];
    for (int i = threadIdx.x; i < A.alphabet * A.alphabet; i += RESCORE_THREADS) s_mat[i] = A.mat[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x % RESCORE_GROUP;
    const uint64_t hit = ((uint64_t)blockIdx.x * RESCORE_THREADS + threadIdx.x) / RESCORE_GROUP;
    if (hit >= A.n_hits) return;      // (a whole group leaves)
    const mmgpu_rescore_pair pair = A.pairs[hit];
    const uint32_t qi = A.hit_query[hit];
    const uint32_t *q = reinterpret_cast<const uint32_t *>(A.q_res) + A.q_off4[qi];
    const uint32_t *t = reinterpret_cast<const uint32_t *>(A.t_res) + A.t_off4[pair.target];
    const int64_t qlen = A.q_len[qi], tlen = A.t_len[pair.target], d = pair.diagonal;

    mmgpu_rescore_hit best = {0, 0, 0u, -1, -1, 0u};      // LocalAlignment()
    auto candidate = [&](int64_t D) {      // a valid one
        const uint32_t q_at = D >= 0 ? (uint32_t)D : 0u, t_at = D >= 0 ? 0u : (uint32_t)(-D);
        const uint32_t len = (uint32_t)(D >= 0 ? min(tlen, qlen - D) : min(tlen + D, qlen));
        const RescoreSummary S = rescore_diagonal<MODE>(q, q_at, t, t_at, len, s_mat, A.alphabet, lane);
        const int score = MODE == MMGPU_RESCORE_HAMMING ? S.matches : max(S.best, 0);
        if (score > best.score) {
            best.score = score;
            best.diagonal = (int32_t)D;
            best.diag_len = len;
            if (MODE == MMGPU_RESCORE_ALIGNMENT) {
                best.start = S.best_start;
                best.end = S.best_end;
            }
        }
    };
    // the reference's order, without the candidates that are valid for neither sequence (they score 0 and replace nothing):
    // d - 65536 k while it still reaches into the target, then d + 65536 k while it still reaches into the query
    for (int64_t k = 1; 65536 * k - d < tlen; k++) candidate(d - 65536 * k);
    for (int64_t k = 0; d + 65536 * k < qlen; k++) candidate(d + 65536 * k);

    if (MODE == MMGPU_RESCORE_HAMMING) best.ident = (uint32_t)best.score;
    if (MODE == MMGPU_RESCORE_ALIGNMENT && best.score > 0) {
        const int64_t D = best.diagonal;
        best.ident = rescore_identities(q, D >= 0 ? (uint32_t)D : 0u, t, D >= 0 ? 0u : (uint32_t)(-D), (uint32_t)best.start, (uint32_t)best.end, lane);
    }
    if (lane == 0) A.out[hit] = best;
}

}  // namespace

hipError_t launch_rescore(const RescoreArgs &A, int mode, hipStream_t stream) {
    if (A.n_hits == 0) return hipSuccess;
    if (A.alphabet > 32) return hipErrorInvalidValue;      // the matrix must fit its LDS copy
    const uint64_t groups_per_block = RESCORE_THREADS / RESCORE_GROUP;
    const dim3 grid((uint32_t)((A.n_hits + groups_per_block - 1) / groups_per_block)), block(RESCORE_THREADS);
    switch (mode) {
    case MMGPU_RESCORE_HAMMING: hipLaunchKernelGGL(rescore_kernel<MMGPU_RESCORE_HAMMING>, grid, block, 0, stream, A); break;
    case MMGPU_RESCORE_SUBSTITUTION: hipLaunchKernelGGL(rescore_kernel<MMGPU_RESCORE_SUBSTITUTION>, grid, block, 0, stream, A); break;
    case MMGPU_RESCORE_ALIGNMENT: hipLaunchKernelGGL(rescore_kernel<MMGPU_RESCORE_ALIGNMENT>, grid, block, 0, stream, A); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

void warm_rescore() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&rescore_kernel<MMGPU_RESCORE_ALIGNMENT>));
}

}  // namespace mmgpu
