// Single-tile Smith-Waterman with the forward scan in packed f16 (gfx950: v_pk_maximum3_f16), the twins of sw_kernel<0..2, BOTH>.
//
// The forward scan of a pair runs in f16 first: 8.5 packed ops per row of two cells instead of the 10 of the int16 scan
// (sw_body.h, at SW_HALF_LIMIT, has the recurrence and the proof that a score of at most SW_HALF_LIMIT = 1792 is the int16
// score, end position and all).  A pair whose f16 maximum exceeds the limit is marked in its result record; the workgroup that
// found it then builds the int16 profile and runs the int16 forward scan over its marked pairs, packed to the front.  The
// reverse scan follows as in sw_kernel.hip, in int16, over every pair that wants one.  One launch, no host round trip, the same
// SwJob: which kernel a batch gets is launch_sw's decision (sw_kernel.hip, sw_half_eligible).
//
// Forward-only kernels (BOTH = false): the f16 body with its int16 re-run beside it needs more registers than the int16 body
// alone, and these kernels sit at the edge of a wavefront each (profiles/sw_half_isa_audit.txt).  launch_sw_half serves a
// forward-only group only where the f16 kernel keeps its twin's wavefronts without scratch - SW_HALF_FORWARD_ONLY below; the
// other groups stay with sw_kernel<G, false>.
#include "mmgpu_internal.h"
#include "pf_device.h"
#include "sw_body.h"

namespace mmgpu {

namespace {

// W = 32: the wide bodies (sw_body.h).  Their f16 pass can be switched off per launch (SwLaunch::half_wide = 0, the A/B switch
// MMGPU_SW_HALF_WIDE): every pair of the job is marked instead, and the int16 scan of the marked pairs is the forward scan - the int16
// column loop of sw_kernel<G, BOTH> in the same grid as the f16 scans of the 16-lane bodies, with no second set of bodies.
template <int R, bool BOTH, int W = GROUP>
__device__ __forceinline__ void sw_half_passes(const SwLaunch &L, const SwJob &job) {
    constexpr bool PF = SW_PREFETCHES<R, false, BOTH>;   // as sw_passes
    const bool f16 = W == GROUP || L.half_wide;   // workgroup-uniform
    if (f16) {
        sw_body<R, false, false, PF, true, false, W>(L, job);
    } else {
        for (uint32_t h = job.hit_begin + threadIdx.x; h < job.hit_end; h += blockDim.x) L.out[L.hit_out[h]].score = SW_HALF_MARK;
    }
    // the results and marks of this job, written by other waves of the workgroup; and every wave is done with the f16 profile
    __threadfence_block();
    __syncthreads();
    if (!f16 || sw_half_any_marked()) {   // workgroup-uniform
        sw_body<R, false, false, PF, false, true, W>(L, job);
        __threadfence_block();
        __syncthreads();
    }
    if constexpr (BOTH) sw_body<R, false, true, PF, false, false, W>(L, job);
}

// which forward-only groups have an f16 kernel (the others: launch_sw_half declines, launch_sw stays with int16)
constexpr bool SW_HALF_FORWARD_ONLY[3] = {false, false, false};

template <int G, bool BOTH>
__global__ __launch_bounds__(WAVES * 64)
__attribute__((amdgpu_waves_per_eu(sw_waves_floor(G, BOTH), sw_waves_cap(G, BOTH)))) void sw_half_kernel(SwLaunch L) {   // (sw_kernel's floors)
    SwJob job = L.jobs[blockIdx.x];
    if (!sw_clip_job(L, job)) return;
    sw_dispatch_shape<G>(job.shape, [&](auto r, auto kind) __attribute__((always_inline)) {
        if constexpr (decltype(kind)::value != SW_MULTI)
            sw_half_passes<decltype(r)::value, BOTH, decltype(kind)::value == SW_WIDE ? 2 * GROUP : GROUP>(L, job);
    });
}

// the forward-only kernels no launch uses, for the audit that decides SW_HALF_FORWARD_ONLY (scripts/sw_isa_audit.py -D ...)
#ifdef MMGPU_SW_HALF_AUDIT_FORWARD
template __global__ void sw_half_kernel<0, false>(SwLaunch);
template __global__ void sw_half_kernel<1, false>(SwLaunch);
template __global__ void sw_half_kernel<2, false>(SwLaunch);
#endif

}  // namespace

// The f16 twin of launch_sw's kernel for this group, if there is one: false = the caller launches the int16 kernel.
// Group 2 is single-tile only where the multi-tile jobs have a group of their own (SW_GROUPS == 4).
bool launch_sw_half(const SwLaunch &L, int group, size_t lds_bytes, bool both_passes, hipStream_t stream) {
    if (group < 0 || group > 2 || (group == 2 && SW_GROUPS != 4)) return false;
    if (!both_passes && !SW_HALF_FORWARD_ONLY[group]) return false;
    dim3 grid(L.n_jobs), block(WAVES * 64);
    const size_t lds = lds_bytes + SW_LDS_HEADER;
    switch (group) {
        case 0: hipLaunchKernelGGL((sw_half_kernel<0, true>), grid, block, lds, stream, L); break;
        case 1: hipLaunchKernelGGL((sw_half_kernel<1, true>), grid, block, lds, stream, L); break;
        default: hipLaunchKernelGGL((sw_half_kernel<2, true>), grid, block, lds, stream, L); break;
    }
    return true;
}

void warm_sw_half() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_half_kernel<0, true>));
}

}  // namespace mmgpu
