// Launch planning of the block aligner's host side (mmgpu_api.hip, block_backtrace): which path a pair takes.  Plain host
// arithmetic over the job records, no HIP in it - tests/block_plan_check.cpp compiles it alone and crosses every limit with a few
// dozen jobs.  The limits are arguments; the values of a real call are the constants below.
#ifndef MMGPU_BLOCK_PLAN_H
#define MMGPU_BLOCK_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mmgpu {

constexpr int BLOCK_MAX_SIZE = 512;        // largest block the first-tier kernel holds in LDS
constexpr int BLOCK_MID_SIZE = 2048;       // second tier: still in LDS (32 KB)
constexpr int BLOCK_REF_MAX_SIZE = 4096;   // MAX_SIZE of the reference (StripedSmithWaterman.cpp:37); third tier, borders in HBM
struct BlockJob {
    uint32_t query, target;
    int32_t score, q_end, t_end;
    uint32_t slot;                // index into out / bt_off
};
struct BkBlock { uint32_t i, j; uint16_t h, w; uint32_t right, tstart; };   // Trace::block_start / block_size / right + the block's first trace entry
struct Block2Job {
    uint32_t query, target;
    int32_t score, q_end, t_end;
    uint32_t slot;                // index into out / bt_off
    uint64_t pool_off;            // the pair's scratch (block list + trace) in the pool; unused without a trace
    uint32_t pool_bytes, pad;     // pad: block4_kernel.hip - the first minimum block size to try (0 = 32)
};

constexpr uint64_t BLOCK_HEAD_MIN_PAIRS = 4096;          // fewer sequence pairs in a call: no head launch
constexpr uint64_t BLOCK_HEAD_SHARE = 16;                // the head is at most a sixteenth of the pairs
constexpr uint64_t BLOCK4_POOL_LIMIT = 3072ull << 20;    // block lists + traces of one group of a block4 launch
constexpr uint64_t BLOCK_TIER_POOL_LIMIT = 16384ull << 20;   // scratch slots of one tier launch

inline uint64_t block_pair_len(const BlockJob &j) { return (uint64_t)j.q_end + 1 + (uint64_t)j.t_end + 1; }

// longest pair first, stable: a counting sort over q_end + t_end + 2 (both ends below 65536)
inline void block_longest_first(std::vector<BlockJob> &jobs) {
    uint64_t longest = 0;
    for (const BlockJob &j : jobs) longest = std::max(longest, block_pair_len(j));
    std::vector<uint32_t> first((size_t)longest + 2, 0u);
    for (const BlockJob &j : jobs) first[(size_t)block_pair_len(j)]++;
    uint32_t run = 0;
    for (size_t len = (size_t)longest + 1; len-- > 0;) { const uint32_t cnt = first[len]; first[len] = run; run += cnt; }
    std::vector<BlockJob> sorted(jobs.size());
    for (const BlockJob &j : jobs) sorted[first[(size_t)block_pair_len(j)]++] = j;
    jobs.swap(sorted);
}

// The longest pairs - one per CU - go straight to the skewed form on a stream of their own, beside everything else: the pairs
// whose blocks grow to thousands of rows are among them, each a dependent chain of tens of milliseconds that nothing shortens
// but starting it first.
inline size_t block_head_size(size_t n_pairs, int compute_units, uint64_t min_pairs = BLOCK_HEAD_MIN_PAIRS, uint64_t share = BLOCK_HEAD_SHARE) {
    return n_pairs >= min_pairs ? std::min<size_t>(n_pairs / share, (size_t)std::max(compute_units, 1)) : 0;
}

// One block4 launch: `todo` (longest first) with slots of `per_res` trace bytes per residue of the pair (+ `margin` residues) behind
// the pair's block list.  The pairs run in groups [group_begin[g], group_begin[g + 1]) whose slots fit `pool_limit` together; a pair
// whose slot alone exceeds it (or 4 GB: pool_bytes is a uint32) goes to `left`.  starts_only: no trace, no slots, one group.
// resume: per result slot, the first minimum block size still to try in its low 16 bits (Block2Job::pad).
struct Block4Plan {
    std::vector<Block2Job> jobs;
    std::vector<uint32_t> group_begin;
    uint64_t pool_need = 0;      // the largest group
    size_t n_groups() const { return group_begin.size() - 1; }
};
inline void block4_plan(const std::vector<BlockJob> &todo, const std::vector<uint32_t> &resume, uint64_t per_res, uint64_t margin,
                        uint64_t pool_limit, bool starts_only, Block4Plan &plan, std::vector<BlockJob> &left) {
    plan.jobs.clear();
    plan.jobs.reserve(todo.size());
    plan.group_begin.assign(1, 0u);
    plan.pool_need = 0;
    uint64_t pool_used = 0;
    for (const BlockJob &j : todo) {
        Block2Job x;
        x.query = j.query; x.target = j.target; x.score = j.score; x.q_end = j.q_end; x.t_end = j.t_end; x.slot = j.slot;
        x.pool_off = 0; x.pool_bytes = 0; x.pad = resume[j.slot] & 0xFFFFu;
        if (!starts_only) {
            const uint64_t len = block_pair_len(j);
            const uint64_t bytes = (((len + 64) * sizeof(BkBlock) + 31) & ~31ull) + per_res * (len + margin);
            if (bytes > pool_limit || bytes > 0xFFFFFFFFull) { left.push_back(j); continue; }
            if (pool_used + bytes > pool_limit) { plan.group_begin.push_back((uint32_t)plan.jobs.size()); pool_used = 0; }
            x.pool_off = pool_used; x.pool_bytes = (uint32_t)bytes;
            pool_used += bytes;
            plan.pool_need = std::max(plan.pool_need, pool_used);
        }
        plan.jobs.push_back(x);
    }
    plan.group_begin.push_back((uint32_t)plan.jobs.size());
}

// Scratch slot of one pair in a tier launch (block_kernel.hip): the border arrays (third tier only), the block list, and
// entries_per_col trace entries (32 B per 64 rows) per column of a pair of `len` residues whose blocks reach max_rows
inline uint64_t block_tier_slot_bytes(uint64_t len, uint64_t entries_per_col, uint64_t max_rows, bool borders) {
    return (borders ? (uint64_t)8 * BLOCK_REF_MAX_SIZE * 2 : 0ull) + (((len + 64) * 16 + 31) & ~31ull) + entries_per_col * 32 * (len + 2 * max_rows);
}
// ... and how many of them a launch over n_todo pairs gets: one per resident wavefront, as far as the pool goes, at least one
inline uint32_t block_tier_slots(size_t n_todo, int compute_units, uint64_t waves_per_cu, uint64_t slot_bytes, uint64_t pool_limit = BLOCK_TIER_POOL_LIMIT) {
    const uint64_t want = std::min<uint64_t>(n_todo, (uint64_t)std::max(compute_units, 1) * waves_per_cu);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, pool_limit / slot_bytes));
}

}  // namespace mmgpu
#endif
