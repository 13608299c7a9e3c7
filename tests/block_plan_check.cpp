// Host check of mmseqs2_amd/csrc/block_plan.h (tests/test_block_plan.py): the launch planning of the block aligner with limits
// small enough that a few dozen jobs cross every one of them - a real call needs 4096 pairs and gigabytes of traces to get there.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "block_plan.h"

using namespace mmgpu;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            failures++;                                                \
        }                                                              \
    } while (0)

static std::vector<BlockJob> random_jobs(int n, int max_len) {
    std::vector<BlockJob> v((size_t)n);
    for (int k = 0; k < n; k++) {
        v[k].query = (uint32_t)(rand() % 7);
        v[k].target = (uint32_t)rand();
        v[k].score = 300 + rand() % 1000;
        v[k].q_end = rand() % max_len;
        v[k].t_end = rand() % max_len;
        v[k].slot = (uint32_t)k;
    }
    return v;
}

static bool same_job(const BlockJob &a, const BlockJob &b) {
    return a.query == b.query && a.target == b.target && a.score == b.score && a.q_end == b.q_end && a.t_end == b.t_end && a.slot == b.slot;
}

static void check_order(int n, int max_len) {
    std::vector<BlockJob> jobs = random_jobs(n, max_len), want = jobs;
    std::stable_sort(want.begin(), want.end(), [](const BlockJob &x, const BlockJob &y) { return block_pair_len(x) > block_pair_len(y); });
    block_longest_first(jobs);
    CHECK(jobs.size() == want.size());
    for (size_t k = 0; k < jobs.size(); k++) CHECK(same_job(jobs[k], want[k]));
}

// every property a launch's plan must have, whatever the limits
static void check_plan(const std::vector<BlockJob> &todo, uint64_t per_res, uint64_t margin, uint64_t limit, bool starts_only) {
    std::vector<uint32_t> resume(todo.size());
    for (size_t k = 0; k < resume.size(); k++) resume[k] = (uint32_t)(32u << (k % 5)) | (k % 3 == 0 ? 0x10000u : 0u);
    Block4Plan plan;
    std::vector<BlockJob> left;
    left.push_back(todo.front());      // (what is in `left` already stays in front)
    block4_plan(todo, resume, per_res, margin, limit, starts_only, plan, left);
    CHECK(same_job(left.front(), todo.front()));
    left.erase(left.begin());
    CHECK(plan.group_begin.front() == 0 && plan.group_begin.back() == plan.jobs.size() && plan.n_groups() >= 1);
    // every job of todo in exactly one group or in left, both in input order
    size_t in_plan = 0, in_left = 0;
    for (const BlockJob &j : todo) {
        const uint64_t len = block_pair_len(j);
        const uint64_t bytes = (((len + 64) * 20 + 31) & ~31ull) + per_res * (len + margin);
        const bool too_large = !starts_only && (bytes > limit || bytes > 0xFFFFFFFFull);
        if (too_large) {
            CHECK(in_left < left.size() && same_job(left[in_left], j));
            in_left++;
        } else {
            CHECK(in_plan < plan.jobs.size());
            const Block2Job &x = plan.jobs[in_plan];
            CHECK(x.query == j.query && x.target == j.target && x.score == j.score && x.q_end == j.q_end && x.t_end == j.t_end && x.slot == j.slot);
            CHECK(x.pad == (resume[j.slot] & 0xFFFFu));
            CHECK(x.pool_bytes == (starts_only ? 0u : (uint32_t)bytes));
            in_plan++;
        }
    }
    CHECK(in_plan == plan.jobs.size() && in_left == left.size());
    // inside a group the slots follow one another (disjoint, input order) and end at or below the limit; pool_need = largest group
    uint64_t largest = 0;
    for (size_t g = 0; g < plan.n_groups(); g++) {
        CHECK(plan.group_begin[g] <= plan.group_begin[g + 1]);
        CHECK(g == 0 || g + 1 == plan.n_groups() || plan.group_begin[g] < plan.group_begin[g + 1]);
        uint64_t end = 0;
        for (uint32_t k = plan.group_begin[g]; k < plan.group_begin[g + 1]; k++) {
            CHECK(plan.jobs[k].pool_off == (starts_only ? 0 : end));
            end += plan.jobs[k].pool_bytes;
        }
        CHECK(end <= limit);
        largest = std::max(largest, end);
        // a group ends only where the next pair would not have fitted
        if (g + 1 < plan.n_groups() && plan.group_begin[g + 1] < plan.jobs.size()) CHECK(end + plan.jobs[plan.group_begin[g + 1]].pool_bytes > limit);
    }
    CHECK(plan.pool_need == largest);
    if (starts_only) {
        CHECK(plan.n_groups() == 1 && plan.pool_need == 0 && left.empty());
        for (const Block2Job &x : plan.jobs) CHECK(x.pool_bytes == 0 && x.pool_off == 0);
    }
}

int main(int argc, char **argv) {
    srand(argc > 1 ? (unsigned)atoi(argv[1]) : 1u);
    // order: ties (few distinct lengths), one job, many lengths
    check_order(1, 50);
    check_order(60, 4);
    check_order(48, 3000);
    check_order(500, 65536);

    // one launch's plan.  A pair of 200 residues at 48 trace bytes per residue and a margin of 512: a block list of
    // (200 + 64) * 20 = 5280 bytes and 48 * 712 = 34176 of trace, 39456 in all: two of them fit a pool of 100 000, a pair of 2000
    // residues (41280 + 48 * 2512 = 161856) does not fit at all
    {
        std::vector<BlockJob> todo = random_jobs(5, 1);
        const int lens[5] = {2000, 200, 200, 200, 150};
        for (int k = 0; k < 5; k++) { todo[k].q_end = lens[k] / 2 - 1; todo[k].t_end = lens[k] / 2 - 1; }
        std::vector<uint32_t> resume(5, 64u | 0x10000u);
        Block4Plan plan;
        std::vector<BlockJob> left;
        block4_plan(todo, resume, 48, 512, 100000, false, plan, left);
        CHECK(left.size() == 1 && left[0].slot == 0);
        CHECK(plan.jobs.size() == 4 && plan.n_groups() == 2 && plan.group_begin[1] == 2);
        CHECK(plan.jobs[0].pool_off == 0 && plan.jobs[0].pool_bytes == 39456 && plan.jobs[1].pool_off == 39456 && plan.jobs[2].pool_off == 0);
        CHECK(plan.jobs[3].pool_off == 39456 && plan.jobs[3].pool_bytes == ((214 * 20 + 31) & ~31) + 48 * 662);
        CHECK(plan.pool_need == 78912 && plan.jobs[0].pad == 64);
        // the same pairs with a pool that would hold them but slots beyond 4 GB (pool_bytes is a uint32): all handed on
        left.clear();
        block4_plan(todo, resume, 1ull << 23, 512, 1ull << 40, false, plan, left);
        CHECK(left.size() == 5 && plan.jobs.empty() && plan.n_groups() == 1 && plan.pool_need == 0);
        check_plan(todo, 1ull << 21, 512, 1ull << 40, false);      // (2 M per residue: the pair of 2000 residues alone passes 4 GB)
    }
    for (int round = 0; round < 20; round++) {
        std::vector<BlockJob> todo = random_jobs(24 + rand() % 40, 400);
        block_longest_first(todo);
        check_plan(todo, 48, 512, 100000, false);       // several groups, the longest pairs handed on
        check_plan(todo, 160, 2048, 400000, false);
        check_plan(todo, 1024, 2048, 1500000, false);   // the skewed form's slots: few pairs per group
        check_plan(todo, 48, 512, 3072ull << 20, false);      // the real limit: one group
        check_plan(todo, 48, 512, 30000, true);         // no trace: no slots, one group, nothing handed on
    }

    // the head: none below 4096 pairs, then a sixteenth of the pairs but at most one per CU (a context that knows no CU count: one)
    CHECK(block_head_size(4095, 256) == 0 && block_head_size(4095, 0) == 0);
    CHECK(block_head_size(4096, 256) == 256 && block_head_size(4096, 0) == 1);
    CHECK(block_head_size(65536, 256) == 256 && block_head_size(65536, 0) == 1);
    CHECK(block_head_size(4800, 304) == 300);
    CHECK(block_head_size(40, 256, 32, 4) == 10 && block_head_size(31, 256, 32, 4) == 0 && block_head_size(40, 3, 32, 4) == 3);

    // tier slots, by hand: 100 residues, 8 entries per column, 512 rows: block list (164 * 16 = 2624) + 8 * 32 * (100 + 1024) = 287744
    CHECK(block_tier_slot_bytes(100, 8, 512, false) == 290368);
    // 1000 residues in the third tier: borders 8 * 4096 * 2 = 65536, block list 1064 * 16 = 17024, trace 64 * 32 * (1000 + 8192) = 18825216
    CHECK(block_tier_slot_bytes(1000, 64, 4096, true) == 18907776);
    CHECK(block_tier_slots(1000, 256, 16, 290368) == 1000 && block_tier_slots(5000, 256, 16, 290368) == 4096);
    CHECK(block_tier_slots(5000, 0, 4, 290368) == 4);
    CHECK(block_tier_slots(1000, 256, 16, 290368, 10 * 290368 + 5) == 10 && block_tier_slots(1000, 256, 16, 290368, 1000) == 1);
    CHECK(block_tier_slots(5000, 256, 4, 18907776) == 908);      // 16 GB / 18.9 MB

    if (failures) return 1;
    printf("OK\n");
    return 0;
}
