// Internal declarations shared by the HIP translation units of libmmgpu (not part of the C-ABI).
#ifndef MMGPU_INTERNAL_H
#define MMGPU_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <array>
#include <string>
#include <map>
#include <mutex>
#include <chrono>
#include <memory>
#include <vector>
#include <thread>
#include <atomic>

#include "../../include/mmgpu.h"
#include "nucl_core.h"
#include "block_plan.h"

namespace mmgpu {

// Target database resident in HBM.  Every sequence starts on a 4-byte boundary so the group-head lane can
// fetch four residues per global_load_dword; `off4` is the start in dwords.
struct DeviceDb {
    uint8_t *res = nullptr;      // residues, 4-byte aligned starts, tail slack of max_len + 64 bytes
    uint32_t *off4 = nullptr;    // [n] start of sequence i in units of 4 bytes
    uint32_t *len = nullptr;     // [n]
    uint32_t n = 0;
    uint32_t max_len = 0;
    uint64_t total_residues = 0;
    int alphabet = 0;
    size_t res_bytes = 0;        // allocated size of `res`
};

// The targets an alignment batch reads, in DeviceDb's layout: the context's resident database, or the private masked copies of a
// batch of mmgpu_sw_prepare_masked (one per pair, id = pair ordinal).  The kernels take res / off4 / len as launch arguments.
struct TargetView {
    const uint8_t *res = nullptr;
    const uint32_t *off4 = nullptr;
    const uint32_t *len = nullptr;
    uint32_t n = 0;
    uint32_t max_len = 0;
    const uint32_t *h_len = nullptr;   // [n] host copy of the lengths (scheduling)
};

// sw_mask_kernel.hip: the masked copies of a batch's targets, gathered out of the resident database
struct SwMaskGatherArgs {
    const uint8_t *src_res;            // the resident targets
    const uint32_t *src_off4, *src_len;
    const uint32_t *src_id;            // [n_pairs] resident id of every pair's target
    uint8_t *dst_res;                  // the batch's arena (filled with the pad letter before the launch)
    const uint32_t *dst_off4;          // [n_pairs] start of pair p's copy in units of 4 bytes
    const uint32_t *span_off;          // [n_pairs + 1]
    const mmgpu_sw_span *spans;        // residues [t_from, t_to) of the copy read as mask_letter; t_to <= the target's length
    uint32_t span_base;                // span_off[0]: spans[k - span_base] is span k of span_off's numbering
    uint32_t mask_letter;
    uint32_t n_pairs;
};
hipError_t launch_sw_mask_gather(const SwMaskGatherArgs &A, hipStream_t stream);

// One workgroup's share of a batch: hits [hit_begin, hit_end) of one query (already sorted by target length).
struct SwJob {
    uint32_t query;
    uint32_t hit_begin;
    uint32_t hit_end;
    uint32_t shape;   // low 8 bits: tile shape (rows per lane - 1, + 32 for multi-tile, + 64 for a single tile on 32-lane groups);
                      // high 24: multi-tile scratch slot
};

// Everything a Smith-Waterman launch needs, device pointers only.
struct SwLaunch {
    const SwJob *jobs;
    uint32_t n_jobs;
    // queries of the batch
    const uint8_t *q_res;     // concatenated numeric residues
    const int8_t *q_cb;       // concatenated rounded composition bias (zeros when absent)
    const uint32_t *q_off;    // [nq+1]
    const int32_t *q_bias;    // [nq] ssw_init bias (StripedSmithWaterman.cpp:1397-1406), decides `word`
    const int32_t *q_minstart; // [nq] reverse scan only for pairs with score >= this
    // profile queries (ssw_init with DBTYPE_HMM_PROFILE): int8 [alphabet][qlen] per query, letter-major, concatenated;
    // q_prof_off[q] = byte offset of the query's block, 0xFFFFFFFF for a sequence query; q_prof_off null = none in the batch
    const int8_t *q_prof;
    const uint32_t *q_prof_off;
    // targets
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const uint32_t *t_len;
    // hits (sorted order) and where each one's result goes
    const uint32_t *hit_target;
    const uint32_t *hit_out;  // index into out[]
    mmgpu_sw_hit *out;
    // reverse pass only: per-hit forward result lives in out[hit_out[h]]
    // scoring
    const int8_t *mat;        // alphabet*alphabet
    int alphabet;
    int gap_open, gap_extend;
    // multi-tile scratch (H/F boundary rows), [scratch slot][4 waves][4 groups][2][scratch_cols] x uint2.  Slots are a
    // pool sized by the workgroups that can be resident at once, not by the jobs of the batch: a workgroup claims a free
    // slot when it starts (scratch_busy, one flag per slot) and releases it when it ends.
    uint2 *scratch;
    uint32_t scratch_cols;
    uint32_t *scratch_busy;
    uint32_t scratch_slots;
    // multi-tile jobs whose tiles all fit this many bytes of LDS (sw_multi_resident) build every tile's profile once; the launch's
    // LDS was sized by the same rule (mmgpu_sw_batch_t::group_lds).  0: none does.
    uint32_t resident_lds = 0;
    // fused hand-over from a prefilter batch: hits of query q live in slots [q * hit_stride, + q_hit_count[q])
    const uint32_t *q_hit_count;   // null for caller-supplied lists
    uint32_t hit_stride;
    // which pairs get a reverse scan (sw_rev_wanted, sw_kernel.hip): 0 = score >= q_minstart (MMGPU_SW_START); 1 = ... and word == 0
    // (MMGPU_SW_START_NOT_WORD: the start of an int16-range hit comes from the block aligner); 2 = the pairs flagged in rev_force,
    // indexed like out[] (mmgpu_sw_reverse_pairs).  rev_only: the forward results are in out[] already, only the reverse scan runs.
    int rev_mode = 0;
    int rev_only = 0;
    const uint8_t *rev_force = nullptr;
    // the wide (32-lane) bodies of an f16 kernel: 1 = f16 forward scan first like the 16-lane bodies, 0 = every pair goes straight to the
    // int16 scan of the marked pairs (sw_half_wide, below)
    int half_wide = 1;
};

constexpr int SW_PF_MAX_LIST = 16384;  // longest list of the fused hand-over (sw_from_pf_kernel orders it in LDS, 4 bytes per slot; PF_MAX_HITS is the prefilter's own LDS limit)
// sw_from_pf_kernel's statistics (cells, pairs, longest target): one workgroup per query adds to slot blockIdx % SLOTS of
// [SLOTS][3] - 10 000 workgroups x 6 atomics on three words serialised at the L2 and were most of the kernel's 0.73 ms
constexpr int SW_FROM_PF_STAT_SLOTS = 64;

struct SwFromPfArgs {
    const mmgpu_pf_hit *pf_hits;   // [nq][pf_stride]
    uint32_t pf_stride;
    const uint32_t *hit_count;     // [nq]
    uint32_t stride;               // slots per query in the alignment batch
    const uint32_t *q_off;
    const uint32_t *t_len;
    uint32_t *hit_target, *hit_out;
    unsigned long long *cells, *pairs;      // slot 0 of [SW_FROM_PF_STAT_SLOTS][3] (cells, pairs, longest target)
    // copies owned by the alignment batch, so that it does not depend on the prefilter batch after this kernel:
    uint32_t *count_copy;          // [nq] list lengths (clipped to stride)
    uint32_t *slot_target;         // [nq * stride] target id of every result slot (list order), 0 beyond the list
};

constexpr int SW_REV_JOB_MAX = 1024;   // most hits of one reverse-scan job of a multi-tile query (sw_rev_multi_kernel)
hipError_t launch_sw_rev_multi(const SwLaunch &L, size_t lds_bytes, hipStream_t stream);
hipError_t launch_sw_from_pf(const SwFromPfArgs &A, uint32_t nq, hipStream_t stream);
// workgroups of the multi-tile kernel group that can be resident on the device at once (sizes the scratch pool)
uint32_t sw_multi_resident_blocks(size_t lds_bytes, bool both_passes, int compute_units);

// rows_per_lane in {8,16,24,32}: a 16-lane group covers 16*rows_per_lane query rows per tile.
// reverse = false: forward score/end scan; true: start-position scan over the reversed prefixes.
#ifndef MMGPU_SW_MAX_R
#define MMGPU_SW_MAX_R 28
#endif
constexpr int SW_MAX_R = MMGPU_SW_MAX_R;   // rows per lane of the largest tile (16 lanes x SW_MAX_R query rows); longer queries are cut into tiles
static_assert(SW_MAX_R >= 16 && SW_MAX_R <= 32, "multi-tile bodies exist for 8..32 rows per lane: a query cut into tiles gets at least SW_MAX_R / 2");
#ifndef MMGPU_SW_MIN_WAVES
#define MMGPU_SW_MIN_WAVES 2
#endif
constexpr int SW_MIN_WAVES = MMGPU_SW_MIN_WAVES;   // occupancy floor (waves per SIMD) the alignment kernels are compiled for
#ifndef MMGPU_SW_GROUPS
#define MMGPU_SW_GROUPS 4
#endif
// kernels per pass: tile shapes grouped by register need (sw_kernel.hip): single tiles of up to SW_GROUP0_MAX_R rows per lane, of up
// to SW_GROUP1_MAX_R, the larger ones, and - always the last group - the queries cut into several tiles (3: the last two in one
// kernel, rounds 1-2).  A wide body has the registers of the 16-lane single-tile body of its R, and its group.
constexpr int SW_GROUPS = MMGPU_SW_GROUPS;
static_assert(SW_GROUPS == 3 || SW_GROUPS == 4, "three or four kernel groups");
constexpr int SW_GROUP0_MAX_R = 12;
constexpr int SW_GROUP1_MAX_R = 24;
__host__ __device__ constexpr int sw_group_of(bool multi, int R) {
    return multi ? SW_GROUPS - 1 : (R <= SW_GROUP0_MAX_R ? 0 : (R <= SW_GROUP1_MAX_R ? 1 : 2));
}
int sw_shape_group(uint32_t shape);
hipError_t launch_sw(const SwLaunch &L, int group, size_t lds_bytes, bool both_passes, hipStream_t stream);
// Build knob for A/B measurements: MMGPU_SW_HALF=0 keeps every batch on the int16 kernels of sw_kernel.hip.  1 (default): the
// single-tile groups of an eligible batch run sw_half_kernel.hip's kernels, whose forward scan is packed f16 with an int16 re-run of
// the pairs that score past SW_HALF_LIMIT (sw_body.h).  launch_sw_half launches the f16 twin of a group's kernel if there is one.
#ifndef MMGPU_SW_HALF
#define MMGPU_SW_HALF 1
#endif
bool launch_sw_half(const SwLaunch &L, int group, size_t lds_bytes, bool both_passes, hipStream_t stream);
void warm_sw_half();

// LDS of an alignment workgroup: a header (the reverse pass's packed live hits and the chunk counter) followed by query profiles,
// one per tile held.  Host (the launch's LDS size) and kernel (which jobs keep all their tiles) use the functions below: both sides
// of one rule, because a kernel that holds more tiles than the host granted writes past its LDS.
constexpr int SW_LDS_HEADER = SW_REV_JOB_MAX * 2 + 64;
__host__ __device__ constexpr int lane_stride_bytes(int R) {
    // R*2 bytes of scores per lane, rounded up to an odd number of 16-byte slots (bank spread)
    int slots = (R * 2 + 15) / 16;
    if ((slots & 1) == 0) slots += 1;
    return slots * 16;
}
// one tile's profile: (alphabet + 1) letters x the lanes of a group (16, or 32 for the wide shapes) x the lane stride
__host__ __device__ constexpr uint32_t sw_profile_bytes(int R, int alphabet, int lanes = 16) {
    return (uint32_t)(alphabet + 1) * (uint32_t)lanes * (uint32_t)lane_stride_bytes(R);
}
// Build knob for A/B measurements: the LDS a multi-tile job may fill with the profiles of all its tiles (header included).  64 KB is
// what a workgroup may ask for without the launch attribute that raises the ceiling; 0 = no job is resident (every tile's profile is
// rebuilt in every round of hits, the path of the jobs that do not fit).
#ifndef MMGPU_SW_RESIDENT_LDS
#define MMGPU_SW_RESIDENT_LDS 65536
#endif
constexpr uint32_t SW_RESIDENT_LDS = MMGPU_SW_RESIDENT_LDS;
static_assert(SW_RESIDENT_LDS <= 65536u, "a workgroup asks for at most 64 KB of dynamic LDS");
// tiles of a query of qlen rows at R rows per lane
__host__ __device__ constexpr uint32_t sw_tiles(uint32_t qlen, int R) { return (qlen + 16u * (uint32_t)R - 1u) / (16u * (uint32_t)R); }
// a multi-tile job is resident when the profiles of all its tiles and the header fit the budget
__host__ __device__ constexpr bool sw_multi_resident(uint32_t n_tiles, int R, int alphabet, uint32_t budget) {
    return (unsigned long long)n_tiles * sw_profile_bytes(R, alphabet) + (unsigned long long)SW_LDS_HEADER <= (unsigned long long)budget;
}
// 21 letters, 64 KB: two tiles of any R (56 320 bytes + header at R = 28), three of R <= 24; not three of R >= 25, not four
static_assert(sw_multi_resident(2, 28, 21, 65536) && sw_multi_resident(3, 24, 21, 65536) && !sw_multi_resident(3, 25, 21, 65536) &&
              !sw_multi_resident(4, 22, 21, 65536) && !sw_multi_resident(2, 8, 21, 0), "residency rule");

// Wide shapes: a query of 16 * SW_MAX_R + 1 .. 32 * SW_MAX_R residues is ONE tile of a 32-lane group (two DPP rows, sw_body.h) instead
// of two tiles of a 16-lane group: R = ceil(qlen / 32) rows per lane, shape code SW_SHAPE_WIDE + R - 1.  Its profile is what the two
// resident tiles took, so it fits the same LDS budget.
constexpr uint32_t SW_SHAPE_MULTI = 32, SW_SHAPE_WIDE = 64;
constexpr int SW_WIDE_MIN_R = (16 * SW_MAX_R + 1 + 31) / 32;   // rows per lane of the shortest wide query
static_assert(sw_profile_bytes(SW_MAX_R, 21, 32) == 2 * sw_profile_bytes(SW_MAX_R, 21) &&
              sw_profile_bytes(SW_MAX_R, 21, 32) + SW_LDS_HEADER <= 65536u, "a wide tile fits a workgroup's 64 KB");
static_assert((lane_stride_bytes(SW_MAX_R) / 16) % 2 == 1 && (lane_stride_bytes(SW_WIDE_MIN_R) / 16) % 2 == 1, "odd number of 16-byte slots");
// Runtime switches for A/B runs and the tests (read from the environment once per process):
// MMGPU_SW_WIDE=0 keeps those queries on the two-tile path (the shapes of before the wide groups);
// MMGPU_SW_HALF_WIDE=0 / 1: the forward scan of the wide bodies in int16 / in f16 with the int16 re-run; unset = the measured default.
bool sw_wide_enabled();
bool sw_half_wide();

// ---------------------------------------------------------------------------------------------------------
// exhaustive ungapped scan (scan_kernel.hip): every query against every resident target of its length window
constexpr int SCAN_CLASSES = 5;                       // rows per lane 8, 16, 24, 32 (one tile), and tiles of 32 for longer queries
constexpr int SCAN_MULTI = SCAN_CLASSES - 1;
constexpr int SCAN_MAX_R = 32;                        // rows per lane of the largest tile: 16 lanes x 32 = 512 query rows
constexpr int SCAN_ROUND = 32;                        // targets a workgroup scores at once: 4 waves x 4 DPP rows x 2 halves
constexpr int SCAN_JOB_TARGETS = 16 * SCAN_ROUND;     // targets per job of a one-tile query (a multi-tile job is one round)
__host__ __device__ constexpr int scan_class_rows(int cls) { return cls == 0 ? 8 : cls == 1 ? 16 : cls == 2 ? 24 : 32; }
// columns a pair's scan covers: the longer target's length, rounded up to whole chunks of R columns (the rest reads the pad letter)
__host__ __device__ constexpr uint32_t scan_cols(uint32_t len, int R) { return (len + (uint32_t)R - 1u) / (uint32_t)R * (uint32_t)R; }
// dwords of one DPP row's boundary line (multi-tile): two buffers of scan_cols + 1 entries, rounded to whole 64-byte lines
__host__ __device__ constexpr uint32_t scan_park_row_words(uint32_t longest) { return 2u * ((scan_cols(longest, SCAN_MAX_R) + 1u + 15u) & ~15u); }

constexpr uint64_t SCAN_NO_PROFILE = ~0ull;           // ScanLaunch::q_prof_off of a sequence query

struct ScanJob {
    uint32_t query;
    uint32_t begin, end;      // positions in the length-sorted id list (longest first)
    uint32_t pad;
};

struct ScanLaunch {
    const ScanJob *jobs;
    uint32_t n_jobs;
    const uint8_t *q_res;     // concatenated numeric residues
    const int8_t *q_cb;       // concatenated rounded composition bias (zeros when absent)
    const uint32_t *q_off;    // [nq + 1]
    const int32_t *q_cap;     // [nq] 255 - B
    // profile queries: q_prof + q_prof_off[query] is the query's int8 [q_prof_letters[query]][qlen], letter-major; a sequence query
    // has SCAN_NO_PROFILE there (its rows come from mat, q_res and q_cb)
    const int8_t *q_prof;
    const uint64_t *q_prof_off;      // [nq]
    const uint32_t *q_prof_letters;  // [nq]
    const uint8_t *t_res;
    const uint32_t *t_off4, *t_len;
    const uint32_t *order;    // [n_targets] ids by length, longest first
    uint32_t n_targets;
    const int8_t *mat;
    int alphabet;
    uint8_t *scores;          // [nq][n_targets]
    // multi-tile launches: persistent workgroups, workgroup b owns the boundary lines park + park_off[b] (dwords) for jobs b, b + grid, ..
    uint32_t *park;
    const uint64_t *park_off;
};
hipError_t launch_scan(const ScanLaunch &L, int cls, uint32_t grid, hipStream_t stream);

struct ScanSelectArgs {
    const uint8_t *scores;    // [nq][n_targets]
    const uint32_t *t_len;
    uint32_t n_targets;
    const uint32_t *q_ident;  // [nq] UINT32_MAX = none
    const uint32_t *q_win;    // [nq][2] inclusive window of target lengths
    int32_t min_score;
    uint32_t max_hits;
    mmgpu_pf_hit *hits;       // [nq][stride]
    uint32_t stride;
    uint32_t *counts;         // [nq]
};
hipError_t launch_scan_select(const ScanSelectArgs &A, uint32_t nq, hipStream_t stream);
void warm_scan();

// ---------------------------------------------------------------------------------------------------------
// exhaustive gapped scan (gscan_api.hip, gscan_kernel.hip): the Gotoh score of every query against every resident target of its
// window.  The pairs of a chunk of queries are an ordinary MMGPU_SW_SCORE_END batch whose lists are slices of the length-ordered id
// list: the planner kernel writes hit_target / hit_out on the device, the host cuts only the job ranges (sw_prepare_dense).
constexpr uint64_t GSCAN_PAIR_BUDGET = 1ull << 24;    // pairs scored at once by default: 16 M x (24 + 8) bytes of records and lists

// the lists of a dense alignment batch: query i of the call aligns against positions [begin[i], begin[i] + count[i]) of `order`; its
// pairs take the slots [slot_base(i), + count[i]) of the three shared device arrays, slot_base = the running sum of the counts
struct SwDenseLists {
    const uint32_t *begin, *count;     // [nq]
    const uint32_t *order;             // [n_targets] host: ids by length, longest first
    const uint64_t *len_prefix;        // [n_targets + 1] host: residues of order[0 .. k)
    uint32_t *d_hit_target, *d_hit_out;   // device, at least sum(count) entries each, owned by the caller
    mmgpu_sw_hit *d_out;
};

struct GscanPlanArgs {
    const uint32_t *order;             // [n_targets] device
    const uint32_t *q_begin, *q_count; // [nq] window slice of every query
    const uint32_t *q_slot;            // [nq] first slot of the query inside its chunk
    uint32_t q_first, n_queries;       // the chunk
    uint32_t *hit_target, *hit_out;
};
hipError_t launch_gscan_plan(const GscanPlanArgs &A, hipStream_t stream);

struct GscanIdentArgs {
    const uint8_t *q_res;
    const int8_t *q_cb;
    const uint32_t *q_off;             // [nq + 1]
    const int8_t *q_prof;              // [alphabet][qlen] blocks as SwLaunch::q_prof, null = no profile query in the batch
    const uint32_t *q_prof_off;        // [nq] 0xFFFFFFFF = sequence query
    const uint32_t *q_ident;           // [nq] UINT32_MAX = none (also: outside the window)
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const int8_t *mat;
    int alphabet;
    int32_t *ident_score;              // [nq]
};
hipError_t launch_gscan_identity(const GscanIdentArgs &A, uint32_t nq, hipStream_t stream);

struct GscanSelectArgs {
    const mmgpu_sw_hit *out;           // the chunk's records
    const uint32_t *order;
    const uint32_t *q_begin, *q_count, *q_slot;
    const uint32_t *q_ident;           // identity target inside the window, else UINT32_MAX
    const int32_t *ident_score;
    const int32_t *q_min_ev;           // [nq]
    const uint32_t *t_len;
    const uint32_t *q_win;             // [nq][2] inclusive window of target lengths
    int32_t *scores;                   // [nq][n_targets] raw scores in id order (kept for mmgpu_gscan_debug_scores)
    uint32_t n_targets;
    uint32_t q_first;
    int32_t min_score;
    uint32_t max_hits;
    mmgpu_pf_hit *hits;                // [nq][stride]
    uint32_t stride;
    uint32_t *counts;
};
hipError_t launch_gscan_select(const GscanSelectArgs &A, uint32_t n_queries, hipStream_t stream);
void warm_gscan();

// ---------------------------------------------------------------------------------------------------------
// ungapped diagonal rescoring (rescore_api.hip, rescore_kernel.hip): one record per hit of a prefilter result list.  RESCORE_GROUP
// lanes (one DPP row) share a hit: lane l walks cells [l * run, (l + 1) * run) of the diagonal, run = ceil(len / RESCORE_GROUP)
// rounded up to RESCORE_STEP (the cells of one dword of residues), and the lanes' summaries are combined in diagonal order.
constexpr int RESCORE_GROUP = 16;
constexpr int RESCORE_STEP = 4;
constexpr int RESCORE_THREADS = 256;      // a workgroup: 16 hits
constexpr int RESCORE_SLACK = 16;         // bytes behind the last query: an unaligned run reads the dword behind its last cell

struct RescoreArgs {
    const uint8_t *q_res;              // every query starts on a 4-byte boundary
    const uint32_t *q_off4, *q_len;    // [nq]
    const uint8_t *t_res;
    const uint32_t *t_off4, *t_len;
    const int8_t *mat;                 // [alphabet][alphabet]
    int alphabet;
    const uint32_t *hit_query;         // [n_hits]
    const mmgpu_rescore_pair *pairs;   // [n_hits]
    uint32_t n_hits;
    mmgpu_rescore_hit *out;            // [n_hits]
};
hipError_t launch_rescore(const RescoreArgs &A, int mode, hipStream_t stream);
void warm_rescore();

// ---------------------------------------------------------------------------------------------------------
// linclust's k-mer matching stage (kmermatch_api.hip, kmermatch_kernel.hip).  A record of the extraction is a k-mer and a packed
// value (0x7FFF - length) << 47 | id << 15 | position (15, 32 and 15 bits): the reference's first sort order (k-mer, length
// descending, id, position) is (k-mer, value) ascending, and the records leave the extraction in (id, position) order.  The length
// field ends below bit 63 on purpose: rocprim's merge path builds its mask as (1 << end_bit) - 1, which for end_bit 64 and a begin_bit
// above 0 shifts by the key's width and then compares the wrong bits.
constexpr uint32_t KMM_LEN_MASK = 0x7FFFu;
constexpr unsigned KMM_ID_SHIFT = 15, KMM_LEN_SHIFT = 47, KMM_LEN_END = 62;
constexpr int KMM_MAX_K = 32;                 // the staging of a round of windows holds 64 + KMM_MAX_K residues
constexpr uint32_t KMM_MAX_LEN = 32766;       // the reference switches its records to int at 32 767 residues; lengths and positions are 15 bits here
constexpr int KMM_STAGES = 5;                 // extract, sort 1, group, sort 2, vote

struct KmmExtractArgs {
    const uint8_t *res;                // the resident database
    const uint32_t *off4, *len;
    uint32_t n;
    int k, alph_size;
    uint8_t reduce[21];
    int kmers_per_seq;
    float kmers_per_seq_scale;
    unsigned long long seed;           // (uint64_t) par.hashShift
    uint4 *rule;                       // [n] {threshold score t, surplus of its bin, kmerConsidered, -}
    uint32_t *count;                   // [n] records of the sequence, the identity record included
    const uint32_t *rec_off;           // [n + 1] exclusive sum of count
    unsigned long long *rec_kmer, *rec_val;
};
struct KmmGroupArgs {
    const unsigned long long *kmer, *val;      // the sorted records
    uint32_t n_records;
    uint32_t *group_start;                     // [n_records] index of the record's representative
    float cov_thr;
    int cov_mode, only_extendable;
    int nucl;                                  // bit 63 of a k-mer is its strand (nuclmatch_api.hip)
};
// the extraction over a nucleotide database (nuclmatch_kernel.hip): 2-bit k-mers, the smaller of a window and its reverse complement
struct NuclExtractArgs {
    const uint8_t *res;                // the resident database, residues A C T G N = 0 .. 4
    const uint32_t *off4, *len;
    const uint32_t *order;             // [n] ids by length, longest first: workgroup b takes sequence order[b]
    uint32_t n;
    int k;
    int kmers_per_seq;
    float kmers_per_seq_scale;
    unsigned long long seed;
    uint4 *rule;                       // as KmmExtractArgs
    uint32_t *count;
    const uint32_t *rec_off;
    unsigned long long *rec_kmer, *rec_val;
};
hipError_t launch_nuclmatch_extract_count(const NuclExtractArgs &A, hipStream_t s);
hipError_t launch_nuclmatch_extract_write(const NuclExtractArgs &A, hipStream_t s);
hipError_t launch_kmm_extract_count(const KmmExtractArgs &A, hipStream_t s);
hipError_t launch_kmm_record_offsets(const uint32_t *count, uint32_t n, uint32_t *tile_sum, uint32_t *rec_off, hipStream_t s);
hipError_t launch_kmm_extract_write(const KmmExtractArgs &A, hipStream_t s);
hipError_t launch_kmm_group_scan(const KmmGroupArgs &A, uint32_t *tile_sum, uint32_t *emit_at, hipStream_t s);
hipError_t launch_kmm_emit(const KmmGroupArgs &A, const uint32_t *emit_at, unsigned long long *pair, uint16_t *diag, hipStream_t s);
hipError_t launch_kmm_vote_scan(const unsigned long long *pair, uint32_t n_pairs, bool nucl, uint32_t *tile_sum, uint32_t *kept_at, hipStream_t s);
hipError_t launch_kmm_vote(const unsigned long long *pair, const uint16_t *diag, uint32_t n_pairs, bool nucl, const uint32_t *kept_at, uint32_t n_kept, uint32_t n,
                           uint32_t *kept_rep, unsigned long long *offsets, mmgpu_pf_hit *records, hipStream_t s);
hipError_t launch_kmm_handover(const unsigned long long *offsets, uint32_t n, const mmgpu_pf_hit *records, uint32_t n_entries, uint32_t *hit_query,
                               mmgpu_rescore_pair *pairs, hipStream_t s);
inline uint32_t kmm_scan_tiles(uint64_t n) { return (uint32_t)((n + 2047) / 2048); }      // tile sums a scan of n elements needs

// ---------------------------------------------------------------------------------------------------------
// prefilter (pf_kernels.hip)
constexpr int PF_T = 4096;             // arrival-ordered index entries per tile (2048: 22 % slower, more tiles)
constexpr int PF_IDS_PER_BIN = 4096;   // targets per replay bin (one 16 KB LDS state table per wavefront)
constexpr int PF_SAT_CAP = 1024;        // saturated elements per query exported in nucleotide mode (16 KB per query)
constexpr int PF_CAND0 = 32;            // candidates per (query, bin) kept in the dense array
constexpr int PF_QSTAGE = 2048;         // longest query whose residues the ungapped kernel stages in LDS
constexpr int PF_MAX_HITS = 4096;      // largest --max-seqs the select kernel sorts in LDS (larger lists: global scratch, PF_MAX_HITS_BIG)
constexpr int PF_MAX_HITS_BIG = 131072;   // == MMGPU_PF_MAX_HITS

struct PfList {        // index list of one similar k-mer of one query position
    uint32_t start;    // first entry in the index arrays
    uint32_t len;
    uint32_t lprefix;  // entries of earlier lists of the same position
    uint32_t pos;      // batch-global query position
};

struct PfCand {        // double-diagonal candidate / surviving element
    uint32_t id;
    uint32_t arr;      // arrival index of the emitting index entry within its query
    uint32_t score;    // exact ungapped score
    uint16_t diag;
    uint16_t pad;
};

// PfCand::score of an element whose count is NOT min(255, exact score): a target of 32768 residues or more in a full batch of
// UngappedAlignment::scoreDiagonalAndUpdateHits takes its count from another element's target (pf_long_kernel), while the rescoring of
// a saturated element (scoreSingleSequence) reads its own.  Bit 31 set: count in bits 30..23, exact score in bits 22..0.
__host__ __device__ inline uint32_t pf_el_count(uint32_t s) { return (s & 0x80000000u) ? ((s >> 23) & 0xFFu) : (s < 255u ? s : 255u); }
__host__ __device__ inline uint32_t pf_el_exact(uint32_t s) { return (s & 0x80000000u) ? (s & 0x7FFFFFu) : s; }

constexpr int PF_PROW = 32;            // bytes per position of the profile-query score rows (21 letters used)
constexpr int PF_PROF_LETTERS = 20;    // Sequence::PROFILE_AA_SIZE

struct PfKmerArgs {
    const uint8_t *q_res;      // batch residues, concatenated
    const int16_t *q_thr;      // per position: adjusted k-mer threshold, -1 = no window / X in window
    uint32_t n_pos;
    uint8_t pat[16];           // Sequence::aaPosInSpacedPattern
    uint32_t kalph, n3;
    uint32_t kbase;            // base of the k-mer index (pf_kmers_exact_kernel): kalph, or the full alphabet for profile targets
    const int16_t *s3;         // [n3][n3] ScoreMatrix::score of the 3-mer matrix (no padding columns)
    const uint32_t *i3;        // [n3][n3] ScoreMatrix::index
    const uint32_t *offsets;   // IndexTable::offsets, [kalph^k + 1]
    const uint32_t *nonempty;  // one bit per k-mer: list not empty (null: not used, the index is dense)
    const uint4 *cofs;         // compact offset table (pf_kernels.hip: 16-byte blocks of 12 k-mers), null = look-ups read `offsets`
    const uint16_t *cum3;      // [n3][cum_w]: cum3[row][k] = number of entries of the row with score >= score_min + k
    uint32_t cum_w;
    int32_t score_min;
    // k = 7 only: the 2-mer tables
    int k;
    const int16_t *s2;         // [n2][n2]
    const uint32_t *i2;
    const uint16_t *cum2;      // [n2][cum2_w]
    uint32_t cum2_w;
    int32_t score2_min;
    // profile queries (Sequence::profile_score / profile_index of the positions of profile queries, 20 per position,
    // sorted descending as Sequence::mapProfile leaves them): q_kind[gp] = 1 marks their positions (null: none in the batch)
    const uint8_t *q_kind;
    const int16_t *prof_score;    // [n_pos][20]
    const uint8_t *prof_letter;   // [n_pos][20]
    int exact;                 // takeOnlyBestKmer: every window matches its own k-mer only (QueryMatcher.cpp:279-282)
    const uint32_t *order;     // [n_pos] work order of the positions (launch_pf_order: grouped by the window's last 3-mer), null = as stored
    // count pass
    uint32_t *nsim;
    // emit pass
    const uint32_t *list_base; // [n_pos + 1]
    PfList *lists;
    uint32_t *pos_entries;
};

struct PfSplitArgs {
    const uint32_t *tile_q, *tile_idx;
    const uint32_t *q_off;            // [nq + 1]
    const uint32_t *q_entries;        // [nq]
    const uint32_t *pos_entry_base;   // [n_pos + 1], relative to the query
    const uint32_t *list_base;        // [n_pos + 1]
    const PfList *lists;
    const uint64_t *idx_entries;      // IndexEntryLocal re-packed to 8 bytes: seqId | position_j << 32 (one line per list)
    uint32_t bins;
    uint32_t *split;                  // [n_tiles][PF_T] (id >> log2 bins) | low diagonal byte << 12 | slot in tile << 20
    uint8_t *split_hi;                // [n_tiles][PF_T] high diagonal byte (same layout)
    uint16_t *bin_off;                // [n_tiles][bins + 1]
    uint32_t *bucket_count;           // [nq][bins]
};

struct PfDedupArgs {
    uint32_t n_queries, bins;         // queries of this launch: q_first .. q_first + n_queries - 1 of the batch
    uint32_t q_first;
    uint32_t cand_origin;             // cand/surv hold the entries cand_origin .. of the batch (stage chunks, pf_api.hip)
    const uint32_t *q_tile_base, *q_ntiles;
    const uint32_t *split;
    const uint8_t *split_hi;
    const uint16_t *bin_off;
    const uint32_t *cand_base;        // [nq * bins + 1]
    PfCand *cand, *surv;
    PfCand *cand_small;               // [nq * bins][PF_CAND0]
    uint32_t *surv_count;             // [nq]
    uint32_t *cand_count;             // [nq * bins]
    uint64_t *cell_counter;           // [nq] ungapped cells scored per query (statistics), may be null
    const uint32_t *q_off;
    const uint8_t *q_res;
    const int8_t *q_corr;             // UngappedAlignment::aaCorrectionScore per position
    const int8_t *mat;                // ungapped matrix, alphabet x alphabet
    int alphabet;
    // profile queries: UngappedAlignment::queryProfile rows (createProfile's profile branch, UngappedAlignment.cpp:405-411),
    // [n_pos][PF_PROW] int8, letter-indexed, filled for the positions of profile queries; q_isprof[q] picks the path
    const int8_t *q_rows;
    const uint8_t *q_isprof;
    // nucleotide searches (QueryMatcher.cpp:147-177): every bucket goes through pf_keepmax_nucl_kernel
    int nucl;
    uint32_t sort_cap;                // foundDiagonalsSize / 2: the branch is skipped for larger candidate sets (:146)
    uint32_t *q_ncand;                // [nq] double-diagonal candidates of the query (nucleotide mode only)
    // nucleotide mode: the saturated elements of every query, for the host's replay of the reference's std::sort (mmgpu_pf_fetch)
    PfCand *sat;                      // [nq][sat_cap], any order
    uint32_t *q_nsat;                 // [nq] their number (may exceed sat_cap: then the list is incomplete)
    uint32_t sat_cap;
    const uint8_t *t_res;
    const uint32_t *t_off4, *t_len;
    uint32_t min_diag_score;
    uint32_t *q_flags;                // [nq] bit 0: a candidate's target has >= 32768 residues (UngappedAlignment::computeLongScore,
                                      // UngappedAlignment.cpp:295-312): pf_long_kernel scores those and clears the bit; where it
                                      // does not run or gives up (sharded / overflow-path / nucleotide queries) the host runs the query
    uint32_t ref_bins;                // BINCOUNT of the reference's CacheFriendlyOperations: the order of its result array (pf_long_kernel)
    // work list of the buckets with more than 64 candidates (bucket index relative to the launch's first bucket), appended by the
    // replay kernel, walked by pf_ungapped_kernel / pf_keepmax_kernel; null: those kernels run one wavefront per bucket of the launch
    uint32_t *big_list, *big_count;
    // overflow emulation (null when the batch has no query on the overflow path)
    const uint32_t *q_nseg;           // [nq] databaseHits flushes of the query (0 = ordinary query)
    const uint32_t *seg_start;        // [nq][PF_MAX_SEG + 2] arrival index at which segment k starts
    // buckets the compact replay hands to the full-state one (more emitting targets than its table holds)
};

struct PfSelectArgs {
    uint32_t q_first, cand_origin;    // as in PfDedupArgs
    int kmer_score;                   // --diag-score 0: scores are match counts (no rescoring, self hit 255)
    const PfCand *surv;
    const uint32_t *cand_base;        // survivors of query q start at cand_base[q * bins]
    uint32_t bins;
    const uint32_t *surv_count;
    const uint32_t *q_identity;
    const int32_t *q_self_score;
    uint32_t max_hits, min_diag_score, ref_bins;
    mmgpu_pf_hit *hits;
    uint32_t hit_stride;
    uint32_t *hit_count, *q_diag_thr;
    // shard of a multi-GPU run (mmgpu_pf_set_shard): exchange records instead of hit lists
    mmgpu_pf_xhit *xhits;             // null = ordinary run
    const uint32_t *global_ids;       // [n_targets] local -> global id
    const uint32_t *q_nseg;           // overflow-path queries (their order key is not shard independent), may be null
    uint32_t *q_flags;                // long-sequence queries (scores not computed on the device), may be null; bit 1 is set here (below)
    // diagonal scoring of sequences: a query whose double-diagonal candidates number foundDiagonalsSize / 2 or more MAY take the
    // reference's unsorted branch (QueryMatcher.cpp:188,204-214: filter, unstable std::sort, exact scores, no rescoring) - the
    // candidate total bounds resultSize from above, such queries are flagged (bit 1 -> MMGPU_PF_SAT_TIE) and left to the host
    const uint32_t *cand_count;       // [nq * bins] candidates per (query, bin), null = no check (modes that count elsewhere)
    uint32_t cand_cap;
    int nucl;                         // nucleotide searches: saturated elements are ordered by target id (QueryMatcher.cpp:154)
    // max_hits above PF_MAX_HITS: the selected elements are sorted in global scratch, [nq][big_stride] keys + diagonals
    uint64_t *big_keys;
    uint16_t *big_diags;
    uint32_t big_stride;              // power of two >= max_hits
    const uint32_t *q_off, *peb, *list_base;
    const PfList *lists;
};

// ---- multi-GPU merge (pf_shard_kernels.hip)
constexpr int PF_XMERGE_CAP = 4096;    // exchange records per query (n_shards * stride) the merge kernel holds in LDS
struct PfXMergeArgs {
    const mmgpu_pf_xhit *xhits;       // [n_shards][nq][stride]
    const uint32_t *counts;           // [n_shards][nq]
    uint32_t n_shards, nq, stride;
    uint32_t max_hits, min_diag_score, ref_bins;
    const int32_t *q_self_score;      // [nq]
    const uint32_t *q_identity;       // [nq] GLOBAL id of the self hit, 0xFFFFFFFF = none
    mmgpu_pf_hit *out_hits;           // [nq][out_stride]
    uint32_t out_stride;
    uint32_t *out_counts;             // [nq]
    uint32_t *out_flags;              // [nq] bit 0: an overflow-path element took part (tie order at the cut not exact)
};
hipError_t launch_pf_xmerge(const PfXMergeArgs &A, hipStream_t s);

struct PfLocalizeArgs {
    const mmgpu_pf_hit *hits;         // [nq][stride] global ids
    const uint32_t *counts;
    uint32_t nq, stride, shard;
    const uint32_t *shard_of, *local_id;   // [global_db_size]
    mmgpu_pf_hit *local_hits;         // [nq][stride] local ids, list order kept
    uint32_t *local_counts;
    uint32_t *local_slot;             // [nq][stride] position of the hit in the query's merged list
};
hipError_t launch_pf_localize(const PfLocalizeArgs &A, hipStream_t s);

// ---- alignment records of the pairs a rank owns, gathered over the ranks (pf_shard_kernels.hip) ----
struct SwOwnedRec {                   // 32 bytes: one aligned pair and where it goes in the merged-list order
    mmgpu_sw_hit hit;
    uint32_t slot;                    // q * stride + position in query q's merged list
    uint32_t pad;
};
struct SwOwnedPackArgs {
    const mmgpu_sw_hit *res;          // [nq * stride] the batch's records, local list order
    const uint32_t *local_counts;     // [nq]
    const uint32_t *local_slot;       // [nq * stride]
    uint32_t nq, stride;
    SwOwnedRec *send;                 // [cap]
    uint32_t cap;
    uint32_t *counter;                // [2]: records packed, records that did not fit (overflow)
};
struct SwOwnedScatterArgs {
    const SwOwnedRec *recv;           // [n_ranks][cap]
    const uint32_t *counters;         // [n_ranks][2]
    uint32_t n_ranks, cap, n_slots;
    mmgpu_sw_hit *full;               // [n_slots], zeroed before
    uint32_t *status;                 // [2]: records scattered, ranks whose send buffer overflowed
};
hipError_t launch_sw_owned_pack(const SwOwnedPackArgs &A, hipStream_t s);
hipError_t launch_sw_owned_scatter(const SwOwnedScatterArgs &A, hipStream_t s);

constexpr int PF_MAX_SEG = 62;         // databaseHits flushes per query the device emulates (QueryMatcher.cpp:310-346)

struct PfSegArgs {
    const uint32_t *ovf_queries;      // queries that gather >= maxDbMatches entries
    uint32_t n_ovf;
    const uint32_t *q_off, *list_base, *pos_entry_base;
    const PfList *lists;
    uint64_t cap;                     // maxDbMatches
    uint32_t *seg_start;              // [nq][PF_MAX_SEG + 2]
    uint32_t *q_nseg;                 // [nq]; PF_MAX_SEG + 1 = more flushes than emulated
    uint32_t *q_final;                // [nq] entries of the last segment
    const uint32_t *q_entries;
};

struct PfOvfElem {                    // element of foundDiagonals on the overflow path
    uint32_t id;
    uint32_t score;                   // exact ungapped score, 0 = not scored yet (CounterResult::count == 0)
    long long ord;                    // position key: order inside a CPU bin through the merges (reversal = negation)
    uint16_t diag;
    uint16_t pad0;
    uint32_t pad1;
};

struct PfOvfArgs {
    PfDedupArgs D;
    const uint32_t *ovf_queries;
    uint32_t n_ovf;
    uint32_t step;                    // flush number 1..nseg, nseg + 1 = the final merge
    const uint32_t *q_final;
    const uint64_t *ovf_base;         // [n_ovf] first element of the query's region in buf_a / buf_b
    PfOvfElem *buf_a, *buf_b;
    uint32_t *o_count;                // [n_ovf * bins]
    uint32_t *totals;                 // [n_ovf][PF_MAX_SEG + 2] overflowHitCount after flush k
};

hipError_t launch_pf_segments(const PfSegArgs &A, hipStream_t s);
hipError_t launch_pf_overflow(const PfOvfArgs &A, hipStream_t s);

constexpr int PF_MERGE_CAP = 8192;     // hits per query the split-merge kernel sorts in LDS

struct PfMergeArgs {
    const mmgpu_pf_hit *hits;    // [n_splits][nq][stride]
    const uint32_t *counts;      // [n_splits][nq]
    uint32_t n_splits, nq, stride;
    uint32_t id_offset[64];
    mmgpu_pf_hit *out_hits;      // [nq][n_splits * stride]
    uint32_t *out_counts;        // [nq]
};

hipError_t launch_pf_merge(const PfMergeArgs &A, hipStream_t s);
hipError_t launch_pf_kmers(const PfKmerArgs &A, bool emit, hipStream_t s);
size_t pf_cofs_bytes(uint64_t table);
hipError_t launch_pf_cofs(const uint32_t *offsets, uint64_t table, void *cofs, hipStream_t s);
// persisted device layout (db_kernels.hip): checksum of a section where it lies on the device; the properties the kernels rely on
hipError_t db_section_checksum(const void *dev, size_t bytes, unsigned long long *scratch, uint64_t *sum, hipStream_t s);
hipError_t db_validate_layout(const uint32_t *off4, const uint32_t *len, uint32_t n, uint64_t res_bytes, uint32_t max_len, const uint32_t *offsets,
                              uint64_t table, const uint64_t *entries, uint64_t n_entries, uint32_t *scratch, uint32_t *bad, hipStream_t s);
hipError_t launch_pf_tiles(const uint32_t *q_tile_base, const uint32_t *q_ntiles, uint32_t nq, uint32_t *tile_q, uint32_t *tile_idx, hipStream_t s);
hipError_t launch_pf_bitmap(const uint32_t *offsets, uint64_t table, uint32_t *bitmap, unsigned long long *nonempty, hipStream_t s);
hipError_t launch_pf_scan(const uint32_t *in, const uint32_t *q_off, uint32_t nq, const uint64_t *base, uint32_t *out,
                          uint64_t *totals, hipStream_t s);
hipError_t launch_pf_split(const PfSplitArgs &A, uint32_t n_tiles, hipStream_t s);
hipError_t launch_pf_dedup(const PfDedupArgs &A, hipEvent_t after_replay, hipEvent_t after_ungapped, hipStream_t s);
hipError_t launch_pf_count(const PfDedupArgs &A, hipEvent_t after_a, hipEvent_t after_b, hipStream_t s);   // --diag-score 0
hipError_t launch_pf_long(const PfDedupArgs &A, bool long_queries, hipStream_t s);   // after launch_pf_dedup: sequences of >= 32768 residues
hipError_t launch_pf_select(const PfSelectArgs &A, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------
// index construction (ix_kernels.hip)
struct IxArgs {
    const uint8_t *t_res;
    const uint32_t *t_off4, *t_len;
    uint32_t n_targets;
    int k, pattern_len, kmer_thr;
    uint32_t kalph;
    uint8_t pat[16];
    int8_t self_score[32];      // (char) subMatrix[a][a], IndexBuilder.cpp:11-22
    uint32_t *counts;           // [table]: count pass = list lengths, fill pass = write cursors
    const uint32_t *offsets;    // [table + 1] (fill pass)
    uint64_t *entries;          // fill pass: seqId | position << 32, unordered inside a list
    uint32_t *scratch;          // one uint32 per residue slot, used by targets with more than 4096 windows
};

struct IxSortArgs {
    uint64_t table;
    const uint32_t *offsets;
    const uint64_t *src;
    uint64_t *dst;
    uint32_t *long_lists;       // k-mers whose list has more than 16 entries
    uint32_t *n_long;
    uint32_t long_cap;
};

hipError_t launch_ix_target(const IxArgs &A, bool fill, hipStream_t s);

// tantan masking of the resident targets (tantan_kernel.hip)
struct TantanArgs {
    const uint8_t *t_res;              // unmasked residues
    uint8_t *out_res;                  // the masked copy (same layout; only masked positions are written)
    const uint32_t *t_off4, *t_len;
    const uint32_t *order;             // [n] target ids, longest first: 64 consecutive ones share a wavefront
    uint32_t n;
    const double *lr;                  // [alphabet][alphabet] likelihood ratios (ProbabilityMatrix, BaseMatrix.h:83-101)
    const double *b2f;                 // [50] background -> repeat state probabilities (Tantan constructor, tantan.cpp:118-131)
    int alphabet;
    double repeat_prob, repeat_end_prob, min_mask_prob;
    uint8_t mask_letter;
    float *probs;                      // forward background probabilities, [wave][position][64 lanes]
    double *scales;                    // scale factors, [wave][position / 16][64 lanes]
    const uint64_t *wave_prob_base, *wave_scale_base;
    unsigned long long *n_masked;
};
hipError_t launch_tantan_mask(const TantanArgs &A, hipStream_t s);
// code-object loading ahead of the first launch (mmgpu_warmup)
void warm_sw();
void warm_block();
void warm_pf();
void warm_ix();
void warm_tantan();
void warm_bt();
hipError_t launch_ix_sort_short(const IxSortArgs &A, hipStream_t s);
hipError_t launch_ix_sort_long(const IxSortArgs &A, uint32_t n_long, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------
// banded traceback (bt_kernel.hip)
struct BtJob {
    uint32_t slot;      // where the caller wants the result (index into info[])
    uint32_t query, target;
    int32_t q_start, q_end, t_start, t_end, score;
    uint64_t bt_off;
};

struct BtLaunch {
    const BtJob *jobs;
    uint32_t n_jobs;
    const uint8_t *q_res;
    const int8_t *q_cb;
    const uint32_t *q_off;
    const int8_t *q_prof;       // profile queries, as in SwLaunch (banded_sw<PROFILE_SEQ>, StripedSmithWaterman.cpp:1565-1567)
    const uint32_t *q_prof_off;
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const int8_t *mat;
    int alphabet, gap_open, gap_extend;
    uint32_t *scratch;          // [blocks][words_per_lane][64 lanes]
    uint32_t words_per_lane;
    uint32_t band_cap;          // words per band row (3 rows), the rest of words_per_lane holds direction bits
    mmgpu_sw_bt *info;          // indexed by BtJob::slot
    char *bt;
    // wave kernel (bt_wave_kernel.hip): one pool of direction bytes, carved up by a bump allocator
    uint8_t *dir_pool;
    unsigned long long dir_pool_bytes;
    unsigned long long *dir_cursor;
};

// ---- block aligner on the device (block_kernel.hip; row a15): int16-range hits ----
// (the tier sizes, BlockJob, Block2Job and BkBlock: block_plan.h)
struct BlockLaunch {
    const BlockJob *jobs;
    uint32_t n_jobs;
    const uint8_t *q_res;
    const int8_t *q_cb;
    const uint32_t *q_off;
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const int8_t *q_prof;         // profile queries, as in SwLaunch: int8 [alphabet][qlen] per query; null = none in the batch
    const uint32_t *q_prof_off;
    int alphabet;
    const int8_t *scores;         // AAMatrix::scores [27 * 32] as ssw_init leaves it (new_simple(1, -1) + set_num of the matrix)
    int gap_open, gap_extend;     // the crate's convention: negative
    mmgpu_sw_block *out;
    const uint64_t *bt_off;
    char *bt;
    uint8_t *pool;                // scratch slots: block list + trace of one pair
    uint64_t slot_bytes;
    uint32_t n_pool_slots;
    uint32_t *pool_busy;
    // test aid (mmgpu_sw_block_growth): per pair 1 + 4 * growth_cap words - the number of blocks of the pair's last alignment run and
    // (i, j, height << 16 | width, right) of each, i.e. Trace::block_start / block_size / right when align_core returns; null = off
    uint32_t *growth = nullptr;
    uint32_t growth_cap = 0;
};
// tier 0: blocks up to BLOCK_MAX_SIZE rows (LDS), 1: up to BLOCK_MID_SIZE (LDS), 2: up to BLOCK_REF_MAX_SIZE rows, border arrays
// in the first 8 * 4096 * 2 bytes of the pair's scratch slot
hipError_t launch_sw_block(const BlockLaunch &L, int tier, hipStream_t stream);

// ---- the same aligner, four pairs per wavefront (block4_kernel.hip): sequence queries; what a launch answers MMGPU_BLOCK_TOO_LARGE
// goes to the next form ----
struct Block2Launch {
    const Block2Job *jobs;
    uint32_t n_jobs;
    uint32_t *counter;            // the queue's head (zero before the launch)
    const uint8_t *q_res;
    const int8_t *q_cb;
    const uint32_t *q_off;
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const int8_t *scores;         // AAMatrix::scores [27 * 32], as BlockLaunch::scores
    int gap_open, gap_extend;     // the crate's convention: negative
    mmgpu_sw_block *out;
    const uint64_t *bt_off;       // multiples of four
    char *bt;                     // null: no strings
    uint8_t *pool;
    uint32_t *growth = nullptr;   // test aid, as BlockLaunch::growth
    uint32_t growth_cap = 0;
    uint8_t *ck_pool = nullptr;   // block4_kernel.hip: checkpoint arrays, 8 * rows bytes per row of a wavefront (4 rows a wavefront; skewed form: one)
    uint32_t trace_bytes = 0;     // walk kernel: the trace is the skewed form's (a byte per cell)
};
// trace = false: start positions only (no scratch, no walk)
// ---- four pairs per wavefront, one 16-lane DPP row = one vector of the crate = one pair (block4_kernel.hip); same launch record ----
constexpr int BLOCK4_MAX_SIZE = 128;     // (tuning aid: MMGPU_BLOCK4_ROWS=128) 1 KB of LDS per pair
constexpr int BLOCK4_LARGE_SIZE = 256;   // the default: 2 KB of LDS per pair
constexpr int BLOCK4_SKEW_SIZE = 1024;   // the skewed form (one pair per wavefront, rows pipelined over columns): first launch; the second holds BLOCK_REF_MAX_SIZE
hipError_t launch_sw_block4(const Block2Launch &L, bool trace, int form, uint32_t n_waves, hipStream_t stream);
hipError_t launch_sw_block4_walk(const Block2Launch &L, hipStream_t stream);
void warm_block4();

// ---- search semantics on the device (block_select.hip, mmgpu_sw_block_starts) ----
struct BlockSelectArgs {
    const mmgpu_sw_hit *res;      // the batch's result records
    uint32_t pairs;
    const uint32_t *qout_off;     // [n_queries + 1] first result slot of every query
    uint32_t n_queries;
    const int32_t *q_minstart;
    const uint32_t *slot_target;  // target id of every result slot
    BlockJob *jobs;               // out: the selected pairs, slot = position in this list
    uint32_t *pair_of_slot;       // out: their result slots
    mmgpu_sw_block *blk;          // out: their answers, initialised (MMGPU_BLOCK_TOO_LARGE until a kernel decides)
    uint32_t *count;              // out (zero before the launch)
    uint32_t cap;
};
struct BlockScatterArgs {
    const mmgpu_sw_block *blk;
    const uint32_t *pair_of_slot;
    uint32_t n;
    mmgpu_sw_hit *res;
    uint8_t *rev_force;           // [pairs], zero before the launch: set for the pairs the block aligner declined
    uint32_t *counts;             // [3] OK / DECLINED / TOO_LARGE (zero before the launch)
};
hipError_t launch_block_select(const BlockSelectArgs &A, hipStream_t stream);
hipError_t launch_block_scatter(const BlockScatterArgs &A, hipStream_t stream);

hipError_t launch_sw_traceback(const BtLaunch &L, hipStream_t stream);
hipError_t launch_sw_traceback_wave(const BtLaunch &L, hipStream_t stream);

// the resident ids by length, longest first (counting sort; ids ascend inside a length), and where each length starts:
// first_le[L] = position of the first target of length <= L in `order` (both scans cut their window slices out of it)
inline void order_targets_by_length(const std::vector<uint32_t> &len, std::vector<uint32_t> &order, std::vector<uint32_t> &first_le) {
    const uint32_t n = (uint32_t)len.size();
    std::vector<uint32_t> start(65536 + 1, 0);      // after the prefix sum: start[k] = targets longer than 65535 - k = where length 65535 - k begins
    for (uint32_t i = 0; i < n; i++) start[65535 - len[i] + 1]++;
    for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
    first_le.resize(65536);
    for (uint32_t L = 0; L < 65536; L++) first_le[L] = start[65535 - L];
    order.resize(n);
    for (uint32_t i = 0; i < n; i++) order[start[65535 - len[i]]++] = i;
}
// positions [begin, end) of `order` whose targets have lengths in the inclusive window [lo, hi]
inline void window_slice(const std::vector<uint32_t> &first_le, uint32_t n, uint32_t lo, uint32_t hi, uint32_t *begin, uint32_t *end) {
    *begin = hi >= 65535u ? 0u : first_le[hi];
    *end = lo == 0 ? n : (lo > 65535u ? 0u : first_le[lo - 1]);
    if (*end < *begin) *end = *begin;
}

// host-side loops over targets / index entries / queries: plain std::thread chunks (the library carries no OpenMP runtime)
inline unsigned host_threads() {
    unsigned n = std::thread::hardware_concurrency();
    return n == 0 ? 1 : std::min(n, 64u);
}

template <typename F>
inline void parallel_for(size_t n, F f) {
    const unsigned nt = (unsigned)std::min<size_t>(host_threads(), std::max<size_t>(n, 1));
    if (nt <= 1 || n < 4096) {
        f((size_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const size_t a = std::min(n, (size_t)t * chunk), b = std::min(n, a + chunk);
        if (a < b) th.emplace_back([=] { f(a, b); });
    }
    for (auto &x : th) x.join();
}

// ---------------------------------------------------------------------------------------------------------
// host-side plumbing shared by the *_api.hip translation units
extern thread_local std::string g_last_error;
inline int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess)                                                                             \
            return mmgpu::fail(MMGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));         \
    } while (0)

// every device buffer of the library is allocated and freed through these two
inline hipError_t dev_malloc(void **p, size_t n) { return hipMalloc(p, n); }
inline void dev_free(void *p) {
    if (p) (void)hipFree(p);
}

// Freed device blocks of one context, kept for the next batch: a streaming search prepares and frees one alignment
// batch per prefilter batch, and hipMalloc / hipFree (which also drains the device) per buffer would cost more than
// the kernels.  Reuse is safe because every use of a block is ordered on the context's stream.  Sizes are rounded to 3 significant bits so that batches of
// similar shape hit the same classes.
struct BlockCache {
    std::multimap<size_t, void *> blocks;
    size_t cached = 0;
    bool closed = false;   // the context is gone (batches may outlive it): blocks go straight back to the runtime
    std::mutex lock;       // a prefilter thread and an alignment thread may work on one context (the fused search of the drop-in)
    // a third of the device's memory (96 GB of 288), read once; an allocation that fails trims the cache and retries
    static size_t limit() {
        static const size_t v = []() -> size_t {
            size_t f = 0, t = 0;
            if (hipMemGetInfo(&f, &t) != hipSuccess || t == 0) return (size_t)16 << 30;
            return t / 3;
        }();
        return v;
    }
    static size_t round_up(size_t n) {
        if (n <= 512) return 512;
        int top = 63 - __builtin_clzll((unsigned long long)n);
        const size_t step = (size_t)1 << (top - 2);
        return (n + step - 1) & ~(step - 1);
    }
    // the smallest parked block of cap .. 2 cap bytes (cap becomes its size): the buffers of consecutive batches differ in size by
    // what their queries happen to need, and on some hosts a fresh hipMalloc costs 25 - 40 ms per GB
    void *take(size_t &cap) {
        std::lock_guard<std::mutex> guard(lock);
        auto it = blocks.lower_bound(cap);
        if (it == blocks.end() || it->first > 2 * cap) return nullptr;
        void *p = it->second;
        cap = it->first;
        blocks.erase(it);
        cached -= cap;
        return p;
    }
    void give(void *p, size_t cap) {
        std::lock_guard<std::mutex> guard(lock);
        if (closed || cached + cap > limit()) { dev_free(p); return; }
        blocks.emplace(cap, p);
        cached += cap;
    }
    void trim() {
        std::lock_guard<std::mutex> guard(lock);
        for (auto &kv : blocks) dev_free(kv.second);
        blocks.clear();
        cached = 0;
    }
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    size_t cap = 0;                // allocated size when the block came from / goes back to a cache
    std::shared_ptr<BlockCache> cache;   // optional (bind): where freed blocks go
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap), cache(std::move(o.cache)) { o.p = nullptr; o.bytes = 0; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; cap = o.cap; cache = std::move(o.cache);
            o.p = nullptr; o.bytes = 0; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void bind(const std::shared_ptr<BlockCache> &c) {
        cache = c;
    }
    void release() {
        if (!p) return;
        if (cache && cap) cache->give(p, cap);
        else dev_free(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(size_t n) {
        release();
        bytes = n;
        if (n == 0) return hipSuccess;
        if (cache) {
            cap = BlockCache::round_up(n);
            p = cache->take(cap);
            if (p) return hipSuccess;
            hipError_t e = dev_malloc(&p, cap);
            if (e != hipSuccess) {      // out of memory with blocks parked in the cache: give them back and retry
                (void)hipGetLastError();
                cache->trim();
                e = dev_malloc(&p, cap);
            }
            if (e != hipSuccess) { p = nullptr; cap = 0; bytes = 0; }   // (bytes = 0: a later, smaller reserve() must allocate)
            return e;
        }
        const hipError_t e = dev_malloc(&p, n);
        if (e != hipSuccess) { p = nullptr; bytes = 0; (void)hipGetLastError(); }
        return e;
    }
    // grow-only (contents are not preserved)
    hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : alloc(n + n / 8); }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A non-blocking stream of one call, beside the context's.  The holder waits for the stream before it destroys it: declare it AFTER
// the buffers its work uses, so that a return with a launch in flight ends the launch before the buffers go back to the cache.
struct SideStream {
    hipStream_t s = nullptr;
    SideStream() = default;
    SideStream(const SideStream &) = delete;
    SideStream &operator=(const SideStream &) = delete;
    ~SideStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// A pinned staging buffer and the event of the last copy out of it (with_event = false: a buffer for blocking copies, no event)
struct PinnedStage {
    uint8_t *p = nullptr;
    hipEvent_t moved = nullptr;
    PinnedStage() = default;
    PinnedStage(const PinnedStage &) = delete;
    PinnedStage &operator=(const PinnedStage &) = delete;
    ~PinnedStage() { if (p) (void)hipHostFree(p); if (moved) (void)hipEventDestroy(moved); }
    hipError_t reserve(size_t bytes, bool with_event = true) {
        const hipError_t e = hipHostMalloc((void **)&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        return with_event ? hipEventCreateWithFlags(&moved, hipEventDisableTiming) : hipSuccess;
    }
};

// Host -> device in chunks: a stream of its own and a ring of staging buffers.  The caller fills slot k (after reserve, or after
// wait when it has been used before), enqueues its copy on `up.s` and calls sent(k).  One thread per slot may do so at a time.  The
// holder waits for the stream before the staging memory goes.
struct UploadRing {
    SideStream up;
    std::vector<PinnedStage> slots;
    UploadRing() = default;
    UploadRing(const UploadRing &) = delete;
    UploadRing &operator=(const UploadRing &) = delete;
    ~UploadRing() { if (up.s) (void)hipStreamSynchronize(up.s); }
    hipError_t open(size_t n_slots) { slots = std::vector<PinnedStage>(n_slots); return up.create(); }
    hipError_t wait(size_t k) const { return hipEventSynchronize(slots[k].moved); }      // the last copy out of slot k
    hipError_t sent(size_t k) const { return hipEventRecord(slots[k].moved, up.s); }
};

template <typename T>
inline hipError_t upload(DevBuf &b, const std::vector<T> &v, hipStream_t s) {
    hipError_t e = b.alloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

// the same through a slice of pinned staging memory (base / cap / used: the caller's arena, large enough - upload_pinned_need):
// the copy is enqueued and the host goes on; the arena must stay untouched until the stream has passed the copy
inline size_t upload_pinned_need(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
template <typename T>
inline hipError_t upload_pinned(DevBuf &b, const std::vector<T> &v, hipStream_t s, void *base, size_t cap, size_t &used) {
    hipError_t e = b.alloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    const size_t n = v.size() * sizeof(T);
    if (!base || used + upload_pinned_need(n) > cap) return hipMemcpyAsync(b.p, v.data(), n, hipMemcpyHostToDevice, s);
    void *st = static_cast<char *>(base) + used;
    used += upload_pinned_need(n);
    memcpy(st, v.data(), n);
    return hipMemcpyAsync(b.p, st, n, hipMemcpyHostToDevice, s);
}

// nucleotide alignment step (nucl_kernel.hip; NuclLaunch is declared in nucl_core.h)
hipError_t launch_nucl_align(const NuclLaunch &L, unsigned blocks, hipStream_t stream);     // 16 lanes per alignment
hipError_t launch_nucl_align_wave(const NuclLaunch &L, unsigned blocks, hipStream_t stream);   // one wavefront per alignment, state in registers (nucl_wave.h): the default

hipError_t launch_pf_order(const PfKmerArgs &A, uint32_t *order, const std::shared_ptr<BlockCache> &cache, hipStream_t s);   // pf_order.hip

struct PfIndex;   // pf_index.h

}  // namespace mmgpu

namespace mmgpu {
// communicator over the contexts that hold the shards of one target database (comm.hip)
struct Comm {
    void *nccl = nullptr;          // ncclComm_t; null = the copy transport of a one-process run (multi_api.hip)
    int rank = 0, n_ranks = 1;
    std::string transport;         // "rccl" | "copy"
};
}  // namespace mmgpu

struct mmgpu_ctx {
    int device = 0;
    mmgpu::Comm *comm = nullptr;   // multi-GPU runs: mmgpu_comm_init_rank / mmgpu_init_multi
    hipStream_t stream = nullptr;
    bool owns_stream = false;      // mmgpu_init_multi gives every context a stream of its own
    mmgpu::DeviceDb db;
    std::vector<uint32_t> h_len;   // host copy of target lengths (scheduling)
    uint32_t mean_len = 0;
    int compute_units = 0;
    std::string name;
    mmgpu::PfIndex *pf = nullptr;  // prefilter index resident in HBM (pf_index.h, pf_index_api.hip)
    // the prefilter's view of the targets when it differs from the alignment's: residues with tantan-masked letters replaced by
    // X (mmgpu_pf_mask_targets; same offsets / lengths as `db`).  null: the prefilter reads db.res (--mask 0, or a caller that
    // loaded an already masked SequenceLookup)
    uint8_t *pf_masked_res = nullptr;
    const uint8_t *pf_res() const { return pf_masked_res ? pf_masked_res : db.res; }
    // shard of a multi-GPU run (mmgpu_pf_set_shard); the flag goes with the resident database (db_release)
    struct Shard {
        bool on = false;
        uint32_t n_shards = 1, shard = 0, global_n = 0;
        mmgpu::DevBuf d_global_ids, d_shard_of, d_local_id;
    } shard;
    std::shared_ptr<mmgpu::BlockCache> cache = std::make_shared<mmgpu::BlockCache>();   // device blocks of freed alignment batches
    // the alignment kernel groups run concurrently on side streams forked from / joined to `stream` (mmgpu_sw_run)
    hipStream_t side[4] = {};      // (SW_GROUPS of them are used)
    hipEvent_t fork = nullptr, join[4] = {};
    // pinned staging for the uploads of mmgpu_sw_prepare_from_pf: a copy from pageable memory blocks the calling thread until the
    // stream has reached it - i.e. until the prefilter batch before it has finished - and everything the host still had to do for
    // the alignment batch (ordering ~1e5 jobs) then ran with the device idle.  mmgpu_sw_block_starts receives its jobs and answers
    // through it.  Threading rule: one call at a time owns the arena, from PinnedLease::acquire (mmgpu_api.hip) - the only place that
    // grows, i.e. frees and reallocates, it - until the holder dies; a call that finds it taken (pinned_busy: a thread prepares the
    // next batch while another runs the block aligner on this one) uses pageable memory
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    std::atomic<bool> pinned_busy{false};
    // exhaustive ungapped scan (scan_api.hip): the [query][target] score bytes and the multi-tile boundary lines, grown to the
    // largest batch and kept; scan_serial names the batch whose scores the scratch holds (mmgpu_scan_debug_scores)
    mmgpu::DevBuf scan_scores, scan_park;
    uint64_t scan_serial = 0;
    // exhaustive gapped scan (gscan_api.hip): the [query][target] int32 scores of the last batch run, kept the same way
    mmgpu::DevBuf gscan_scores;
    uint64_t gscan_serial = 0;
};

// device memory for a context's long-lived buffers (targets, masked view): when the runtime is out of memory the blocks the
// context's own cache has parked go back first (DevBuf::alloc does the same for batch buffers)
inline hipError_t dev_malloc_ctx(mmgpu_ctx *c, void **p, size_t n) {
    hipError_t e = mmgpu::dev_malloc(p, n);
    if (e != hipSuccess && c && c->cache) {
        (void)hipGetLastError();
        c->cache->trim();
        e = mmgpu::dev_malloc(p, n);
    }
    return e;
}

struct mmgpu_pf_batch_t;
struct mmgpu_sw_batch_t;
namespace mmgpu {
// comm.hip
int comm_require_rccl();
int comm_group_start();
int comm_group_end();
int comm_init_all(mmgpu_ctx **ctxs, int n);
int comm_allgather(mmgpu_ctx *c, const void *send, void *recv, size_t bytes);
void comm_free(mmgpu_ctx *c);
// the phases of the two exchange steps (pf_api.hip, mmgpu_api.hip); mmgpu_pf_exchange_merge / mmgpu_sw_gather_owned run them on
// one context, multi_api.hip runs each phase over the contexts of a process (the collective inside an RCCL group)
struct XchgBlock { const void *send; void *recv; size_t bytes; };   // one all-gather: `bytes` per rank
int pf_xchg_begin(mmgpu_ctx *c, mmgpu_pf_batch_t *b, int n_ranks, XchgBlock blocks[2]);
int pf_xchg_merge(mmgpu_ctx *c, mmgpu_pf_batch_t *b, int n_ranks, const uint32_t *identity_global);
// sharded runs: the queries whose merged list is flagged inexact, run once more against a context that holds the whole database
// (mmgpu_pf_exchange_redo_unsplit; multi_api.hip applies one run's rows to every context of the process)
struct PfRedoRows {
    std::vector<uint32_t> q;            // the flagged queries
    std::vector<mmgpu_pf_hit> hits;     // [q.size()][stride]: the unsplit run's lists (ids of the whole database)
    std::vector<uint32_t> counts;
    std::vector<int32_t> status;        // the unsplit run's own status (MMGPU_PF_OK, or what the host has to do itself)
    uint32_t stride = 0;
};
int pf_redo_flagged(mmgpu_ctx *c, mmgpu_pf_batch_t *b, std::vector<uint32_t> &flagged);      // synchronises the context's stream
int pf_redo_run(mmgpu_ctx *full, const mmgpu_pf_params *par, const mmgpu_pf_query *qs, const std::vector<uint32_t> &flagged, PfRedoRows &rows);
int pf_redo_apply(mmgpu_ctx *c, mmgpu_pf_batch_t *b, const PfRedoRows &rows);               // synchronises the context's stream
const int32_t *pf_batch_redo_status(const mmgpu_pf_batch_t *b);      // [nq]: -1 = not re-run, else the unsplit run's status
int sw_gather_begin(mmgpu_ctx *c, mmgpu_sw_batch_t *b, int n_ranks, XchgBlock blocks[2]);
int sw_gather_finish(mmgpu_ctx *c, mmgpu_sw_batch_t *b, int n_ranks);
int sw_gather_overflowed(mmgpu_ctx *c, mmgpu_sw_batch_t *b, bool *overflowed);   // true once: the caller repeats the phases (dense buffers)
int pf_batch_merged_flags(mmgpu_pf_batch_t *b, const void **d_flags);
const int32_t *pf_batch_host_status(const mmgpu_pf_batch_t *b);
bool pf_batch_merged_lists(mmgpu_pf_batch_t *b, const mmgpu_pf_hit **hits, const uint32_t **counts, uint32_t *stride, uint32_t *nq);
void pf_index_free(mmgpu_ctx *c);   // pf_index_api.hip
void db_release(mmgpu_ctx *c);      // db_api.hip: the targets, masked view, index and shard flag of a context go (ResidentDb, pf_index.h)
// device-resident results of a prefilter batch that has been run (false if it has not)
bool pf_batch_device_lists(mmgpu_pf_batch_t *b, const mmgpu_pf_hit **hits, const uint32_t **counts, uint32_t *stride, uint32_t *nq);
// mmgpu_api.hip, for gscan_api.hip: a MMGPU_SW_SCORE_END batch over dense lists (mmgpu_sw_prepare's checks, queries, job rules and
// kernels; target_ids / n_targets of the queries are not read), and its kernel launches without the batch's own timing events
int sw_prepare_dense(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, const SwDenseLists &lists, mmgpu_sw_batch_t **out);
int sw_run_dense(mmgpu_ctx *c, mmgpu_sw_batch_t *b);

// scan_common.hip: what a batch of either exhaustive scan holds and does like the other's (mmgpu_scan_batch_t and
// mmgpu_gscan_batch_t derive from the record).  `who` is the entry point's name, the head of every message.
struct ScanBatchCommon {
    uint32_t nq = 0, n_targets = 0, max_hits = 0, stride = 0;
    int32_t min_score = 0;
    int alphabet = 0;
    const uint8_t *db_res = nullptr;      // the resident database the batch was prepared against (a reload invalidates the batch)
    uint64_t serial = 0;                  // names this batch in mmgpu_ctx::scan_serial / gscan_serial
    bool ran = false;
    DevBuf d_mat, d_hits, d_counts;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // around the last run
    ~ScanBatchCommon() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};
// the checks of a prepare call before and after the scan's own; have_args: the parameters, their matrix and the queries are there;
// score_size: bytes per entry of the [query][target] score scratch (4 GiB of it at most)
int scan_check_db(const char *who, const mmgpu_ctx *c, bool have_args, int alphabet);
int scan_check_size(const char *who, const mmgpu_ctx *c, uint32_t nq, uint32_t max_hits, size_t score_size);
void scan_fill_header(ScanBatchCommon *b, const mmgpu_ctx *c, uint32_t nq, int alphabet, int32_t min_score, uint32_t max_hits, uint64_t serial);
// the matrix, the list buffers, and the wait for the stream that ends a prepare call's uploads
int scan_upload_common(mmgpu_ctx *c, ScanBatchCommon *b, const int8_t *matrix);
int scan_check_batch(const char *who, const mmgpu_ctx *c, const ScanBatchCommon *b, bool must_have_run);
int scan_fetch_lists(const char *who, mmgpu_ctx *c, ScanBatchCommon *b, void *hits, uint32_t hit_stride, void *counts, hipMemcpyKind kind);
int scan_kernel_ms(const char *who, mmgpu_ctx *c, ScanBatchCommon *b, float *ms);
// one query's row of the context's score scratch, if the scratch still holds this batch's (the two scans keep a serial and a
// scratch each on the context); kind: "scan" / "gapped scan"
int scan_debug_scores(const char *who, const char *kind, mmgpu_ctx *c, ScanBatchCommon *b, uint64_t mmgpu_ctx::*serial, DevBuf mmgpu_ctx::*scratch,
                      size_t score_size, uint32_t query, void *out, size_t cap);
void scan_sync_for_free(mmgpu_ctx *c);      // before a batch is deleted: nothing of it is in flight
}

// a k-mer matching batch (kmermatch_api.hip); rescore_api.hip reads its result for the hand-over
struct mmgpu_kmermatch_batch_t {
    mmgpu_kmermatch_params par{};             // (a nucleotide batch: k, the selection, the hash seed and the coverage rule; no alphabet)
    bool nucl = false;                        // a mmgpu_nuclmatch_batch_t
    mmgpu::DevBuf d_order;                    // nucl: ids by length, longest first
    uint32_t n = 0;                           // sequences
    uint64_t bound = 0;                       // records at most (computeKmerCount)
    const uint8_t *db_res = nullptr;          // the resident database the batch was prepared against (a reload invalidates the batch)
    bool ran = false;
    uint64_t n_records = 0, n_pairs = 0, n_kept = 0;
    mmgpu::DevBuf d_offsets, d_records;       // the result: uint64[n + 1], mmgpu_pf_hit[n + n_kept]
    hipEvent_t ev[mmgpu::KMM_STAGES + 1] = {};      // around the stages of the last run
    ~mmgpu_kmermatch_batch_t() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
// the nucleotide stage's batch (nuclmatch_api.hip) is the same record under a type of its own: the hand-over to the rescoring does not take it
struct mmgpu_nuclmatch_batch_t : mmgpu_kmermatch_batch_t {};
namespace mmgpu {
// kmermatch_api.hip: what the two stages' entry points share; `who` names the calling entry point in the messages
int kmm_check_batch(const char *who, const mmgpu_ctx *c, const mmgpu_kmermatch_batch_t *b, bool must_have_run);
int kmm_new_batch(const char *who, mmgpu_ctx *c, const mmgpu_kmermatch_params &par, bool nucl, uint64_t bound, mmgpu_kmermatch_batch_t *b);
int kmm_run_impl(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b);
int kmm_fetch(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, mmgpu_kmermatch_counts *counts, void *offsets, void *records, hipMemcpyKind kind);
int kmm_kernel_ms(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, float *ms);
}
#endif
