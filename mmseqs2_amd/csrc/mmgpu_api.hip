// Host side of libmmgpu: context, host helpers, batch scheduling, launches.  (What a context holds resident: db_api.hip.)
// Everything here is plumbing around the kernels in sw_kernel.hip; see include/mmgpu.h for the contract.
#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "mmgpu_internal.h"

#include <chrono>

using namespace mmgpu;

namespace mmgpu {
thread_local std::string g_last_error;
}
using mmgpu::g_last_error;

extern "C" const char *mmgpu_last_error(void) { return g_last_error.c_str(); }

extern "C" int mmgpu_init(mmgpu_ctx **out, int device_id) {
    if (!out) return fail(MMGPU_ERR_ARG, "mmgpu_init: ctx is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(MMGPU_ERR_ARG, "mmgpu_init: no such device");
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    mmgpu_ctx *c = new mmgpu_ctx();
    c->device = device_id;
    c->compute_units = prop.multiProcessorCount;
    c->name = prop.name;
    *out = c;
    return MMGPU_OK;
}

namespace mmgpu {
// the context's pinned staging arena (mmgpu_ctx::pinned) for the length of a call.  acquire() grows the arena to `need`
// bytes and returns it, or null - another thread's call holds it, or pinned memory cannot be had - and the caller copies from / to
// pageable memory instead.  The holder lets go when it dies: keep it until the stream has passed the last copy that uses the arena
struct PinnedLease {
    mmgpu_ctx *c = nullptr;
    PinnedLease() = default;
    PinnedLease(const PinnedLease &) = delete;
    PinnedLease &operator=(const PinnedLease &) = delete;
    ~PinnedLease() { if (c) c->pinned_busy.store(false, std::memory_order_release); }
    void *acquire(mmgpu_ctx *ctx, size_t need);
};

void *PinnedLease::acquire(mmgpu_ctx *ctx, size_t need) {
    if (c || ctx->pinned_busy.exchange(true, std::memory_order_acquire)) return nullptr;
    c = ctx;
    if (need > ctx->pinned_cap) {      // grown by a quarter more than asked for: the next batch is about as large
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        ctx->pinned_cap = 0;
        if (hipHostMalloc(&ctx->pinned, need + need / 4, hipHostMallocDefault) == hipSuccess) ctx->pinned_cap = need + need / 4;
        else (void)hipGetLastError();   // pageable copies then
    }
    return ctx->pinned_cap >= need ? ctx->pinned : nullptr;
}

}  // namespace mmgpu

extern "C" void mmgpu_destroy(mmgpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    mmgpu::db_release(c);
    (void)hipDeviceSynchronize();
    mmgpu::comm_free(c);
    if (c->owns_stream && c->stream) (void)hipStreamDestroy(c->stream);
    for (auto &st : c->side) if (st) (void)hipStreamDestroy(st);
    if (c->fork) (void)hipEventDestroy(c->fork);
    for (auto &e : c->join) if (e) (void)hipEventDestroy(e);
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->cache->trim();
    c->cache->closed = true;
    delete c;
}

extern "C" int mmgpu_set_stream(mmgpu_ctx *c, void *s) {
    if (!c) return fail(MMGPU_ERR_ARG, "ctx is NULL");
    c->stream = reinterpret_cast<hipStream_t>(s);
    return MMGPU_OK;
}

extern "C" int mmgpu_synchronize(mmgpu_ctx *c) {
    if (!c) return fail(MMGPU_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MMGPU_OK;
}

extern "C" int mmgpu_device_info(mmgpu_ctx *c, int *cus, char *name, int cap) {
    if (!c) return fail(MMGPU_ERR_ARG, "ctx is NULL");
    if (cus) *cus = c->compute_units;
    if (name && cap > 0) {
        strncpy(name, c->name.c_str(), (size_t)cap - 1);
        name[cap - 1] = 0;
    }
    return MMGPU_OK;
}

extern "C" int mmgpu_device_memory(mmgpu_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!c) return fail(MMGPU_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return MMGPU_OK;
}

// Loads the code objects of the hot kernels now instead of at their first launch (the runtime loads a translation unit's code
// object lazily: 0.1 - 0.2 s in total, paid inside the first prefilter block and the first alignment batch of a process).  A
// caller that has something else to do meanwhile - the fused search masks / reads its databases on the host - calls this on a
// helper thread right after mmgpu_init.
extern "C" int mmgpu_warmup(mmgpu_ctx *c) {
    if (!c) return fail(MMGPU_ERR_ARG, "mmgpu_warmup: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    mmgpu::warm_tantan();
    mmgpu::warm_ix();
    mmgpu::warm_pf();
    mmgpu::warm_sw();
    mmgpu::warm_block();
    mmgpu::warm_block4();
    mmgpu::warm_bt();
    mmgpu::warm_scan();
    mmgpu::warm_gscan();
    mmgpu::warm_rescore();
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// host-side helpers
// ---------------------------------------------------------------------------------------------------------
// SubstitutionMatrix::calcLocalAaBiasCorrection, src/commons/SubstitutionMatrix.cpp:79-112.  The reference mixes
// float and double (`deltaS_i /= -1.0 * (float)windowLength`, `deltaS_i += pBack[a] * (float)subMat[a]`); each
// statement below rounds where the reference's expression rounds.
extern "C" int mmgpu_host_comp_bias(const int16_t *submat, const double *pback, int alphabet, const uint8_t *seq,
                                    uint32_t len, float scale, float *out) {
    if (!submat || !pback || (!seq && len) || (!out && len)) return fail(MMGPU_ERR_ARG, "mmgpu_host_comp_bias: NULL argument");
    const int n = (int)len, half_window = 20;
    for (int i = 0; i < n; i++) {
        if (seq[i] >= alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_host_comp_bias: residue code >= alphabet");
        const int lo = std::max(0, i - half_window), hi = std::min(n, i + half_window);
        const int16_t *row = submat + (int)seq[i] * alphabet;
        int sum = 0;
        for (int j = lo; j < hi; j++) sum += row[seq[j]];
        sum -= row[seq[i]];
        float delta = (float)sum;
        delta = (float)((double)delta / (-1.0 * (double)(float)(hi - lo)));
        for (int a = 0; a < alphabet; a++) delta = (float)((double)delta + pback[a] * (double)(float)row[a]);
        out[i] = scale * delta;
    }
    return MMGPU_OK;
}

// The same correction for a whole block of queries (what Prefiltering::runSplit / Alignment::run compute per query inside
// their OpenMP loops, QueryMatcher.cpp:108-116, Matcher::initQuery -> ssw_init StripedSmithWaterman.cpp:1371-1381): sequences
// are dealt to n_threads host threads.  out_float (may be NULL) receives the float bias, out_round (may be NULL) ssw_init's int8
// rounding of it; both are indexed like `residues`.
extern "C" int mmgpu_host_comp_bias_batch(const int16_t *submat, const double *pback, int alphabet, const uint8_t *residues,
                                          const uint64_t *offsets, uint32_t n, float scale, float *out_float, int8_t *out_round,
                                          int n_threads) {
    if (!submat || !pback || !offsets || (!residues && n && offsets[n])) return fail(MMGPU_ERR_ARG, "mmgpu_host_comp_bias_batch: NULL argument");
    if (n_threads < 1) n_threads = 1;
    n_threads = (int)std::min<uint32_t>((uint32_t)n_threads, std::max<uint32_t>(n, 1u));
    std::atomic<uint32_t> next(0);
    std::atomic<int> bad(0);
    auto work = [&]() {
        std::vector<float> tmp;
        for (;;) {
            const uint32_t b = next.fetch_add(64);
            if (b >= n) return;
            for (uint32_t i = b; i < std::min(n, b + 64); i++) {
                const uint64_t o = offsets[i];
                const uint32_t len = (uint32_t)(offsets[i + 1] - o);
                float *dst = out_float ? out_float + o : (tmp.resize(len), tmp.data());
                if (mmgpu_host_comp_bias(submat, pback, alphabet, residues + o, len, scale, dst) != MMGPU_OK) { bad = 1; return; }
                if (out_round) mmgpu_host_round_comp_bias(dst, len, out_round + o);
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    return bad ? fail(MMGPU_ERR_ARG, "mmgpu_host_comp_bias_batch: residue code >= alphabet") : MMGPU_OK;
}

// Length-bucket sharding of a target database over n_shards devices (the reference balances
// residues over its splits, DBReader::decomposeDomainByAminoAcid, src/commons/DBReader.cpp:1108-1150, and libmarv deals
// length partitions to devices).  Targets are binned by length (boundaries below), the bins are walked from the longest
// to the shortest and their members dealt round-robin, the deal continuing from bin to bin: every shard receives the same
// length distribution (+-1 sequence per bin) and therefore the same number of residues, index entries and alignment
// cells to within a fraction of a percent.  Inside a shard the local ids follow the global ids (ascending), so that
// "same score -> smaller id first" orders of the shard and of the whole database agree.
extern "C" int mmgpu_host_partition_targets(const uint64_t *offsets, uint32_t n, uint32_t n_shards, uint32_t *shard_of,
                                            uint32_t *local_id, uint32_t *shard_sizes, uint64_t *shard_residues) {
    if (!offsets || !shard_of || !local_id || !shard_sizes || n_shards == 0) return fail(MMGPU_ERR_ARG, "mmgpu_host_partition_targets: bad argument");
    static const uint32_t bound[] = {32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 768, 896, 1024,
                                     1280, 1536, 2048, 2560, 3072, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536};
    const int nb = (int)(sizeof(bound) / sizeof(bound[0]));
    std::vector<uint8_t> bin(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        int b = 0;
        while (b < nb - 1 && len > bound[b]) b++;
        bin[i] = (uint8_t)b;
    }
    uint32_t next = 0;
    for (int b = nb - 1; b >= 0; b--)
        for (uint32_t i = 0; i < n; i++)
            if (bin[i] == b) {
                shard_of[i] = next;
                next = next + 1 == n_shards ? 0 : next + 1;
            }
    for (uint32_t s = 0; s < n_shards; s++) {
        shard_sizes[s] = 0;
        if (shard_residues) shard_residues[s] = 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        local_id[i] = shard_sizes[shard_of[i]]++;
        if (shard_residues) shard_residues[shard_of[i]] += offsets[i + 1] - offsets[i];
    }
    return MMGPU_OK;
}

extern "C" int mmgpu_host_round_comp_bias(const float *bias, uint32_t len, int8_t *out) {
    if ((!bias || !out) && len) return fail(MMGPU_ERR_ARG, "mmgpu_host_round_comp_bias: NULL argument");
    for (uint32_t i = 0; i < len; i++) out[i] = (int8_t)((bias[i] < 0.0f) ? bias[i] - 0.5 : bias[i] + 0.5);
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Smith-Waterman batches
// ---------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t JOB_HITS = 256;   // most hits per workgroup (8 rounds of 32); the reverse pass packs a job with one thread per hit (sw_kernel.hip)
static_assert(JOB_HITS <= 256, "a job may hold at most one hit per thread of the 256-thread workgroup");
constexpr uint32_t JOB_ROUND = 32;   // targets a workgroup has in flight
constexpr uint64_t JOB_CELLS = 60000000ull;   // cut a job once it holds this many forward cells
constexpr uint32_t LONG_QUERY = 1024;  // multi-tile queries from this length on are scheduled per wave (8 targets)
}  // namespace

struct mmgpu_sw_batch_t {
    int mode = 0;
    int alphabet = 0, gap_open = 0, gap_extend = 0;
    uint64_t cells = 0, pairs = 0;
    uint64_t valid_pairs = 0;   // from_pf: slots actually holding a hit (pairs counts all slots)
    uint32_t n_queries = 0;
    // all jobs of the batch, by kernel group (sw_kernel.hip), longest first inside a group; SwJob::shape picks the body
    uint32_t n_jobs = 0, n_multi_jobs = 0;
    uint32_t n_rev_jobs = 0;      // reverse-scan jobs of the multi-tile queries (mode START), behind the forward jobs in d_jobs
    uint32_t group_begin[SW_GROUPS + 1] = {};
    size_t group_lds[SW_GROUPS] = {};   // most profile bytes any job of the group holds: one tile, or all tiles of a resident multi-tile job
    DevBuf d_jobs;
    DevBuf d_scratch;             // multi-tile jobs: [scratch slot][4 waves][4 groups][2 buffers][scratch_cols] x uint2
    DevBuf d_scratch_busy;        // one flag per slot of the pool (sw_kernel claims / releases)
    uint32_t scratch_slots = 0;
    DevBuf d_pf_counts, d_slot_target;   // from_pf: list lengths and slot -> target id, copied out of the prefilter batch
    DevBuf d_qout_off, d_out_target;     // mmgpu_sw_block_starts: h_qout_off / h_out_target on the device (uploaded on first use)
    DevBuf d_qres, d_qcb, d_qoff, d_qbias, d_qminstart, d_hit_target, d_hit_out, d_out, d_mat;
    DevBuf d_qprof, d_qprof_off;   // profile queries only (empty otherwise)
    bool any_profile = false;
    // fused hand-over from a prefilter batch (mmgpu_sw_prepare_from_pf): lists, counts and statistics live on the device
    bool from_pf = false;
    uint32_t pf_stride = 0, slot_stride = 0;
    DevBuf d_stats;                        // [2] unsigned long long: cells, pairs
    std::vector<uint32_t> h_out_target;   // target id of every result slot (kept for mmgpu_sw_traceback, mode >= START)
    std::vector<uint32_t> h_qout_off;     // [nq + 1] first result slot of every query
    std::vector<uint32_t> h_qoff;         // [nq + 1] residue offsets
    std::vector<uint8_t> h_query_is_profile;   // profile queries of the batch (empty: none)
    DevBuf d_bt_scratch, d_bt_jobs, d_bt_info, d_bt_str, d_bt_cursor;
    uint32_t scratch_cols = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // one pair per mmgpu_sw_run since prepare
    bool ran = false;
    // mmgpu_sw_traceback's host copies of the last run's results
    std::vector<mmgpu_sw_hit> h_res;
    std::vector<uint32_t> h_slot_target;
    bool h_res_valid = false;
    uint32_t block_pairs_tier[3] = {0, 0, 0};   // last mmgpu_sw_block_backtrace call: pairs decided with blocks <= 512 / 2048 / 4096 rows
    uint32_t block_pairs_fast = 0;              // ... by block4_kernel.hip's first launch (four pairs per wavefront, blocks <= 256 rows)
    uint32_t block_pairs_skew = 0;              // ... and by its skewed launches (one pair per wavefront, blocks <= 1024 / 4096 rows)
    // pairs this rank owns of a sharded run's merged lists (mmgpu_sw_prepare_owned / mmgpu_sw_gather_owned)
    bool owned = false;
    uint32_t o_stride = 0, o_cap = 0;
    int o_ranks = 0;
    bool o_dense = false;          // a rank's send buffer overflowed once: every rank's buffer holds all slots from now on
    DevBuf o_lhits, o_lcounts, o_lslot;        // merged lists restricted to this shard's targets (local ids) + their list positions
    DevBuf o_send, o_counter, o_recv, o_recv_counters, o_full, o_status;
    // mmgpu_sw_prepare_masked: the batch's own targets - one masked copy per pair in DeviceDb's layout, id = pair ordinal
    // (hit_target, h_out_target and the jobs of the later calls name these ids)
    bool masked = false;
    DevBuf m_res, m_off4, m_len;
    std::vector<uint32_t> m_h_len;
    uint32_t m_max_len = 0;
    // sw_prepare_dense: lists and records live in arrays of the caller (the chunks of an exhaustive gapped scan share one set);
    // d_hit_target / d_hit_out / d_out stay empty
    uint32_t *x_hit_target = nullptr, *x_hit_out = nullptr;
    mmgpu_sw_hit *x_out = nullptr;
};

// the targets a batch's kernels read: the resident database, or the batch's masked copies
static TargetView sw_targets(const mmgpu_ctx *c, const mmgpu_sw_batch_t *b) {
    TargetView v;
    if (b && b->masked) {
        v.res = b->m_res.as<uint8_t>();
        v.off4 = b->m_off4.as<uint32_t>();
        v.len = b->m_len.as<uint32_t>();
        v.n = (uint32_t)b->m_h_len.size();
        v.max_len = b->m_max_len;
        v.h_len = b->m_h_len.data();
    } else {
        v.res = c->db.res;
        v.off4 = c->db.off4;
        v.len = c->db.len;
        v.n = c->db.n;
        v.max_len = c->db.max_len;
        v.h_len = c->h_len.data();
    }
    return v;
}

// which kernel body serves a query of this length: 16 lanes x R rows per tile (any R since round 5: the padding of a tile is
// below 16 rows, it was below 32 with even R only), at most 16 * SW_MAX_R rows per tile; longer queries are cut into equal tiles
// (multi-tile bodies).  wide: a query of up to 32 * SW_MAX_R rows is one tile of a 32-lane group (R = ceil(qlen / 32)) instead of two
// tiles - a single-tile job in every respect: no scratch slot, no reverse job, rounds of 16 hits (four per wavefront).
static void pick_class(uint32_t qlen, int *rows_per_lane, bool *multi, bool *wide) {
    constexpr uint32_t max_rows = 16u * (uint32_t)SW_MAX_R;
    *wide = mmgpu::sw_wide_enabled() && qlen > max_rows && qlen <= 2 * max_rows;
    if (*wide) {
        *rows_per_lane = (int)((qlen + 31) / 32);
        *multi = false;
        return;
    }
    const uint32_t n_tiles = (qlen + max_rows - 1) / max_rows;
    const uint32_t rows = (qlen + n_tiles - 1) / n_tiles;       // rows per tile before rounding
    *rows_per_lane = (int)std::max<uint32_t>(1u, (rows + 15) / 16);
    *multi = n_tiles > 1;
}

// Slots of a job that should hold about `rounds` rounds of `round` hits: whole workgroup rounds (4 waves x 8), so
// that no wave idles while its neighbours run a second round; only jobs below one workgroup round (long queries cut
// per wave) may hold 8 or 16.
static uint32_t job_slots(uint32_t round, uint64_t rounds) {
    const uint64_t slots = std::max<uint64_t>(1, rounds) * round;
    if (slots >= JOB_ROUND) return (uint32_t)std::min<uint64_t>(JOB_HITS, slots / JOB_ROUND * JOB_ROUND);
    return slots >= 16 ? 16u : round;
}

// device-resident hit lists an alignment batch is built from (the fused hand-over and the multi-GPU path)
struct DeviceLists {
    const mmgpu_pf_hit *hits = nullptr;
    const uint32_t *counts = nullptr;
    uint32_t stride = 0;
};

namespace {

// a batch under preparation: freed (with its buffers) unless the preparation hands it to the caller
struct SwBatchFree {
    mmgpu_ctx *c;
    void operator()(mmgpu_sw_batch_t *b) const { mmgpu_sw_free(c, b); }
};

double prep_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One call of sw_prepare_impl: its arguments, the batch, and the host arrays its steps hand to one another.  The steps run in the
// order they are declared in.  Two of them depend on where the lists are: a list on the device (`pf`: the fused hand-over, the
// lists of mmgpu_sw_prepare_from_lists, the owned pairs of a sharded run) gets fixed jobs over its slots while the queries are
// copied and is ordered by sw_from_pf_kernel at the end (order_device_lists); a list of the caller is sorted and cut on the host
// (cut_list_jobs, join_list_jobs) and uploaded as it stands.
struct SwPrepare {
    mmgpu_ctx *c;
    const mmgpu_sw_params *par;
    const mmgpu_sw_query *qs;
    uint32_t nq;
    int mode;
    const DeviceLists *pf;        // null: the lists are the caller's (mmgpu_sw_query::target_ids)
    const mmgpu_sw_masks *masks;  // mmgpu_sw_prepare_masked: the batch aligns against masked copies of its targets (caller's lists only)
    const SwDenseLists *dense;    // sw_prepare_dense: the lists are slices of the length-ordered id list, written on the device by the caller
    mmgpu_sw_batch_t *b = nullptr;
    TargetView tv;                // the targets the lists name: the resident database, or the batch's copies once plan_masked has run

    std::vector<uint8_t> qres;
    std::vector<int8_t> qcb, mat;
    std::vector<uint32_t> qoff;
    std::vector<int32_t> qbias, qminstart;
    std::vector<int8_t> qprof;                       // profile queries: [alphabet][qlen] blocks, concatenated
    std::vector<uint32_t> qprof_off;
    std::vector<uint32_t> hit_target, hit_out;       // caller's lists only
    std::vector<SwJob> jobs;
    std::vector<SwJob> rev_jobs;          // multi-tile queries, mode START: the reverse scan runs per query (sw_rev_multi_kernel)
    std::vector<uint64_t> rev_cells, job_cells;
    std::vector<SwJob> sorted;            // the jobs as uploaded (asynchronously: lives until the stream is drained)
    struct Deferred { uint32_t query, hit_cursor, out_cursor, shape, round; bool multi; };   // caller-supplied lists, scheduled by cut_list_jobs
    std::vector<Deferred> deferred;
    struct PerQuery { std::vector<SwJob> jobs; std::vector<uint64_t> cells; uint64_t sum_cells = 0; uint32_t max_tlen = 0; uint32_t rev_mid_len = 0; bool bad = false; };
    std::vector<PerQuery> per_query;      // [deferred.size()]
    uint64_t total_hits = 0;
    uint32_t pf_stride = 0, n_multi = 0, max_tlen = 0;
    uint32_t hit_cursor = 0, out_cursor = 0;
    int minp = 0;
    bool any_multi = false;
    PinnedLease pinned;                   // the context's staging arena, from enqueue_uploads until the call ends (stream drained)
    // masked batch: the lists over the copies (ids = pair ordinals) that take the caller's place, and what the gather kernel reads
    std::vector<mmgpu_sw_query> m_queries;
    std::vector<uint32_t> m_ids, m_src, m_off4;
    uint64_t m_bytes = 0;
    double mark = prep_now();

    void lap(const char *what);
    int check_params();
    void new_batch();
    int size_buffers();
    int plan_masked();
    int gather_masked();
    int copy_query(uint32_t i, int *qminp);
    void add_slot_jobs(uint32_t i, uint32_t shape, uint32_t round, bool multi);
    void add_rev_jobs(uint32_t query, uint32_t first, uint32_t n, uint32_t shape, uint64_t cells_per_hit);
    int copy_queries();
    void cut_list_jobs_of(size_t from, size_t to);
    void cut_list_jobs();
    void cut_dense_jobs();
    int join_list_jobs();
    void order_jobs();
    int enqueue_uploads();
    hipError_t alloc_scratch(uint32_t longest);
    int finish_host_lists();
    int order_device_lists();
};

// where the host side of a batch's preparation goes
void SwPrepare::lap(const char *what) {
    static const bool prep_trace = getenv("MMGPU_TRACE") != nullptr;
    if (!prep_trace) return;
    const double t = prep_now();
    fprintf(stderr, "[mmgpu sw_prepare] %s %.3f s\n", what, t - mark);
    mark = t;
}

int SwPrepare::check_params() {
    if (pf) {
        pf_stride = pf->stride;
        if (pf_stride > (uint32_t)SW_PF_MAX_LIST) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare_from_pf: lists longer than 16384");
    }
    if (!c->db.res) return fail(MMGPU_ERR_STATE, "mmgpu_sw_prepare: no targets loaded");
    if (par->alphabet != c->db.alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: alphabet differs from the loaded targets");
    if (mode != MMGPU_SW_SCORE_END && mode != MMGPU_SW_START && mode != MMGPU_SW_START_NOT_WORD) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare: unknown mode");
    if (par->gap_extend < 0 || par->gap_open < 0 || par->gap_open > 32767)
        return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: need 0 <= gap_extend and 0 <= gap_open <= 32767");
    // The acceptance rule (include/mmgpu.h mmgpu_sw_params, oracle/sw_oracle.c): the cell-by-cell recurrence equals the
    // reference's striped lazy-F result only if  gap_open > gap_extend >= 0  and  min(P) + min(comp_bias) + gap_extend > -gap_open.
    // The reference itself runs outside it (with other numbers), so such a batch is UNSUPPORTED, not a bad argument: the host
    // falls back to its own aligner.  The second half is checked per query in copy_query.
    if (par->gap_open <= par->gap_extend)
        return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare: gap_open <= gap_extend (the reference's int16 pass is not the plain recurrence there)");
    for (int i = 0; i < par->alphabet * par->alphabet; i++) minp = std::min<int>(minp, par->mat[i]);
    return MMGPU_OK;
}

void SwPrepare::new_batch() {
    b->mode = mode;
    b->alphabet = par->alphabet;
    b->gap_open = par->gap_open;
    b->gap_extend = par->gap_extend;
    b->n_queries = nq;
    for (DevBuf *d : {&b->d_qres, &b->d_qcb, &b->d_qoff, &b->d_qbias, &b->d_qminstart, &b->d_hit_target, &b->d_hit_out, &b->d_out,
                      &b->d_mat, &b->d_stats, &b->d_bt_scratch, &b->d_bt_jobs, &b->d_bt_info, &b->d_bt_str, &b->d_bt_cursor, &b->d_scratch_busy,
                      &b->d_pf_counts, &b->d_slot_target, &b->d_qprof, &b->d_qprof_off, &b->d_qout_off, &b->d_out_target, &b->d_jobs, &b->d_scratch})
        d->bind(c->cache);
}

int SwPrepare::size_buffers() {
    qoff.assign(nq + 1, 0);
    qbias.assign(std::max<uint32_t>(nq, 1), 0);
    qminstart.assign(std::max<uint32_t>(nq, 1), 0);
    qprof_off.assign(std::max<uint32_t>(nq, 1), 0xFFFFFFFFu);
    for (uint32_t i = 0; i < nq; i++) {
        // a query without targets may come without residues (Alignment::run never maps the query of an empty list, :322)
        const bool empty_ok = !pf && !dense && qs[i].n_targets == 0 && qs[i].qlen == 0;
        if (!empty_ok && (qs[i].qlen == 0 || qs[i].qlen > 65535 || !qs[i].q)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: bad query");
        qoff[i + 1] = qoff[i] + qs[i].qlen;
        total_hits += pf ? pf_stride : dense ? dense->count[i] : qs[i].n_targets;
    }
    if (total_hits > 0xFFFFFFF0ull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare: more than 2^32 pairs in one batch");
    qres.resize(qoff[nq]);
    qcb.assign(qoff[nq], 0);
    if (!pf && !dense) {
        hit_target.resize((size_t)total_hits);
        hit_out.resize((size_t)total_hits);
    }
    b->h_qout_off.assign(nq + 1, 0);
    if (mode >= MMGPU_SW_START && !pf) b->h_out_target.resize((size_t)total_hits);
    return MMGPU_OK;
}

// A masked batch's targets: pair p of the lists (query-major, list order) gets copy p of an arena laid out like the resident database
// (mmgpu_load_targets), and the lists are rewritten to name the copies.  Everything after this step schedules over `tv`, the view of
// the copies; the copies themselves are made at the end of the preparation (gather_masked).
int SwPrepare::plan_masked() {
    if (!masks->span_off) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: NULL span_off");
    if (masks->mask_letter < 0 || masks->mask_letter >= par->alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: mask letter outside the alphabet");
    const size_t P = (size_t)total_hits;
    m_ids.resize(P);
    m_src.resize(P);
    m_off4.resize(std::max<size_t>(P, 1));
    b->m_h_len.resize(P);
    m_queries.assign(qs, qs + nq);
    uint64_t cur4 = 16;      // the layout of mmgpu_load_targets: 64 B in front, 4-byte boundaries, max_len + 64 B behind
    uint32_t max_len = 0;
    size_t p = 0;
    for (uint32_t i = 0; i < nq; i++) {
        m_queries[i].target_ids = m_ids.data() + p;
        for (uint32_t k = 0; k < qs[i].n_targets; k++, p++) {
            const uint32_t t = qs[i].target_ids[k];
            if (t >= c->db.n) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: target id out of range");
            const uint32_t l = c->h_len[t];
            if (masks->span_off[p + 1] < masks->span_off[p]) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: span_off not monotone");
            if (!masks->spans && masks->span_off[p + 1] != masks->span_off[p]) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: NULL spans");
            for (uint32_t z = masks->span_off[p]; z < masks->span_off[p + 1]; z++)
                if (masks->spans[z].t_from > masks->spans[z].t_to || masks->spans[z].t_to > l)
                    return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: span outside its target (need t_from <= t_to <= length)");
            if (cur4 > 0xFFFFFFFFull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare_masked: more than 16 GiB of masked copies in one batch");
            m_ids[p] = (uint32_t)p;
            m_src[p] = t;
            m_off4[p] = (uint32_t)cur4;
            b->m_h_len[p] = l;
            max_len = std::max(max_len, l);
            cur4 += (l + 3) / 4;
        }
    }
    m_bytes = cur4 * 4 + max_len + 64;
    b->m_max_len = max_len;
    b->masked = true;
    qs = m_queries.data();
    tv = sw_targets(c, b);      // (host side only until gather_masked has allocated the copies)
    return MMGPU_OK;
}

// ... and the copies: pad letters everywhere (one memset), then sw_mask_gather_kernel, on the context's stream behind the uploads
int SwPrepare::gather_masked() {
    hipStream_t s = c->stream;
    const size_t P = m_src.size();
    DevBuf d_src, d_span_off, d_spans;
    for (DevBuf *d : {&d_src, &d_span_off, &d_spans, &b->m_res, &b->m_off4, &b->m_len}) d->bind(c->cache);
    const uint32_t s_first = masks->span_off[0], n_spans = masks->span_off[P] - s_first;
    struct Event {      // MMGPU_TRACE: the memset + kernel between two events
        hipEvent_t e = nullptr;
        ~Event() { if (e) (void)hipEventDestroy(e); }
    } t0, t1;
    const bool timed = getenv("MMGPU_TRACE") && hipEventCreate(&t0.e) == hipSuccess && hipEventCreate(&t1.e) == hipSuccess;
    auto enqueue = [&]() -> int {
        HIP_TRY(b->m_res.alloc((size_t)m_bytes));
        HIP_TRY(upload(b->m_off4, m_off4, s));
        HIP_TRY(upload(b->m_len, b->m_h_len, s));
        HIP_TRY(upload(d_src, m_src, s));
        HIP_TRY(d_span_off.alloc((P + 1) * 4));
        HIP_TRY(hipMemcpyAsync(d_span_off.p, masks->span_off, (P + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(d_spans.alloc(std::max<size_t>(n_spans, 1) * sizeof(mmgpu_sw_span)));
        if (n_spans) HIP_TRY(hipMemcpyAsync(d_spans.p, masks->spans + s_first, (size_t)n_spans * sizeof(mmgpu_sw_span), hipMemcpyHostToDevice, s));
        if (timed) HIP_TRY(hipEventRecord(t0.e, s));
        HIP_TRY(hipMemsetAsync(b->m_res.p, par->alphabet, (size_t)m_bytes, s));
        SwMaskGatherArgs A;
        A.src_res = c->db.res;
        A.src_off4 = c->db.off4;
        A.src_len = c->db.len;
        A.src_id = d_src.as<uint32_t>();
        A.dst_res = b->m_res.as<uint8_t>();
        A.dst_off4 = b->m_off4.as<uint32_t>();
        A.span_off = d_span_off.as<uint32_t>();
        A.spans = d_spans.as<mmgpu_sw_span>();
        A.span_base = s_first;      // (span_off counts from the caller's first span; only the spans from there on were uploaded)
        A.mask_letter = (uint32_t)masks->mask_letter;
        A.n_pairs = (uint32_t)P;
        HIP_TRY(launch_sw_mask_gather(A, s));
        if (timed) HIP_TRY(hipEventRecord(t1.e, s));
        return MMGPU_OK;
    };
    const int e = enqueue();
    // the span buffers of this step die with it; after a failure (out of memory for the copies) the batch and its buffers go as well
    const hipError_t drained = hipStreamSynchronize(s);
    if (e) return e;
    HIP_TRY(drained);
    float ms = 0;
    if (timed && hipEventElapsedTime(&ms, t0.e, t1.e) == hipSuccess)
        fprintf(stderr, "[mmgpu sw_prepare] masked copies: %zu pairs, %u spans, arena %llu bytes, memset + sw_mask_gather_kernel %.3f ms\n", P, n_spans,
                (unsigned long long)m_bytes, ms);
    tv = sw_targets(c, b);
    return MMGPU_OK;
}

// residues, composition bias / profile rows, bias and start-score threshold of query i; *qminp = its lowest substitution score
int SwPrepare::copy_query(uint32_t i, int *qminp) {
    const mmgpu_sw_query &Q = qs[i];
    memcpy(qres.data() + qoff[i], Q.q, Q.qlen);
    int mincb = 0;
    *qminp = minp;
    for (uint32_t k = 0; k < Q.qlen; k++) {
        if (Q.q[k] >= par->alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: query residue code >= alphabet");
        if (Q.comp_bias && !Q.profile) { qcb[qoff[i] + k] = Q.comp_bias[k]; mincb = std::min<int>(mincb, Q.comp_bias[k]); }
    }
    if (Q.profile) {
        // ssw_init with a profile query (StripedSmithWaterman.cpp:1386-1406): the first PROFILE_AA_SIZE letter rows are the
        // profile, the X row scores 0, no composition bias; bias = |min| over the profile rows
        if (Q.profile_letters == 0 || (int)Q.profile_letters > par->alphabet)
            return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: profile_letters must be in [1, alphabet]");
        if (qprof.size() + (size_t)par->alphabet * Q.qlen > 0xFFFFFFF0ull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare: more than 4 GB of query profiles in one batch");
        qprof_off[i] = (uint32_t)qprof.size();
        qprof.resize(qprof.size() + (size_t)par->alphabet * Q.qlen, 0);
        const uint32_t rows = std::min<uint32_t>(Q.profile_letters, (uint32_t)par->alphabet - 1);   // :1389-1390 zeroes the last letter (X)
        memcpy(qprof.data() + qprof_off[i], Q.profile, (size_t)rows * Q.qlen);
        *qminp = 0;
        for (size_t k = 0; k < (size_t)Q.profile_letters * Q.qlen; k++) *qminp = std::min<int>(*qminp, Q.profile[k]);
        b->any_profile = true;
        b->h_query_is_profile.resize(nq, 0);
        b->h_query_is_profile[i] = 1;
    }
    if (!(*qminp + mincb + par->gap_extend > -par->gap_open))
        return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_prepare: gap penalties too small for this matrix (adjacent insertion+deletion could win)");
    qbias[i] = std::abs(*qminp) + std::abs(mincb);   // ssw_init :1397-1406
    qminstart[i] = Q.min_start_score;
    return MMGPU_OK;
}

// Reverse-scan jobs of a multi-tile query: consecutive slots of its list, as many as hold about six forward jobs'
// worth of cells (one pair in six reaches the start-score threshold on hit lists), whole workgroup rounds, at most
// SW_REV_JOB_MAX; the kernel packs the live pairs of a job before it deals them to its waves.
void SwPrepare::add_rev_jobs(uint32_t query, uint32_t first, uint32_t n, uint32_t shape, uint64_t cells_per_hit) {
    uint64_t per = 6 * JOB_CELLS / std::max<uint64_t>(cells_per_hit, 1);
    per = std::min<uint64_t>(std::max<uint64_t>(per / JOB_ROUND * JOB_ROUND, JOB_ROUND), (uint64_t)SW_REV_JOB_MAX);
    for (uint32_t k = 0; k < n; k += (uint32_t)per) {
        SwJob j;
        j.query = query;
        j.hit_begin = first + k;
        j.hit_end = first + std::min<uint32_t>(k + (uint32_t)per, n);
        j.shape = shape;
        rev_jobs.push_back(j);
        rev_cells.push_back(cells_per_hit * (j.hit_end - j.hit_begin) * 65536u + (n - k));
    }
}

// a list on the device: fixed jobs over the query's slots, the kernel clips them to the list length (SwLaunch::q_hit_count); order
// and statistics come from sw_from_pf_kernel.  Hits per job: as many rounds as fit JOB_CELLS at the length the hits will probably
// have (prefilter hits are mostly about as long as the query; the database mean otherwise)
// (c->mean_len is the resident database's mean on purpose: only device lists come here, and a masked batch has none - its lists are
// the caller's, cut over the copies' own lengths in cut_list_jobs_of)
void SwPrepare::add_slot_jobs(uint32_t i, uint32_t shape, uint32_t round, bool multi) {
    const mmgpu_sw_query &Q = qs[i];
    const uint64_t est_cells = (uint64_t)Q.qlen * ((Q.qlen + c->mean_len) / 2 + 1) * round;
    const uint32_t per_job = job_slots(round, JOB_CELLS / est_cells);
    for (uint32_t k = 0; k < pf_stride; k += per_job) {
        SwJob j;
        j.query = i;
        j.hit_begin = hit_cursor + k;
        j.hit_end = hit_cursor + std::min<uint32_t>(k + per_job, pf_stride);
        j.shape = shape | (multi ? n_multi++ << 8 : 0u);
        jobs.push_back(j);
        // stand-in for the cell count the host cannot see: query length x slots; the lists are sorted by
        // target length on the device, so among equals a query's earlier jobs hold the longer targets
        job_cells.push_back((uint64_t)Q.qlen * (j.hit_end - j.hit_begin) * 65536u + (pf_stride - k));
    }
    if (multi && mode >= MMGPU_SW_START)
        add_rev_jobs(i, hit_cursor, pf_stride, shape, (uint64_t)Q.qlen * ((Q.qlen + c->mean_len) / 2 + 1));
    max_tlen = tv.max_len;
}

int SwPrepare::copy_queries() {
    for (uint32_t i = 0; i < nq; i++) {
        const mmgpu_sw_query &Q = qs[i];
        if (Q.qlen == 0) {      // empty list, no residues: no jobs, no result slots
            b->h_qout_off[i + 1] = out_cursor;
            continue;
        }
        int qminp;
        if (int e = copy_query(i, &qminp)) return e;
        int rpl; bool multi, wide;
        pick_class(Q.qlen, &rpl, &multi, &wide);
        any_multi |= multi;
        // [0,32): single tile R = 1..32, [32,64): multi-tile, [64,96): single tile on 32-lane groups
        const uint32_t shape = (multi ? SW_SHAPE_MULTI : wide ? SW_SHAPE_WIDE : 0u) + (uint32_t)rpl - 1;
        const int grp = sw_shape_group(shape);
        // a multi-tile job that fits keeps the profiles of all its tiles (sw_multi_resident: the kernel asks the same question)
        const uint32_t held = multi && sw_multi_resident(sw_tiles(Q.qlen, rpl), rpl, par->alphabet, SW_RESIDENT_LDS) ? sw_tiles(Q.qlen, rpl) : 1u;
        b->group_lds[grp] = std::max(b->group_lds[grp], (size_t)held * sw_profile_bytes(rpl, par->alphabet, wide ? 32 : 16));
        // jobs are cut at multiples of one workgroup round (4 waves x 8 targets); for queries of several tiles a
        // single wave's 8 targets already run for milliseconds, so those are cut per wave to shorten the tail
        // (a wide job's workgroup round is 4 waves x 4 targets)
        const uint32_t round = (multi && Q.qlen >= LONG_QUERY) ? JOB_ROUND / 4 : wide ? JOB_ROUND / 2 : JOB_ROUND;
        const uint32_t n_slots = pf ? pf_stride : dense ? dense->count[i] : Q.n_targets;
        if (pf) add_slot_jobs(i, shape, round, multi);
        // caller-supplied list: the sort by target length and the job cuts are done for all queries in parallel (cut_list_jobs)
        else deferred.push_back(Deferred{i, hit_cursor, out_cursor, shape, round, multi});
        hit_cursor += n_slots;
        out_cursor += n_slots;
        b->h_qout_off[i + 1] = out_cursor;
    }
    return MMGPU_OK;
}

// the caller's lists of deferred[from, to): sorted by target length (longest first) so the 8 targets a wave runs together end
// together, and cut into jobs
void SwPrepare::cut_list_jobs_of(size_t from, size_t to) {
    std::vector<uint32_t> ord;
    for (size_t d = from; d < to; d++) {
        const Deferred &D = deferred[d];
        const mmgpu_sw_query &Q = qs[D.query];
        PerQuery &P = per_query[d];
        const bool same_list = d > from && Q.target_ids == qs[deferred[d - 1].query].target_ids && Q.n_targets == qs[deferred[d - 1].query].n_targets;
        if (!same_list) {   // all-vs-all callers hand the same list to every query: sort it once (per thread)
            ord.resize(Q.n_targets);
            std::iota(ord.begin(), ord.end(), 0u);
            for (uint32_t k = 0; k < Q.n_targets; k++)
                if (Q.target_ids[k] >= tv.n) { P.bad = true; break; }
            if (P.bad) continue;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t bb) {
                return tv.h_len[Q.target_ids[a]] > tv.h_len[Q.target_ids[bb]];
            });
        }
        for (uint32_t k = 0; k < Q.n_targets; k++) {
            const uint32_t t = Q.target_ids[ord[k]];
            hit_target[D.hit_cursor + k] = t;
            hit_out[D.hit_cursor + k] = D.out_cursor + ord[k];
            P.sum_cells += (uint64_t)Q.qlen * tv.h_len[t];
            P.max_tlen = std::max(P.max_tlen, tv.h_len[t]);
        }
        // Jobs: consecutive hits of the (length-sorted) list, cut at multiples of one workgroup round (32 targets)
        // once a job holds JOB_CELLS forward cells, at the latest after JOB_HITS hits - a 5000-residue query against
        // 300 long targets must not become one 7e9-cell workgroup.
        for (uint32_t k = 0; k < Q.n_targets;) {
            uint64_t jc = 0;
            uint32_t e = k;
            while (e < Q.n_targets && e - k < JOB_HITS) {
                const uint32_t stop = std::min<uint32_t>(e + D.round, Q.n_targets);
                for (; e < stop; e++) jc += (uint64_t)Q.qlen * tv.h_len[hit_target[D.hit_cursor + e]];
                // cut at 8, 16 (long queries) or whole workgroup rounds: no wave idles while another runs a second round
                const uint32_t held = e - k;
                if (jc >= JOB_CELLS && (held <= 16 || held % JOB_ROUND == 0)) break;
            }
            SwJob j;
            j.query = D.query;
            j.hit_begin = D.hit_cursor + k;
            j.hit_end = D.hit_cursor + e;
            j.shape = D.shape;      // (multi-tile jobs get their scratch slot number when the lists are joined)
            P.jobs.push_back(j);
            P.cells.push_back(jc);
            k = e;
        }
        if (Q.n_targets) P.rev_mid_len = tv.h_len[hit_target[D.hit_cursor + Q.n_targets / 2]];
        if (mode >= MMGPU_SW_START)
            for (uint32_t k = 0; k < Q.n_targets; k++) b->h_out_target[D.out_cursor + k] = Q.target_ids[k];
    }
}

// 3 M pairs of a 10 000-query block cost 0.2 s on one thread (the sort's comparisons read the length table at random) - the queries
// are independent, so threads take contiguous ranges of them; the jobs are concatenated in query order afterwards
// (join_list_jobs), so the result does not depend on the number of threads.
void SwPrepare::cut_list_jobs() {
    per_query.resize(deferred.size());
    static const unsigned host_threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const size_t n_thr = std::max<size_t>(1, std::min<size_t>(host_threads, total_hits / 65536 + 1));
    if (n_thr <= 1) {
        cut_list_jobs_of(0, deferred.size());
        return;
    }
    // ranges of about equal numbers of pairs
    std::vector<std::thread> pool;
    size_t from = 0;
    uint64_t acc = 0;
    const uint64_t share = total_hits / n_thr + 1;
    for (size_t d = 0; d < deferred.size(); d++) {
        acc += qs[deferred[d].query].n_targets;
        if (acc >= share || d + 1 == deferred.size()) {
            pool.emplace_back(&SwPrepare::cut_list_jobs_of, this, from, d + 1);
            from = d + 1;
            acc = 0;
        }
    }
    for (std::thread &t : pool) t.join();
}

// dense lists: query i's list is positions [begin, begin + count) of the length-ordered id list, so it is sorted already and the
// cells of any stretch of it come from the prefix sums - the same cuts as cut_list_jobs_of without touching a pair
void SwPrepare::cut_dense_jobs() {
    per_query.resize(deferred.size());
    for (size_t d = 0; d < deferred.size(); d++) {
        const Deferred &D = deferred[d];
        const uint64_t qlen = qs[D.query].qlen;
        const uint32_t beg = dense->begin[D.query], n = dense->count[D.query];
        const uint64_t *pre = dense->len_prefix + beg;
        PerQuery &P = per_query[d];
        P.sum_cells = qlen * (pre[n] - pre[0]);
        P.max_tlen = n ? tv.h_len[dense->order[beg]] : 0;
        for (uint32_t k = 0; k < n;) {
            uint64_t jc = 0;
            uint32_t e = k;
            while (e < n && e - k < JOB_HITS) {
                const uint32_t stop = std::min<uint32_t>(e + D.round, n);
                jc += qlen * (pre[stop] - pre[e]);
                e = stop;
                const uint32_t held = e - k;
                if (jc >= JOB_CELLS && (held <= 16 || held % JOB_ROUND == 0)) break;
            }
            P.jobs.push_back(SwJob{D.query, D.hit_cursor + k, D.hit_cursor + e, D.shape});
            P.cells.push_back(jc);
            k = e;
        }
    }
}

int SwPrepare::join_list_jobs() {
    for (size_t d = 0; d < deferred.size(); d++) {
        const Deferred &D = deferred[d];
        PerQuery &P = per_query[d];
        if (P.bad) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: target id out of range");
        b->cells += P.sum_cells;
        max_tlen = std::max(max_tlen, P.max_tlen);
        for (size_t z = 0; z < P.jobs.size(); z++) {
            SwJob j = P.jobs[z];
            if (D.multi) j.shape |= n_multi++ << 8;
            jobs.push_back(j);
            job_cells.push_back(P.cells[z]);
        }
        const uint32_t n_t = dense ? 0u : qs[D.query].n_targets;      // (dense batches are SCORE_END)
        if (D.multi && mode >= MMGPU_SW_START && n_t)
            add_rev_jobs(D.query, D.hit_cursor, n_t, D.shape, (uint64_t)qs[D.query].qlen * (P.rev_mid_len + 1));
    }
    return MMGPU_OK;
}

// `sorted` = the forward jobs by kernel group, longest job first inside a group (the dispatcher hands out workgroups in blockIdx
// order, so the tail is the shortest jobs), then the reverse-scan jobs, longest first
void SwPrepare::order_jobs() {
    sorted.resize(jobs.size());
    std::vector<uint32_t> ord(jobs.size());
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t bb) {
        const int ga = sw_shape_group(jobs[a].shape & 0xFFu), gb = sw_shape_group(jobs[bb].shape & 0xFFu);
        return ga != gb ? ga < gb : job_cells[a] > job_cells[bb];
    });
    for (size_t z = 0; z < ord.size(); z++) {
        sorted[z] = jobs[ord[z]];
        b->group_begin[sw_shape_group(sorted[z].shape & 0xFFu) + 1]++;
    }
    for (int g = 0; g < SW_GROUPS; g++) b->group_begin[g + 1] += b->group_begin[g];
    b->n_jobs = (uint32_t)sorted.size();
    b->n_multi_jobs = n_multi;
    std::vector<uint32_t> ro(rev_jobs.size());
    std::iota(ro.begin(), ro.end(), 0u);
    std::stable_sort(ro.begin(), ro.end(), [&](uint32_t a, uint32_t bb) { return rev_cells[a] > rev_cells[bb]; });
    for (uint32_t z : ro) sorted.push_back(rev_jobs[z]);
    b->n_rev_jobs = (uint32_t)rev_jobs.size();
}

int SwPrepare::enqueue_uploads() {
    b->pairs = total_hits;
    b->h_qoff = qoff;
    b->from_pf = pf != nullptr;
    b->pf_stride = pf_stride;
    b->slot_stride = pf_stride;
    hipStream_t s = c->stream;
    mat.assign(par->mat, par->mat + par->alphabet * par->alphabet);
    // lists on the device (pf): the stream still holds the prefilter batch - the uploads go through pinned staging so that this
    // thread is not parked behind it (mmgpu_ctx::pinned); sized here, once, for everything uploaded below
    void *pin = nullptr;
    size_t pin_cap = 0, pin_used = 0;
    if (pf) {
        pin_cap = upload_pinned_need(qres.size()) + upload_pinned_need(qcb.size()) + upload_pinned_need(qoff.size() * 4) +
                  upload_pinned_need(qbias.size() * 4) + upload_pinned_need(qminstart.size() * 4) + upload_pinned_need(mat.size()) +
                  upload_pinned_need((jobs.size() + rev_jobs.size()) * sizeof(SwJob)) + upload_pinned_need(qprof.size()) +
                  upload_pinned_need(qprof_off.size() * 4);
        pin = pinned.acquire(c, pin_cap);      // (nothing of an earlier batch is in flight from it: every prepare ends with the stream drained)
    }
    auto up = [&](DevBuf &buf, const auto &vec) { return upload_pinned(buf, vec, s, pin, pin_cap, pin_used); };
    HIP_TRY(up(b->d_qres, qres));
    HIP_TRY(up(b->d_qcb, qcb));
    HIP_TRY(up(b->d_qoff, qoff));
    HIP_TRY(up(b->d_qbias, qbias));
    HIP_TRY(up(b->d_qminstart, qminstart));
    if (b->any_profile) {
        HIP_TRY(up(b->d_qprof, qprof));
        HIP_TRY(up(b->d_qprof_off, qprof_off));
    }
    if (pf) {
        HIP_TRY(b->d_hit_target.alloc(std::max<size_t>((size_t)total_hits, 1) * 4));
        HIP_TRY(b->d_hit_out.alloc(std::max<size_t>((size_t)total_hits, 1) * 4));
        HIP_TRY(b->d_stats.alloc(SW_FROM_PF_STAT_SLOTS * 24));      // (cells, pairs, longest target) x slots: sw_from_pf_kernel
        HIP_TRY(hipMemsetAsync(b->d_stats.p, 0, SW_FROM_PF_STAT_SLOTS * 24, s));
        HIP_TRY(b->d_pf_counts.alloc(std::max<size_t>(nq, 1) * 4));
        HIP_TRY(b->d_slot_target.alloc(std::max<size_t>((size_t)total_hits, 1) * 4));
    } else if (dense) {
        b->x_hit_target = dense->d_hit_target;
        b->x_hit_out = dense->d_hit_out;
        b->x_out = dense->d_out;
    } else {
        HIP_TRY(upload(b->d_hit_target, hit_target, s));
        HIP_TRY(upload(b->d_hit_out, hit_out, s));
    }
    HIP_TRY(up(b->d_mat, mat));
    if (!dense) HIP_TRY(b->d_out.alloc(std::max<size_t>((size_t)total_hits, 1) * sizeof(mmgpu_sw_hit)));
    order_jobs();
    HIP_TRY(up(b->d_jobs, sorted));
    return MMGPU_OK;
}

// column scratch of the multi-tile jobs: a pool with one slot per workgroup that can be resident at once (not one
// per job: a batch of long queries against one very long target would ask for 100+ GB), sized by the longest
// target any list holds
hipError_t SwPrepare::alloc_scratch(uint32_t longest) {
    b->scratch_cols = ((longest + 15u) & ~15u) + 16;      // whole 16-column stretches: every line starts on a 128-byte boundary
    b->scratch_slots = std::min<uint32_t>(std::max<uint32_t>(std::max<uint32_t>(n_multi, (uint32_t)rev_jobs.size()), 1),
                                          sw_multi_resident_blocks(b->group_lds[SW_GROUPS - 1], mode >= MMGPU_SW_START, c->compute_units));
    hipError_t e = b->d_scratch.alloc((size_t)b->scratch_slots * 4 * 4 * 2 * (size_t)b->scratch_cols * sizeof(uint2));
    if (e != hipSuccess) return e;
    e = b->d_scratch_busy.alloc((size_t)b->scratch_slots * 4);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(b->d_scratch_busy.p, 0, (size_t)b->scratch_slots * 4, c->stream);
}

int SwPrepare::finish_host_lists() {
    if (any_multi) HIP_TRY(alloc_scratch(max_tlen));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the host vectors of this call die with it
    return MMGPU_OK;
}

// sw_from_pf_kernel orders every list by target length and counts cells, pairs and the longest target, which sizes the scratch
int SwPrepare::order_device_lists() {
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(b->d_out.p, 0, std::max<size_t>((size_t)total_hits, 1) * sizeof(mmgpu_sw_hit), s));
    SwFromPfArgs F;
    F.pf_hits = pf->hits;
    F.pf_stride = pf_stride;
    F.hit_count = pf->counts;
    F.stride = pf_stride;
    F.q_off = b->d_qoff.as<uint32_t>();
    F.t_len = tv.len;
    F.hit_target = b->d_hit_target.as<uint32_t>();
    F.hit_out = b->d_hit_out.as<uint32_t>();
    F.cells = b->d_stats.as<unsigned long long>();
    F.pairs = b->d_stats.as<unsigned long long>() + 1;
    F.count_copy = b->d_pf_counts.as<uint32_t>();
    F.slot_target = b->d_slot_target.as<uint32_t>();
    HIP_TRY(launch_sw_from_pf(F, nq, s));
    HIP_TRY(hipStreamSynchronize(s));   // the host vectors of this call die with it
    unsigned long long st[3] = {0, 0, 0}, slots[SW_FROM_PF_STAT_SLOTS * 3];
    HIP_TRY(hipMemcpy(slots, b->d_stats.p, sizeof(slots), hipMemcpyDeviceToHost));
    for (int z = 0; z < SW_FROM_PF_STAT_SLOTS; z++) {
        st[0] += slots[z * 3];
        st[1] += slots[z * 3 + 1];
        st[2] = std::max(st[2], slots[z * 3 + 2]);
    }
    b->cells = st[0];
    b->valid_pairs = st[1];
    if (any_multi) {
        HIP_TRY(alloc_scratch((uint32_t)st[2]));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return MMGPU_OK;
}

}  // namespace

static int sw_prepare_impl(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, int mode,
                           const DeviceLists *pf, const mmgpu_sw_masks *masks, mmgpu_sw_batch_t **out, const SwDenseLists *dense = nullptr) {
    if (!c || !par || !out || (!qs && nq)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare: NULL argument");
    SwPrepare S{c, par, qs, nq, mode, pf, masks, dense};
    if (int e = S.check_params()) return e;
    S.tv = sw_targets(c, nullptr);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mmgpu_sw_batch_t, SwBatchFree> b(new mmgpu_sw_batch_t(), SwBatchFree{c});
    S.b = b.get();
    S.new_batch();
    if (int e = S.size_buffers()) return e;
    if (masks)
        if (int e = S.plan_masked()) return e;
    if (int e = S.copy_queries()) return e;
    S.lap("queries copied, buffers sized");
    if (!S.deferred.empty()) {
        if (dense) S.cut_dense_jobs();
        else S.cut_list_jobs();
        S.lap("lists sorted by target length, jobs cut (threads)");
        if (int e = S.join_list_jobs()) return e;
    }
    S.lap("jobs joined");
    if (int e = S.enqueue_uploads()) return e;
    S.lap("uploads enqueued, jobs ordered");
    if (masks) {
        if (int e = S.gather_masked()) return e;
        S.lap("masked copies of the targets gathered");
    }
    if (int e = pf ? S.order_device_lists() : S.finish_host_lists()) return e;
    S.lap("scratch + stream drained");
    *out = b.release();
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_prepare(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq,
                                int mode, mmgpu_sw_batch_t **out) {
    return sw_prepare_impl(c, par, qs, nq, mode, nullptr, nullptr, out);
}

extern "C" int mmgpu_sw_prepare_masked(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, int mode,
                                       const mmgpu_sw_masks *masks, mmgpu_sw_batch_t **out) {
    if (out) *out = nullptr;
    if (!masks) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_masked: NULL masks");
    return sw_prepare_impl(c, par, qs, nq, mode, nullptr, masks, out);
}

// test hook: pair p's copy as the kernels read it, its pad letters included
extern "C" int mmgpu_sw_debug_masked_target(mmgpu_ctx *c, mmgpu_sw_batch_t *b, uint32_t pair, uint8_t *out, size_t cap, uint32_t *len) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_debug_masked_target: NULL argument");
    if (!b->masked) return fail(MMGPU_ERR_STATE, "mmgpu_sw_debug_masked_target: not a batch of mmgpu_sw_prepare_masked");
    if (pair >= b->m_h_len.size()) return fail(MMGPU_ERR_ARG, "mmgpu_sw_debug_masked_target: pair index out of range");
    const uint32_t l = b->m_h_len[pair];
    const size_t bytes = ((size_t)l + 3) & ~(size_t)3;
    if (len) *len = l;
    if (!out && cap == 0) return MMGPU_OK;      // the size query
    if (cap < bytes || (!out && bytes)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_debug_masked_target: buffer too small (needs (len + 3) & ~3 bytes)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t off4 = 0;
    HIP_TRY(hipMemcpy(&off4, b->m_off4.as<uint32_t>() + pair, 4, hipMemcpyDeviceToHost));
    if (bytes) HIP_TRY(hipMemcpy(out, b->m_res.as<uint8_t>() + (size_t)off4 * 4, bytes, hipMemcpyDeviceToHost));
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_prepare_from_pf(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq,
                                        int mode, mmgpu_pf_batch_t *pf, mmgpu_sw_batch_t **out) {
    if (!pf) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_from_pf: NULL prefilter batch");
    DeviceLists L;
    uint32_t pf_nq = 0;
    if (!pf_batch_device_lists(pf, &L.hits, &L.counts, &L.stride, &pf_nq))
        return fail(MMGPU_ERR_STATE, "mmgpu_sw_prepare_from_pf: the prefilter batch was never run, or is an exchange batch of a sharded run");
    if (pf_nq != nq) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_from_pf: query count differs from the prefilter batch");
    return sw_prepare_impl(c, par, qs, nq, mode, &L, nullptr, out);
}

extern "C" int mmgpu_sw_prepare_from_lists(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, int mode,
                                           const void *d_hits, const void *d_counts, uint32_t stride, mmgpu_sw_batch_t **out) {
    if ((!d_hits || !d_counts) && nq) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_from_lists: NULL list pointers");
    if (stride == 0) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_from_lists: stride must be >= 1");
    DeviceLists L;
    L.hits = (const mmgpu_pf_hit *)d_hits;
    L.counts = (const uint32_t *)d_counts;
    L.stride = stride;
    return sw_prepare_impl(c, par, qs, nq, mode, &L, nullptr, out);
}

// ---- multi-GPU: every rank aligns the pairs of the merged lists whose target it holds; the records are gathered over the
// communicator in merged-list order ("run each pair on the GPU owning t; gather mmgpu_sw_hits per query") ----
extern "C" int mmgpu_sw_prepare_owned(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, int mode,
                                      mmgpu_pf_batch_t *merged, mmgpu_sw_batch_t **out) {
    if (!c || !merged || !out) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_owned: NULL argument");
    if (!c->shard.on) return fail(MMGPU_ERR_STATE, "mmgpu_sw_prepare_owned: no shard set (mmgpu_pf_set_shard)");
    const mmgpu_pf_hit *mh = nullptr;
    const uint32_t *mc = nullptr;
    uint32_t stride = 0, mnq = 0;
    if (!mmgpu::pf_batch_merged_lists(merged, &mh, &mc, &stride, &mnq)) return fail(MMGPU_ERR_STATE, "mmgpu_sw_prepare_owned: the prefilter batch holds no merged lists (mmgpu_pf_exchange_merge first)");
    if (mnq != nq) return fail(MMGPU_ERR_ARG, "mmgpu_sw_prepare_owned: query count differs from the prefilter batch");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf lh, lc, ls;
    lh.bind(c->cache); lc.bind(c->cache); ls.bind(c->cache);
    HIP_TRY(lh.alloc(std::max<size_t>((size_t)nq * stride, 1) * sizeof(mmgpu_pf_hit)));
    HIP_TRY(lc.alloc(std::max<size_t>(nq, 1) * 4));
    HIP_TRY(ls.alloc(std::max<size_t>((size_t)nq * stride, 1) * 4));
    PfLocalizeArgs A;
    A.hits = mh;
    A.counts = mc;
    A.nq = nq;
    A.stride = stride;
    A.shard = c->shard.shard;
    A.shard_of = c->shard.d_shard_of.as<uint32_t>();
    A.local_id = c->shard.d_local_id.as<uint32_t>();
    A.local_hits = lh.as<mmgpu_pf_hit>();
    A.local_counts = lc.as<uint32_t>();
    A.local_slot = ls.as<uint32_t>();
    HIP_TRY(launch_pf_localize(A, c->stream));
    DeviceLists L;
    L.hits = lh.as<mmgpu_pf_hit>();
    L.counts = lc.as<uint32_t>();
    L.stride = stride;
    if (int e = sw_prepare_impl(c, par, qs, nq, mode, &L, nullptr, out)) return e;
    mmgpu_sw_batch_t *b = *out;
    b->owned = true;
    b->o_stride = stride;
    b->o_lhits = std::move(lh);
    b->o_lcounts = std::move(lc);
    b->o_lslot = std::move(ls);
    return MMGPU_OK;
}

namespace mmgpu {

// phase 1: pack the owned records (compacted with a device counter) and name the two all-gathers of the step.  The send
// buffer holds 1.5 x the even share of the slots (+ 4096): the deal by length bucket gives every rank its share to within
// a few percent; a rank that packs more reports it in its counter and the scatter phase raises the batch's overflow status.
int sw_gather_begin(mmgpu_ctx *c, mmgpu_sw_batch_t *b, int n_ranks, XchgBlock blocks[2]) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_gather_owned: NULL argument");
    if (!b->owned || !b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_gather_owned: not a batch of mmgpu_sw_prepare_owned that has been run");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t slots = (uint64_t)b->n_queries * b->o_stride;
    static const char *dense = getenv("MMGPU_SW_GATHER_DENSE");      // every rank may own everything (no overflow possible)
    const uint64_t cap64 = (dense || b->o_dense || n_ranks == 1) ? slots : std::min<uint64_t>(slots, slots / (uint64_t)n_ranks * 3 / 2 + 4096);
    const uint32_t cap = (uint32_t)std::max<uint64_t>(cap64, 1);
    if (b->o_cap != cap || b->o_ranks != n_ranks) {
        for (DevBuf *d : {&b->o_send, &b->o_counter, &b->o_recv, &b->o_recv_counters, &b->o_full, &b->o_status}) d->bind(c->cache);
        HIP_TRY(b->o_send.alloc((size_t)cap * sizeof(SwOwnedRec)));
        HIP_TRY(b->o_counter.alloc(8));
        HIP_TRY(b->o_recv.alloc((size_t)cap * sizeof(SwOwnedRec) * n_ranks));
        HIP_TRY(b->o_recv_counters.alloc((size_t)8 * n_ranks));
        HIP_TRY(b->o_full.alloc(std::max<size_t>(slots, 1) * sizeof(mmgpu_sw_hit)));
        HIP_TRY(b->o_status.alloc(8));
        b->o_cap = cap;
        b->o_ranks = n_ranks;
    }
    HIP_TRY(hipMemsetAsync(b->o_counter.p, 0, 8, c->stream));
    SwOwnedPackArgs P;
    P.res = b->d_out.as<mmgpu_sw_hit>();
    P.local_counts = b->o_lcounts.as<uint32_t>();
    P.local_slot = b->o_lslot.as<uint32_t>();
    P.nq = b->n_queries;
    P.stride = b->o_stride;
    P.send = b->o_send.as<SwOwnedRec>();
    P.cap = cap;
    P.counter = b->o_counter.as<uint32_t>();
    HIP_TRY(launch_sw_owned_pack(P, c->stream));
    blocks[0] = XchgBlock{b->o_send.p, b->o_recv.p, (size_t)cap * sizeof(SwOwnedRec)};
    blocks[1] = XchgBlock{b->o_counter.p, b->o_recv_counters.p, 8};
    return MMGPU_OK;
}

// after phase 3: did a rank pack more than its send buffer holds (hits clustered in one shard)?  Every rank sees all counters, so
// every rank answers the same; the caller then repeats the three phases with buffers that hold every slot (o_dense).
int sw_gather_overflowed(mmgpu_ctx *c, mmgpu_sw_batch_t *b, bool *overflowed) {
    HIP_TRY(hipSetDevice(c->device));
    uint32_t st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st, b->o_status.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *overflowed = st[1] != 0 && !b->o_dense;
    if (*overflowed) b->o_dense = true;
    return MMGPU_OK;
}

// phase 3: scatter every rank's records into the merged-list order
int sw_gather_finish(mmgpu_ctx *c, mmgpu_sw_batch_t *b, int n_ranks) {
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t slots = (uint64_t)b->n_queries * b->o_stride;
    HIP_TRY(hipMemsetAsync(b->o_full.p, 0, std::max<size_t>(slots, 1) * sizeof(mmgpu_sw_hit), c->stream));
    HIP_TRY(hipMemsetAsync(b->o_status.p, 0, 8, c->stream));
    SwOwnedScatterArgs S;
    S.recv = b->o_recv.as<SwOwnedRec>();
    S.counters = b->o_recv_counters.as<uint32_t>();
    S.n_ranks = (uint32_t)n_ranks;
    S.cap = b->o_cap;
    S.n_slots = (uint32_t)slots;
    S.full = b->o_full.as<mmgpu_sw_hit>();
    S.status = b->o_status.as<uint32_t>();
    HIP_TRY(launch_sw_owned_scatter(S, c->stream));
    return MMGPU_OK;
}

}  // namespace mmgpu

extern "C" int mmgpu_sw_gather_owned(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const void **d_full, const void **d_status) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_gather_owned: NULL argument");
    const int n = c->comm ? c->comm->n_ranks : 1;
    for (int attempt = 0; attempt < 2; attempt++) {
        mmgpu::XchgBlock blk[2];
        if (int e = mmgpu::sw_gather_begin(c, b, n, blk)) return e;
        for (int k = 0; k < 2; k++)
            if (int e = mmgpu::comm_allgather(c, blk[k].send, blk[k].recv, blk[k].bytes)) return e;
        if (int e = mmgpu::sw_gather_finish(c, b, n)) return e;
        // uneven shards: one more round with send buffers that hold every slot (all ranks decide alike: they see all counters)
        bool again = false;
        if (n > 1 && attempt == 0)
            if (int e = mmgpu::sw_gather_overflowed(c, b, &again)) return e;
        if (!again) break;
    }
    if (d_full) *d_full = b->o_full.p;
    if (d_status) *d_status = b->o_status.p;
    return MMGPU_OK;
}

// host copy of the gathered records (synchronises the context's stream); MMGPU_ERR_STATE if a rank's send buffer overflowed
// (cannot happen after mmgpu_sw_gather_owned's own second round; kept as the check it is)
extern "C" int mmgpu_sw_fetch_owned(mmgpu_ctx *c, mmgpu_sw_batch_t *b, mmgpu_sw_hit *out, uint32_t *records) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_fetch_owned: NULL argument");
    if (!b->owned || !b->o_full.p) return fail(MMGPU_ERR_STATE, "mmgpu_sw_fetch_owned: nothing gathered (mmgpu_sw_gather_owned first)");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st, b->o_status.p, 8, hipMemcpyDeviceToHost, c->stream));
    if (out) HIP_TRY(hipMemcpyAsync(out, b->o_full.p, (size_t)b->n_queries * b->o_stride * sizeof(mmgpu_sw_hit), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (records) *records = st[0];
    if (st[1]) return fail(MMGPU_ERR_STATE, "mmgpu_sw_fetch_owned: the send buffer of a rank overflowed (uneven shards); rerun the gather with MMGPU_SW_GATHER_DENSE=1");
    return MMGPU_OK;
}

// The kernel groups of a batch, forked from / joined to the context's stream.  rev_only: the forward results are in d_out, only
// the reverse scan of the pairs flagged in rev_force runs (mmgpu_sw_reverse_pairs).
static int sw_launch_groups(mmgpu_ctx *c, mmgpu_sw_batch_t *b, bool rev_only, const uint8_t *rev_force) {
    // one launch per kernel group (jobs longest first); the groups run concurrently on side streams forked from /
    // joined to the context's stream.  With start positions asked for, a workgroup runs the reverse scan of its
    // pairs right after their forward scan (it reads the forward results of its own pairs only).
    if (!c->fork) {
        // the group with the long multi-tile jobs gets the highest stream priority: its forward + reverse chain is
        // the critical path, the other groups fill the CUs it leaves
        int prio_low = 0, prio_high = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));   // numerically lower = higher priority
        for (int g = 0; g < SW_GROUPS; g++) {
            const int prio = g == SW_GROUPS - 1 ? prio_high : (g == 0 ? prio_low : (prio_low + prio_high) / 2);
            HIP_TRY(hipStreamCreateWithPriority(&c->side[g], hipStreamNonBlocking, prio));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
        for (auto &e : c->join) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(c->fork, c->stream));
    for (int g = 0; g < SW_GROUPS; g++) HIP_TRY(hipStreamWaitEvent(c->side[g], c->fork, 0));
    const TargetView T = sw_targets(c, b);
    for (int g = SW_GROUPS - 1; g >= 0; g--) {
        hipStream_t st = c->side[g];
        {
            SwLaunch L;
            L.jobs = b->d_jobs.as<SwJob>() + b->group_begin[g];
            L.n_jobs = b->group_begin[g + 1] - b->group_begin[g];
            L.q_res = b->d_qres.as<uint8_t>();
            L.q_cb = b->d_qcb.as<int8_t>();
            L.q_off = b->d_qoff.as<uint32_t>();
            L.q_bias = b->d_qbias.as<int32_t>();
            L.q_minstart = b->d_qminstart.as<int32_t>();
            L.q_prof = b->any_profile ? b->d_qprof.as<int8_t>() : nullptr;
            L.q_prof_off = b->any_profile ? b->d_qprof_off.as<uint32_t>() : nullptr;
            L.t_res = T.res;
            L.t_off4 = T.off4;
            L.t_len = T.len;
            L.hit_target = b->x_hit_target ? b->x_hit_target : b->d_hit_target.as<uint32_t>();
            L.hit_out = b->x_hit_out ? b->x_hit_out : b->d_hit_out.as<uint32_t>();
            L.out = b->x_out ? b->x_out : b->d_out.as<mmgpu_sw_hit>();
            L.mat = b->d_mat.as<int8_t>();
            L.alphabet = b->alphabet;
            L.gap_open = b->gap_open;
            L.gap_extend = b->gap_extend;
            L.q_hit_count = b->from_pf ? b->d_pf_counts.as<uint32_t>() : nullptr;
            L.hit_stride = b->slot_stride;
            L.scratch = b->d_scratch.as<uint2>();
            L.scratch_cols = b->scratch_cols;
            L.scratch_busy = b->d_scratch_busy.as<uint32_t>();
            L.scratch_slots = std::max<uint32_t>(b->scratch_slots, 1);
            L.resident_lds = SW_RESIDENT_LDS;
            L.rev_mode = rev_only ? 2 : (b->mode == MMGPU_SW_START_NOT_WORD ? 1 : 0);
            L.rev_only = rev_only ? 1 : 0;
            L.rev_force = rev_force;
            L.half_wide = sw_half_wide() ? 1 : 0;
            HIP_TRY(launch_sw(L, g, b->group_lds[g], b->mode >= MMGPU_SW_START, st));
            if (g == SW_GROUPS - 1 && b->n_rev_jobs && b->mode >= MMGPU_SW_START) {   // reads the forward results of this stream's kernel
                SwLaunch Rv = L;
                Rv.jobs = b->d_jobs.as<SwJob>() + b->n_jobs;
                Rv.n_jobs = b->n_rev_jobs;
                HIP_TRY(launch_sw_rev_multi(Rv, b->group_lds[g], st));
            }
            if (getenv("MMGPU_TRACE")) {   // debugging aid: run the groups one at a time and say which one is in flight
                fprintf(stderr, "[sw_run] group %d jobs %u lds %zu both %d from_pf %d scratch_cols %u\n", g, L.n_jobs, b->group_lds[g], (int)(b->mode >= MMGPU_SW_START), (int)b->from_pf, b->scratch_cols);
                fflush(stderr);
                const auto t0 = std::chrono::steady_clock::now();
                hipError_t e = hipStreamSynchronize(st);
                fprintf(stderr, "[sw_run] group %d done after %.2f ms: %s\n", g,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), hipGetErrorString(e));
                fflush(stderr);
            }
        }
    }
    for (int k = 0; k < SW_GROUPS; k++) {
        HIP_TRY(hipEventRecord(c->join[k], c->side[k]));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->join[k], 0));
    }
    return MMGPU_OK;
}

namespace mmgpu {
int sw_prepare_dense(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, const SwDenseLists &lists, mmgpu_sw_batch_t **out) {
    return sw_prepare_impl(c, par, qs, nq, MMGPU_SW_SCORE_END, nullptr, nullptr, out, &lists);
}
int sw_run_dense(mmgpu_ctx *c, mmgpu_sw_batch_t *b) { return sw_launch_groups(c, b, false, nullptr); }
}  // namespace mmgpu

extern "C" int mmgpu_sw_run(mmgpu_ctx *c, mmgpu_sw_batch_t *b) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_run: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (b->events.size() < 256) {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        b->events.push_back(std::make_pair(ev0, ev1));
        HIP_TRY(hipEventRecord(ev0, c->stream));
    }
    if (int e = sw_launch_groups(c, b, false, nullptr)) return e;
    if (ev1) HIP_TRY(hipEventRecord(ev1, c->stream));
    b->ran = true;
    b->h_res_valid = false;
    return MMGPU_OK;
}

// Start positions after the fact for the pairs the caller names (MMGPU_SW_START_NOT_WORD batches: the int16-range hits the block
// aligner declined, StripedSmithWaterman.cpp:873-882 "Block alignment failed" -> alignStartPosBacktrace): the reverse scan of
// exactly those pairs, the forward results staying as they are.
extern "C" int mmgpu_sw_reverse_pairs(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const uint32_t *pair_index, uint32_t n, mmgpu_sw_hit *out) {
    if (!c || !b || (!pair_index && n)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_reverse_pairs: NULL argument");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_reverse_pairs: batch was never run");
    if (b->mode < MMGPU_SW_START) return fail(MMGPU_ERR_STATE, "mmgpu_sw_reverse_pairs: the batch was prepared without a start-position mode");
    if (b->owned) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_reverse_pairs: not for batches of owned pairs (sharded runs)");
    if (n == 0) return MMGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint8_t> flags((size_t)b->pairs, (uint8_t)0);
    for (uint32_t k = 0; k < n; k++) {
        if (pair_index[k] >= b->pairs) return fail(MMGPU_ERR_ARG, "mmgpu_sw_reverse_pairs: pair index out of range");
        flags[pair_index[k]] = 1;
    }
    DevBuf d_flags;
    d_flags.bind(c->cache);
    HIP_TRY(d_flags.alloc(flags.size()));
    HIP_TRY(hipMemcpyAsync(d_flags.p, flags.data(), flags.size(), hipMemcpyHostToDevice, c->stream));
    if (int e = sw_launch_groups(c, b, true, d_flags.as<uint8_t>())) return e;
    if (out)
        for (uint32_t k = 0; k < n; k++)
            HIP_TRY(hipMemcpyAsync(out + k, b->d_out.as<mmgpu_sw_hit>() + pair_index[k], sizeof(mmgpu_sw_hit), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the flags die with this scope)
    if (b->h_res_valid)      // the host copy mmgpu_sw_traceback / mmgpu_sw_block_backtrace read
        for (uint32_t k = 0; k < n; k++)
            HIP_TRY(hipMemcpy(&b->h_res[pair_index[k]], b->d_out.as<mmgpu_sw_hit>() + pair_index[k], sizeof(mmgpu_sw_hit), hipMemcpyDeviceToHost));
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_fetch(mmgpu_ctx *c, mmgpu_sw_batch_t *b, mmgpu_sw_hit *out) {
    if (!c || !b || (!out && b->pairs)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_fetch: NULL argument");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_fetch: batch was never run");
    HIP_TRY(hipSetDevice(c->device));
    if (b->pairs)
        HIP_TRY(hipMemcpyAsync(out, b->d_out.p, (size_t)b->pairs * sizeof(mmgpu_sw_hit), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_fetch_device(mmgpu_ctx *c, mmgpu_sw_batch_t *b, void *d_out) {
    if (!c || !b || (!d_out && b->pairs)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_fetch_device: NULL argument");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_fetch_device: batch was never run");
    HIP_TRY(hipSetDevice(c->device));
    if (b->pairs)
        HIP_TRY(hipMemcpyAsync(d_out, b->d_out.p, (size_t)b->pairs * sizeof(mmgpu_sw_hit), hipMemcpyDeviceToDevice, c->stream));
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_batch_stats(mmgpu_sw_batch_t *b, uint64_t *cells, uint64_t *pairs) {
    if (!b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_batch_stats: NULL argument");
    if (cells) *cells = b->cells;
    if (pairs) *pairs = b->from_pf ? b->valid_pairs : b->pairs;
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_last_kernel_ms(mmgpu_ctx *c, mmgpu_sw_batch_t *b, float *ms) {
    if (!c || !b || !ms) return fail(MMGPU_ERR_ARG, "mmgpu_sw_last_kernel_ms: NULL argument");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_last_kernel_ms: batch was never run");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(b->events.back().second));
    HIP_TRY(hipEventElapsedTime(ms, b->events.back().first, b->events.back().second));
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_kernel_ms_mean(mmgpu_ctx *c, mmgpu_sw_batch_t *b, uint32_t last_n, float *ms, uint32_t *n_used) {
    if (!c || !b || !ms) return fail(MMGPU_ERR_ARG, "mmgpu_sw_kernel_ms_mean: NULL argument");
    if (!b->ran || b->events.empty()) return fail(MMGPU_ERR_STATE, "mmgpu_sw_kernel_ms_mean: batch was never run");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = std::min<size_t>(last_n ? last_n : b->events.size(), b->events.size());
    double sum = 0;
    for (size_t k = b->events.size() - n; k < b->events.size(); k++) {
        float t = 0;
        HIP_TRY(hipEventSynchronize(b->events[k].second));
        HIP_TRY(hipEventElapsedTime(&t, b->events[k].first, b->events[k].second));
        sum += t;
    }
    *ms = (float)(sum / (double)n);
    if (n_used) *n_used = (uint32_t)n;
    return MMGPU_OK;
}

extern "C" void mmgpu_sw_free(mmgpu_ctx *c, mmgpu_sw_batch_t *b) {
    if (!b) return;
    if (c) (void)hipSetDevice(c->device);
    for (auto &e : b->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete b;
}

extern "C" int mmgpu_sw_batch(mmgpu_ctx *c, const mmgpu_sw_params *par, const mmgpu_sw_query *qs, uint32_t nq, int mode,
                              mmgpu_sw_hit *out) {
    mmgpu_sw_batch_t *b = nullptr;
    int rc = mmgpu_sw_prepare(c, par, qs, nq, mode, &b);
    if (rc != MMGPU_OK) return rc;
    rc = mmgpu_sw_run(c, b);
    if (rc == MMGPU_OK) rc = mmgpu_sw_fetch(c, b, out);
    mmgpu_sw_free(c, b);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------
// backtrace
// ---------------------------------------------------------------------------------------------------------
// host copies of the results (and, for device-resident lists, of the slot -> target map): fetched once per run of the batch
static int sw_host_results(mmgpu_sw_batch_t *b, hipStream_t s) {
    if (b->h_res_valid) return MMGPU_OK;
    b->h_res.resize((size_t)b->pairs);
    if (b->pairs) HIP_TRY(hipMemcpyAsync(b->h_res.data(), b->d_out.p, (size_t)b->pairs * sizeof(mmgpu_sw_hit), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (b->from_pf) {
        b->h_slot_target.resize((size_t)b->pairs);
        if (b->pairs) HIP_TRY(hipMemcpy(b->h_slot_target.data(), b->d_slot_target.p, (size_t)b->pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    b->h_res_valid = true;
    return MMGPU_OK;
}

// ---- a15: the block aligner's start position / backtrace for int16-range hits (block_kernel.hip) ----
struct BlockAuto { uint32_t selected = 0, ok = 0, declined = 0, too_large = 0; };      // mmgpu_sw_block_starts: what the device selected / answered

namespace {

// what an entry point wants of block_backtrace
struct BlockWant {
    BlockAuto *select = nullptr;    // mmgpu_sw_block_starts: the device picks the pairs, their answers go into the batch's records
    bool starts_only = false;       // start positions only: no trace, no walk
    bool no_strings = false;        // start positions / identities / lengths only (implied by starts_only)
    uint32_t *growth = nullptr;     // mmgpu_sw_block_growth: the block lists
    uint32_t growth_cap = 0;
};

// One call of block_backtrace: its arguments and what its steps hand to one another.  The steps run in the order they are declared
// in.  Three tiers of block_kernel.hip (tier_rounds) take what the four-pairs-per-wavefront kernels of block4_kernel.hip
// (block4_passes: sequence queries) leave; every launch answers MMGPU_BLOCK_TOO_LARGE for a pair it hands on.
struct BlockRun {
    mmgpu_ctx *c;
    mmgpu_sw_batch_t *b;
    const uint32_t *pair_index;
    uint32_t n;                      // pairs asked for; with BlockWant::select: pairs the device selected
    mmgpu_sw_block *out;             // [n] host copy of the answers (select: in the pinned arena, or out_auto)
    char *bt;
    BlockWant want;
    hipStream_t s;                   // the context's stream

    std::vector<BlockJob> jobs;      // int16-range pairs, longest first once ordered
    std::vector<BlockJob> slow_jobs; // what block4_passes leaves: profile queries, pairs whose slot would not fit the pool
    std::vector<uint64_t> bt_off;    // [n] where a pair's string goes (multiples of four)
    uint64_t off = 0;                // ... and their total
    std::vector<mmgpu_sw_block> out_auto;
    PinnedLease pinned;              // the context's staging arena, held to the end of the call (`out` may point into it)
    std::vector<int8_t> scores;
    std::vector<uint32_t> resume;    // per slot: the first minimum block size still to try (bit 16: only the slot was too small)
    size_t growth_bytes = 0;
    const char *first_tier_env = getenv("MMGPU_BLOCK_FIRST_TIER");      // test aid: every pair through block_kernel.hip's tier 0 / 1 / 2
    BlockLaunch L;
    DevBuf d_out, d_sel_jobs, d_sel_pairs, d_sel_cnt, d_flags, d_btoff, d_bt, d_scores, d_growth, d_jobs[3], d_pool[3], d_busy[3];
    struct PassBufs {      // what a block4 launch in flight holds: two of them run side by side (everything else, the long head)
        DevBuf j2, cnt, pool, ck;
        hipStream_t st = nullptr;
        Block4Plan plan;
    } PB[2];
    // (the streams last: a return with work in flight on one of them waits for it before the buffers above go back to the cache.
    // They live to the end of the call - the head's beside the two of tier_rounds, three besides the context's at most - and their
    // holders wait once more for streams the steps have already drained)
    SideStream head_stream, extra[2];
    double t_mark = prep_now();

    BlockRun(mmgpu_ctx *c_, mmgpu_sw_batch_t *b_, const uint32_t *pair_index_, uint32_t n_, mmgpu_sw_block *out_, char *bt_, const BlockWant &w)
        : c(c_), b(b_), pair_index(pair_index_), n(n_), out(out_), bt(bt_), want(w), s(c_->stream) {
        for (DevBuf *d : {&d_out, &d_sel_jobs, &d_sel_pairs, &d_sel_cnt, &d_flags, &d_btoff, &d_bt, &d_scores, &d_growth, &d_jobs[0], &d_jobs[1],
                          &d_jobs[2], &d_pool[0], &d_pool[1], &d_pool[2], &d_busy[0], &d_busy[1], &d_busy[2]})
            d->bind(c->cache);
        for (PassBufs &x : PB) { x.j2.bind(c->cache); x.cnt.bind(c->cache); x.pool.bind(c->cache); x.ck.bind(c->cache); }
    }
    static bool trace_on() {
        static const bool on = getenv("MMGPU_TRACE") != nullptr;
        return on;
    }
    void lap(const char *what);
    int select_jobs();
    int list_jobs();
    int score_table();
    int buffers_and_uploads();
    int block4_launch(PassBufs &B, const std::vector<BlockJob> &todo, int form, uint64_t per_res, uint64_t margin, uint64_t waves_per_cu,
                      std::vector<BlockJob> &left);
    int block4_collect(PassBufs &B, std::vector<BlockJob> &left);
    int block4_passes();
    int tier_rounds();
    int scatter_answers();
    int download_strings();
};

void BlockRun::lap(const char *what) {
    if (!trace_on()) return;
    const double t = prep_now();
    fprintf(stderr, "[mmgpu block aligner] %s %.3f s\n", what, t - t_mark);
    t_mark = t;
}

// the device picks the pairs (block_select.hip): int16-range hits that pass the query's start-score threshold
int BlockRun::select_jobs() {
    if (!b->d_qout_off.p) {
        HIP_TRY(b->d_qout_off.alloc(b->h_qout_off.size() * 4));
        HIP_TRY(hipMemcpyAsync(b->d_qout_off.p, b->h_qout_off.data(), b->h_qout_off.size() * 4, hipMemcpyHostToDevice, s));
    }
    if (!b->from_pf && !b->d_out_target.p) {
        HIP_TRY(b->d_out_target.alloc(std::max<size_t>(b->h_out_target.size(), 1) * 4));
        HIP_TRY(hipMemcpyAsync(b->d_out_target.p, b->h_out_target.data(), b->h_out_target.size() * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(d_sel_cnt.alloc(32));
    HIP_TRY(hipMemsetAsync(d_sel_cnt.p, 0, 32, s));
    BlockSelectArgs A;
    A.res = b->d_out.as<mmgpu_sw_hit>();
    A.pairs = (uint32_t)b->pairs;
    A.qout_off = b->d_qout_off.as<uint32_t>();
    A.n_queries = (uint32_t)(b->h_qout_off.size() - 1);
    A.q_minstart = b->d_qminstart.as<int32_t>();
    A.slot_target = b->from_pf ? b->d_slot_target.as<uint32_t>() : b->d_out_target.as<uint32_t>();
    A.jobs = nullptr; A.pair_of_slot = nullptr; A.blk = nullptr;
    A.count = d_sel_cnt.as<uint32_t>();
    A.cap = 0;      // first pass: count only
    HIP_TRY(launch_block_select(A, s));
    uint32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, d_sel_cnt.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    n = cnt;
    want.select->selected = n;
    if (n == 0) return MMGPU_OK;
    HIP_TRY(d_sel_jobs.alloc((size_t)n * sizeof(BlockJob)));
    HIP_TRY(d_sel_pairs.alloc((size_t)n * 4));
    HIP_TRY(d_out.alloc((size_t)n * sizeof(mmgpu_sw_block)));
    HIP_TRY(hipMemsetAsync(d_sel_cnt.p, 0, 4, s));
    A.jobs = d_sel_jobs.as<BlockJob>();
    A.pair_of_slot = d_sel_pairs.as<uint32_t>();
    A.blk = d_out.as<mmgpu_sw_block>();
    A.cap = n;
    HIP_TRY(launch_block_select(A, s));
    jobs.resize(n);
    // the selected jobs come back once and all n answers after every launch (block4_collect): through pinned memory where the
    // context's staging arena can be had for the length of this call (mmgpu_ctx::pinned; a thread preparing the next batch of
    // the context meanwhile then uploads from pageable memory, as this call copies to it when that thread holds the arena) -
    // the copies of pageable memory were ~5 ms of a 45 ms call
    const size_t out_bytes = (size_t)n * sizeof(mmgpu_sw_block), jobs_bytes = (size_t)n * sizeof(BlockJob);
    const size_t pin_need = upload_pinned_need(out_bytes) + upload_pinned_need(jobs_bytes);
    void *pin = pinned.acquire(c, pin_need);
    if (pin) {
        BlockJob *pj = reinterpret_cast<BlockJob *>(static_cast<char *>(pin) + upload_pinned_need(out_bytes));
        HIP_TRY(hipMemcpyAsync(pj, d_sel_jobs.p, jobs_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(jobs.data(), pj, jobs_bytes);
        out = static_cast<mmgpu_sw_block *>(pin);
    } else {
        HIP_TRY(hipMemcpyAsync(jobs.data(), d_sel_jobs.p, jobs_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        out_auto.resize(n);
        out = out_auto.data();
    }
    // (string offsets as in the other form: block_kernel.hip - profile queries, pairs beyond the pool - walks back whatever is asked)
    bt_off.assign(n, 0);
    for (const BlockJob &j : jobs) {
        bt_off[j.slot] = off;
        off += (block_pair_len(j) + 1 + 3) & ~3ull;
    }
    lap("device selection + job download");
    return MMGPU_OK;
}

// the caller names the pairs: what is no int16-range hit is answered here (MMGPU_BLOCK_NOT_WORD), the others become jobs
int BlockRun::list_jobs() {
    if (int e = sw_host_results(b, s)) return e;
    bt_off.assign(std::max<uint32_t>(n, 1), 0);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t p = pair_index[k];
        if (p >= b->pairs) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_backtrace: pair index out of range");
        const mmgpu_sw_hit &h = b->h_res[p];
        out[k].q_start = -1; out[k].t_start = -1; out[k].ident = 0; out[k].bt_len = 0; out[k].bt_off = off; out[k].reserved = 0;
        bt_off[k] = off;
        const uint32_t q = (uint32_t)(std::upper_bound(b->h_qout_off.begin(), b->h_qout_off.end(), p) - b->h_qout_off.begin() - 1);
        // (profile queries run the same kernel with the query's score rows in place of matrix + bias: block_kernel.hip, BkSeq::prof)
        if (h.score <= 0 || h.word != 1 || h.t_end < 0) {
            out[k].status = MMGPU_BLOCK_NOT_WORD;
            continue;
        }
        out[k].status = MMGPU_BLOCK_TOO_LARGE;    // overwritten by the kernel
        BlockJob j;
        j.query = q;
        j.target = b->from_pf ? b->h_slot_target[p] : b->h_out_target[p];
        j.score = h.score; j.q_end = h.q_end; j.t_end = h.t_end;
        j.slot = k;
        jobs.push_back(j);
        off += (block_pair_len(j) + 1 + 3) & ~3ull;      // (multiples of four: the walk kernel of block4_kernel.hip stores a string in dwords)
    }
    lap("result download + job list");
    return MMGPU_OK;
}

// the AAMatrix as ssw_init leaves it: new_simple(1, -1) with the substitution matrix written over it (:708,:1469-1474)
int BlockRun::score_table() {
    std::vector<int8_t> mat((size_t)b->alphabet * b->alphabet);
    scores.assign(27 * 32, (int8_t)-128);
    HIP_TRY(hipMemcpy(mat.data(), b->d_mat.p, mat.size(), hipMemcpyDeviceToHost));
    for (int x = 0; x < 26; x++)
        for (int y = 0; y < 26; y++) scores[x * 32 + y] = x == y ? 1 : -1;
    for (int x = 0; x < b->alphabet; x++)
        for (int y = 0; y < b->alphabet; y++) { scores[x * 32 + y] = mat[(size_t)x * b->alphabet + y]; scores[y * 32 + x] = mat[(size_t)x * b->alphabet + y]; }
    return MMGPU_OK;
}

// the answers, string offsets, strings and score table on the device; what every launch of the call has in common (L)
int BlockRun::buffers_and_uploads() {
    if (!want.select) HIP_TRY(d_out.alloc((size_t)n * sizeof(mmgpu_sw_block)));
    growth_bytes = want.growth ? (size_t)n * (1 + 4 * (size_t)want.growth_cap) * 4 : 0;
    if (want.growth) {
        HIP_TRY(d_growth.alloc(growth_bytes));
        HIP_TRY(hipMemsetAsync(d_growth.p, 0, growth_bytes, s));
    }
    HIP_TRY(d_btoff.alloc(bt_off.size() * 8));
    HIP_TRY(d_bt.alloc((size_t)off + 16));
    HIP_TRY(d_scores.alloc(scores.size()));
    if (!want.select) HIP_TRY(hipMemcpyAsync(d_out.p, out, (size_t)n * sizeof(mmgpu_sw_block), hipMemcpyHostToDevice, s));      // (select: block_select_kernel wrote them)
    HIP_TRY(hipMemcpyAsync(d_btoff.p, bt_off.data(), bt_off.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_scores.p, scores.data(), scores.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    lap("buffers + uploads");
    L.q_res = b->d_qres.as<uint8_t>();
    L.q_cb = b->d_qcb.as<int8_t>();
    L.q_off = b->d_qoff.as<uint32_t>();
    const TargetView T = sw_targets(c, b);
    L.t_res = T.res;
    L.t_off4 = T.off4;
    L.scores = d_scores.as<int8_t>();
    L.q_prof = b->any_profile ? b->d_qprof.as<int8_t>() : nullptr;
    L.q_prof_off = b->any_profile ? b->d_qprof_off.as<uint32_t>() : nullptr;
    L.alphabet = b->alphabet;
    L.gap_open = -b->gap_open;
    L.gap_extend = -b->gap_extend;
    L.out = d_out.as<mmgpu_sw_block>();
    L.bt_off = d_btoff.as<uint64_t>();
    L.bt = d_bt.as<char>();
    L.growth = want.growth ? d_growth.as<uint32_t>() : nullptr;
    L.growth_cap = want.growth_cap;
    b->block_pairs_tier[0] = b->block_pairs_tier[1] = b->block_pairs_tier[2] = 0;
    b->block_pairs_fast = 0;
    b->block_pairs_skew = 0;
    return MMGPU_OK;
}

// one launch: `todo` (longest first) through form 1 (four pairs per wavefront, 256 rows) or 3 (skewed, one pair per wavefront,
// 4096 rows), slots of `per_res` trace bytes per residue of the pair; pairs whose slot would not fit the pool go to `left`.  With a
// trace the pairs run in groups whose block lists + traces fit the pool, each group = fill launch + walk launch on the pass's stream
int BlockRun::block4_launch(PassBufs &B, const std::vector<BlockJob> &todo, int form, uint64_t per_res, uint64_t margin, uint64_t waves_per_cu,
                            std::vector<BlockJob> &left) {
    block4_plan(todo, resume, per_res, margin, BLOCK4_POOL_LIMIT, want.starts_only, B.plan, left);
    const std::vector<Block2Job> &j2 = B.plan.jobs;
    if (j2.empty()) return MMGPU_OK;
    const size_t n_groups = B.plan.n_groups();
    const int rows = form == 1 ? BLOCK4_LARGE_SIZE : BLOCK_REF_MAX_SIZE;
    if (j2.size() * sizeof(Block2Job) > B.j2.bytes) HIP_TRY(B.j2.alloc(j2.size() * sizeof(Block2Job)));
    if (n_groups * 4 > B.cnt.bytes) HIP_TRY(B.cnt.alloc(n_groups * 4));
    if (B.plan.pool_need > B.pool.bytes) HIP_TRY(B.pool.alloc((size_t)B.plan.pool_need));
    HIP_TRY(hipMemcpyAsync(B.j2.p, j2.data(), j2.size() * sizeof(Block2Job), hipMemcpyHostToDevice, B.st));
    HIP_TRY(hipMemsetAsync(B.cnt.p, 0, n_groups * 4, B.st));
    Block2Launch L2;
    L2.q_res = L.q_res; L2.q_cb = L.q_cb; L2.q_off = L.q_off; L2.t_res = L.t_res; L2.t_off4 = L.t_off4;
    L2.scores = L.scores; L2.gap_open = L.gap_open; L2.gap_extend = L.gap_extend;
    L2.out = L.out; L2.bt_off = L.bt_off; L2.bt = want.no_strings ? nullptr : L.bt;
    L2.pool = B.pool.as<uint8_t>();
    L2.growth = L.growth; L2.growth_cap = L.growth_cap;
    L2.trace_bytes = form == 1 ? 0u : 1u;
    for (size_t g = 0; g < n_groups; g++) {
        L2.jobs = B.j2.as<Block2Job>() + B.plan.group_begin[g];
        L2.n_jobs = B.plan.group_begin[g + 1] - B.plan.group_begin[g];
        L2.counter = B.cnt.as<uint32_t>() + g;
        const uint32_t waves = (uint32_t)std::min<uint64_t>(form == 1 ? (L2.n_jobs + 3) / 4 : L2.n_jobs, (uint64_t)std::max(c->compute_units, 1) * waves_per_cu);
        const size_t ck_bytes = (size_t)waves * (form == 1 ? 4 : 1) * 8 * (size_t)rows;
        if (ck_bytes > B.ck.bytes) HIP_TRY(B.ck.alloc(ck_bytes));
        L2.ck_pool = B.ck.as<uint8_t>();
        HIP_TRY(launch_sw_block4(L2, !want.starts_only, form, waves, B.st));
        if (!want.starts_only) HIP_TRY(launch_sw_block4_walk(L2, B.st));
    }
    if (trace_on()) fprintf(stderr, "[mmgpu block aligner] %s, blocks <= %d rows, %llu trace bytes per residue: %zu pairs in %zu group(s), pool %.1f MB\n",
                            form == 1 ? "four pairs per wavefront" : "one pair per wavefront, rows skewed over columns", rows, (unsigned long long)per_res,
                            j2.size(), n_groups, B.plan.pool_need / 1048576.0);
    return MMGPU_OK;
}

// ... and its end: the answers; what it handed on (MMGPU_BLOCK_TOO_LARGE) is appended to `left`
int BlockRun::block4_collect(PassBufs &B, std::vector<BlockJob> &left) {
    std::vector<Block2Job> &j2 = B.plan.jobs;
    if (j2.empty()) return MMGPU_OK;
    HIP_TRY(hipStreamSynchronize(B.st));
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * sizeof(mmgpu_sw_block), hipMemcpyDeviceToHost));
    for (const Block2Job &x : j2)
        if (out[x.slot].status == MMGPU_BLOCK_TOO_LARGE) {
            BlockJob j;
            j.query = x.query; j.target = x.target; j.score = x.score; j.q_end = x.q_end; j.t_end = x.t_end; j.slot = x.slot;
            const uint32_t rs = (uint32_t)out[x.slot].reserved;
            resume[x.slot] = std::max(32u, std::min(rs & 0xFFFFu, (uint32_t)BLOCK_REF_MAX_SIZE)) | (rs & 0x10000u);
            left.push_back(j);
        }
    if (trace_on()) {      // where in the (longest-first) launch the handed-on pairs stood
        size_t by_16th[16] = {};
        for (size_t k = 0; k < j2.size(); k++)
            if (out[j2[k].slot].status == MMGPU_BLOCK_TOO_LARGE) by_16th[k * 16 / j2.size()]++;
        fprintf(stderr, "[mmgpu block aligner] handed on, by sixteenth of the launch's %zu pairs:", j2.size());
        for (size_t z : by_16th) fprintf(stderr, " %zu", z);
        fprintf(stderr, "\n");
    }
    j2.clear();
    return MMGPU_OK;
}

// block4_kernel.hip: sequence queries.  Launch 1: four pairs per wavefront, blocks up to 256 rows.  What it answers TOO_LARGE (blocks
// would grow further, or the trace overflowed the pair's slot) goes through the skewed form - one pair per wavefront, its rows
// pipelined over the columns - with blocks up to 1024 rows, then the crate's 4096; each launch starts at the minimum block size the
// one before got to (mmgpu_sw_block::reserved of a TOO_LARGE answer).
int BlockRun::block4_passes() {
    constexpr uint64_t block4_waves = 16;        // wavefronts per CU
    constexpr uint64_t block4_per_res = 48;      // trace bytes per residue of a pair, launch 1
    resume.assign((size_t)n, 0u);
    PB[0].st = s;
    std::vector<BlockJob> seq_jobs, head, rest, handed, again, skew, skew_again;
    for (const BlockJob &j : jobs) {      // (`jobs` is sorted longest first)
        if (!b->h_query_is_profile.empty() && b->h_query_is_profile[j.query]) slow_jobs.push_back(j);
        else seq_jobs.push_back(j);
    }
    const size_t before = slow_jobs.size();
    // the head launch (block_head_size): the longest pairs in the skewed form, on a stream and with buffers of their own
    const size_t n_head = block_head_size(seq_jobs.size(), c->compute_units);
    head.assign(seq_jobs.begin(), seq_jobs.begin() + n_head);
    rest.assign(seq_jobs.begin() + n_head, seq_jobs.end());
    if (n_head) {
        if (head_stream.create() != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_sw_block_backtrace: hipStreamCreate");
        PB[1].st = head_stream.s;
        HIP_TRY(hipStreamSynchronize(s));      // (the uploads of buffers_and_uploads)
        if (int e = block4_launch(PB[1], head, 3, 1024, 2048, 4, skew_again)) return e;
    }
    // launch 1: everything else, slots for the usual 32 / 64-row blocks (half a byte per cell).  Resident wavefronts by LDS: 3.4 KB of
    // score table + 8 KB (four pairs' border arrays); the skewed form's 32 KB allow four
    // (Measured and dropped in round 6: launch 1 cut in two - the longest eighth of the pairs first, so that its hand-ons could start
    // their chains in the skewed form beside the other seven eighths.  500 of the 536 hand-ons of configs[2] do come from that
    // eighth, but it takes 15 ms of its own - the longest pairs - and the 500 chains another 25: 44.7 ms per call against 43.5.
    // The call is as long as ONE pair's chain through blocks of thousands of rows on one wavefront.)
    if (int e = block4_launch(PB[0], rest, 1, block4_per_res, 512, block4_waves, skew)) return e;
    if (int e = block4_collect(PB[0], handed)) return e;
    lap("four pairs per wavefront + status download");
    // ... once more for the pairs whose slot was too small (256-row blocks all the way: 128 bytes per residue)
    for (const BlockJob &j : handed) (resume[j.slot] & 0x10000u ? again : skew).push_back(j);
    if (!again.empty()) {
        block_longest_first(again);
        if (int e = block4_launch(PB[0], again, 1, 160, 2048, block4_waves, skew)) return e;
        if (int e = block4_collect(PB[0], skew)) return e;
        lap("four pairs per wavefront, larger slots + status download");
    }
    // launch 2: the skewed form for blocks beyond 256 rows (a byte per cell: slots for blocks of 1024 rows, then the crate's bound)
    block_longest_first(skew);
    if (int e = block4_launch(PB[0], skew, 3, 1024, 2048, 4, skew_again)) return e;
    if (int e = block4_collect(PB[0], skew_again)) return e;
    if (n_head)
        if (int e = block4_collect(PB[1], skew_again)) return e;
    if (!skew.empty() || n_head) lap("skewed form (and the head) + status download");
    const size_t n_skew = skew.size() + n_head;
    if (!skew_again.empty()) {
        block_longest_first(skew_again);
        if (int e = block4_launch(PB[0], skew_again, 3, 4096, 8192, 4, slow_jobs)) return e;
        if (int e = block4_collect(PB[0], slow_jobs)) return e;
        lap("skewed form, the crate's slots + status download");
    }
    block_longest_first(slow_jobs);
    b->block_pairs_skew = (uint32_t)(n_skew - (slow_jobs.size() - before));
    b->block_pairs_fast = (uint32_t)(seq_jobs.size() - n_skew);
    return MMGPU_OK;
}

// Three tiers (block_kernel.hip) for what is left - profile queries, pairs whose slot would not fit the pool - each a launch over
// what the one before left undecided (TOO_LARGE), all carved out of ONE scratch pool per tier (hipMalloc costs ~40 ms per GB on
// this platform, so the pool is sized for the usual case, not the worst):
//   tier 0  blocks <= 512 rows, borders in LDS; slot = block list + TWO trace entries (32 B per 64 rows) per column for the
//           256th-longest pair - nearly every pair stays at 32 / 64-row blocks; a pair that is longer or grows further
//           overflows its slot and moves on
//   tier 1  blocks <= 2048 rows in LDS, slot = the crate's own bound for that size (Trace::new, scan_block.rs:1742-1748)
//   tier 2  the crate's 4096 rows, borders in the slot
// The tiers of a round run side by side, the second and third on streams of their own.
int BlockRun::tier_rounds() {
    if (slow_jobs.empty()) return MMGPU_OK;
    const int first_tier = first_tier_env ? std::max(0, std::min(2, atoi(first_tier_env))) : 0;
    const uint64_t tier0_entries = first_tier_env ? 2 : BLOCK_MAX_SIZE / 64;
    // (small calls: slots for the longest pair, everything starts in tier 0)
    const uint64_t typical_len = block_pair_len(slow_jobs[slow_jobs.size() > 1024 ? 255 : 0]);
    std::vector<BlockJob> wait[3];      // longest first inside each
    for (const BlockJob &j : slow_jobs) wait[first_tier == 0 && block_pair_len(j) > typical_len ? 1 : first_tier].push_back(j);
    while (!wait[0].empty() || !wait[1].empty() || !wait[2].empty()) {
        int n_launched = 0;
        for (int tier = 2; tier >= 0; tier--) {      // (the long chains first)
            std::vector<BlockJob> &todo = wait[tier];
            if (todo.empty()) continue;
            const uint64_t longest_todo = block_pair_len(todo.front());
            const uint64_t slot_bytes = tier == 0   ? block_tier_slot_bytes(typical_len, tier0_entries, BLOCK_MAX_SIZE, false)
                                        : tier == 1 ? block_tier_slot_bytes(longest_todo, BLOCK_MID_SIZE / 64, BLOCK_MID_SIZE, false)
                                                    : block_tier_slot_bytes(longest_todo, BLOCK_REF_MAX_SIZE / 64, BLOCK_REF_MAX_SIZE, true);
            // (tier 0: 16 wavefronts per CU is what its 9 KB of LDS allows; 8 per CU, or 32 with a 128-row first tier, move the call by
            // +12 % / -3 %, profiles/r04_exp_block_occupancy.txt - the kernel is bound by its ~200 instructions per column, not by latency)
            const uint32_t slots = block_tier_slots(todo.size(), c->compute_units, tier == 0 ? 16 : 4, slot_bytes);
            hipStream_t st = s;
            if (n_launched > 0) {
                if (extra[n_launched - 1].create() != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_sw_block_backtrace: hipStreamCreate");
                st = extra[n_launched - 1].s;
            }
            if ((size_t)slot_bytes * slots > d_pool[tier].bytes) HIP_TRY(d_pool[tier].alloc((size_t)slot_bytes * slots));
            if ((size_t)slots * 4 > d_busy[tier].bytes) HIP_TRY(d_busy[tier].alloc((size_t)slots * 4));
            if (todo.size() * sizeof(BlockJob) > d_jobs[tier].bytes) HIP_TRY(d_jobs[tier].alloc(todo.size() * sizeof(BlockJob)));
            HIP_TRY(hipMemsetAsync(d_busy[tier].p, 0, (size_t)slots * 4, st));
            HIP_TRY(hipMemcpyAsync(d_jobs[tier].p, todo.data(), todo.size() * sizeof(BlockJob), hipMemcpyHostToDevice, st));
            L.jobs = d_jobs[tier].as<BlockJob>();
            L.n_jobs = (uint32_t)todo.size();
            L.pool = d_pool[tier].as<uint8_t>();
            L.slot_bytes = slot_bytes;
            L.n_pool_slots = slots;
            L.pool_busy = d_busy[tier].as<uint32_t>();
            HIP_TRY(launch_sw_block(L, tier, st));
            if (trace_on()) fprintf(stderr, "[mmgpu block aligner] tier %d: %zu pairs, %u slots of %.1f KB\n", tier, todo.size(), slots, slot_bytes / 1024.0);
            n_launched++;
        }
        for (const SideStream &x : extra)
            if (x.s) HIP_TRY(hipStreamSynchronize(x.s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * sizeof(mmgpu_sw_block), hipMemcpyDeviceToHost));
        std::vector<BlockJob> next[3];
        for (int tier = 0; tier < 3; tier++) {
            size_t left = 0;
            for (const BlockJob &j : wait[tier])
                if (out[j.slot].status == MMGPU_BLOCK_TOO_LARGE && tier < 2) { next[tier + 1].push_back(j); left++; }
            b->block_pairs_tier[tier] += (uint32_t)(wait[tier].size() - left);
        }
        for (int tier = 0; tier < 3; tier++) {
            block_longest_first(next[tier]);
            wait[tier].swap(next[tier]);
        }
        lap("round of tier launches + status download");
    }
    return MMGPU_OK;
}

// mmgpu_sw_block_starts: the answers into the batch's records; what the block aligner declined gets its reverse scan (:873-882)
int BlockRun::scatter_answers() {
    HIP_TRY(d_flags.alloc((size_t)b->pairs));
    HIP_TRY(hipMemsetAsync(d_flags.p, 0, (size_t)b->pairs, s));
    HIP_TRY(hipMemsetAsync(d_sel_cnt.p, 0, 32, s));
    BlockScatterArgs S;
    S.blk = d_out.as<mmgpu_sw_block>();
    S.pair_of_slot = d_sel_pairs.as<uint32_t>();
    S.n = n;
    S.res = b->d_out.as<mmgpu_sw_hit>();
    S.rev_force = d_flags.as<uint8_t>();
    S.counts = d_sel_cnt.as<uint32_t>();
    HIP_TRY(launch_block_scatter(S, s));
    uint32_t counts[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(counts, d_sel_cnt.p, 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    want.select->ok = counts[0]; want.select->declined = counts[1]; want.select->too_large = counts[2];
    if (counts[1]) {
        if (int e = sw_launch_groups(c, b, true, d_flags.as<uint8_t>())) return e;
        HIP_TRY(hipStreamSynchronize(s));
    }
    b->h_res_valid = false;
    lap("answers scattered into the records (+ reverse scan of declined pairs)");
    return MMGPU_OK;
}

int BlockRun::download_strings() {
    if (off && !want.no_strings) HIP_TRY(hipMemcpyAsync(bt, d_bt.p, (size_t)off, hipMemcpyDeviceToHost, s));
    if (want.growth) HIP_TRY(hipMemcpyAsync(want.growth, d_growth.p, growth_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));      // the host vectors and the buffers of the call die with it
    lap("backtrace strings download");
    return MMGPU_OK;
}

}  // namespace

static int block_backtrace(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const uint32_t *pair_index, uint32_t n, mmgpu_sw_block *out,
                           char *bt, size_t bt_cap, size_t *bt_used, const BlockWant &want) {
    if (!c || !b || (!want.select && ((!pair_index && n) || (!out && n)))) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_backtrace: NULL argument");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_block_backtrace: batch was never run");
    if (b->alphabet > 26) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_block_backtrace: alphabet above 26 letters");
    HIP_TRY(hipSetDevice(c->device));
    if (b->mode < MMGPU_SW_START && !b->from_pf && b->h_out_target.empty())
        return fail(MMGPU_ERR_STATE, "mmgpu_sw_block_backtrace: the batch keeps no slot -> target map (prepare it with MMGPU_SW_START)");
    BlockRun R(c, b, pair_index, n, out, bt, want);
    if (int e = want.select ? R.select_jobs() : R.list_jobs()) return e;
    if (bt_used) *bt_used = (size_t)R.off;
    if (!want.no_strings && (R.off > bt_cap || (!bt && R.off))) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_backtrace: bt buffer too small (see *bt_used)");
    if (R.jobs.empty()) return MMGPU_OK;
    block_longest_first(R.jobs);
    if (int e = R.score_table()) return e;
    if (int e = R.buffers_and_uploads()) return e;
    if (R.first_tier_env) R.slow_jobs = R.jobs;
    else if (int e = R.block4_passes()) return e;
    if (int e = R.tier_rounds()) return e;
    return want.select ? R.scatter_answers() : R.download_strings();
}


// One call = what `mmseqs search` needs of the block aligner in alignment mode 2 without backtraces: the device picks every int16-range
// hit that passes its query's start-score threshold, runs the block aligner for start positions only, writes them into the batch's
// records and scans backwards for the pairs it declined.  Afterwards mmgpu_sw_fetch returns records whose start positions are the
// reference's for every pair that passes the gate, whichever path they took.
extern "C" int mmgpu_sw_block_starts(mmgpu_ctx *c, mmgpu_sw_batch_t *b, uint32_t *n_selected, uint32_t *n_declined, uint32_t *n_too_large) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_starts: NULL argument");
    if (b->mode != MMGPU_SW_START_NOT_WORD) return fail(MMGPU_ERR_STATE, "mmgpu_sw_block_starts: the batch was not prepared with MMGPU_SW_START_NOT_WORD");
    if (b->owned) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_sw_block_starts: not for batches of owned pairs (sharded runs)");
    BlockAuto au;
    BlockWant want;
    want.select = &au;
    want.starts_only = want.no_strings = true;
    const int rc = block_backtrace(c, b, nullptr, 0, nullptr, nullptr, 0, nullptr, want);
    if (n_selected) *n_selected = au.selected;
    if (n_declined) *n_declined = au.declined;
    if (n_too_large) *n_too_large = au.too_large;
    return rc;
}

extern "C" int mmgpu_sw_block_backtrace(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const uint32_t *pair_index, uint32_t n, mmgpu_sw_block *out,
                                        char *bt, size_t bt_cap, size_t *bt_used) {
    BlockWant want;
    want.starts_only = bt == nullptr && bt_cap == MMGPU_BLOCK_STARTS_ONLY;
    want.no_strings = want.starts_only || (bt == nullptr && bt_cap == MMGPU_BLOCK_NO_STRINGS);
    return block_backtrace(c, b, pair_index, n, out, bt, bt_cap, bt_used, want);
}

extern "C" int mmgpu_sw_block_growth(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const uint32_t *pair_index, uint32_t n, mmgpu_sw_block *out,
                                     uint32_t *growth, uint32_t growth_cap) {
    if (!growth || growth_cap == 0) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_growth: no buffer");
    BlockWant want;
    want.no_strings = true;
    want.growth = growth;
    want.growth_cap = growth_cap;
    return block_backtrace(c, b, pair_index, n, out, nullptr, 0, nullptr, want);
}

extern "C" int mmgpu_sw_block_tiers(const mmgpu_sw_batch_t *b, uint32_t *first_tier, uint32_t *second_tier) {
    if (!b) return fail(MMGPU_ERR_ARG, "mmgpu_sw_block_tiers: NULL batch");
    if (first_tier) *first_tier = b->block_pairs_fast + b->block_pairs_tier[0];
    if (second_tier) *second_tier = b->block_pairs_skew + b->block_pairs_tier[1] + b->block_pairs_tier[2];
    return MMGPU_OK;
}

extern "C" int mmgpu_sw_traceback(mmgpu_ctx *c, mmgpu_sw_batch_t *b, const uint32_t *pair_index, uint32_t n, mmgpu_sw_bt *info,
                                  char *bt, size_t bt_cap, size_t *bt_used) {
    if (!c || !b || (!pair_index && n) || (!info && n)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_traceback: NULL argument");
    if (b->mode < MMGPU_SW_START) return fail(MMGPU_ERR_STATE, "mmgpu_sw_traceback: the batch was prepared without MMGPU_SW_START");
    if (!b->ran) return fail(MMGPU_ERR_STATE, "mmgpu_sw_traceback: batch was never run");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (int e = sw_host_results(b, s)) return e;      // (callers ask for the size first and for the strings second)
    const std::vector<mmgpu_sw_hit> &res = b->h_res;
    const std::vector<uint32_t> &pf_host = b->h_slot_target;
    std::vector<BtJob> jobs;
    jobs.reserve(n);
    uint64_t off = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t p = pair_index[k];
        if (p >= b->pairs) return fail(MMGPU_ERR_ARG, "mmgpu_sw_traceback: pair index out of range");
        const mmgpu_sw_hit &h = res[p];
        info[k].bt_off = off;
        info[k].bt_len = 0;
        info[k].ident = 0;
        info[k].reserved = 0;
        if (h.score <= 0 || h.q_start < 0 || h.t_start < 0 || h.q_end < h.q_start || h.t_end < h.t_start) {
            info[k].status = MMGPU_BT_NO_START;
            continue;
        }
        info[k].status = MMGPU_BT_TOO_LARGE;   // overwritten by the kernel
        BtJob j;
        j.slot = k;
        j.query = (uint32_t)(std::upper_bound(b->h_qout_off.begin(), b->h_qout_off.end(), p) - b->h_qout_off.begin() - 1);
        j.target = b->from_pf ? pf_host[p] : b->h_out_target[p];
        j.q_start = h.q_start; j.q_end = h.q_end; j.t_start = h.t_start; j.t_end = h.t_end; j.score = h.score;
        j.bt_off = off;
        off += (uint64_t)(h.q_end - h.q_start + 1) + (uint64_t)(h.t_end - h.t_start + 1) + 1;
        jobs.push_back(j);
    }
    if (bt_used) *bt_used = (size_t)off;
    if (off > bt_cap || (!bt && off)) return fail(MMGPU_ERR_ARG, "mmgpu_sw_traceback: bt buffer too small (see *bt_used)");
    if (jobs.empty()) return MMGPU_OK;
    auto cost = [](const BtJob &j) {
        const int64_t ql = j.q_end - j.q_start + 1, tl = j.t_end - j.t_start + 1;
        return ql * (2 * (std::llabs(tl - ql) + 1) + 1);
    };
    std::stable_sort(jobs.begin(), jobs.end(), [&](const BtJob &x, const BtJob &y) { return cost(x) > cost(y); });
    HIP_TRY(b->d_bt_jobs.reserve(jobs.size() * sizeof(BtJob)));
    HIP_TRY(b->d_bt_info.reserve((size_t)n * sizeof(mmgpu_sw_bt)));
    HIP_TRY(b->d_bt_str.reserve((size_t)off + 16));
    HIP_TRY(hipMemcpyAsync(b->d_bt_info.p, info, (size_t)n * sizeof(mmgpu_sw_bt), hipMemcpyHostToDevice, s));
    BtLaunch L;
    L.q_res = b->d_qres.as<uint8_t>();
    L.q_cb = b->d_qcb.as<int8_t>();
    L.q_off = b->d_qoff.as<uint32_t>();
    L.q_prof = b->any_profile ? b->d_qprof.as<int8_t>() : nullptr;
    L.q_prof_off = b->any_profile ? b->d_qprof_off.as<uint32_t>() : nullptr;
    const TargetView T = sw_targets(c, b);
    L.t_res = T.res;
    L.t_off4 = T.off4;
    L.mat = b->d_mat.as<int8_t>();
    L.alphabet = b->alphabet;
    L.gap_open = b->gap_open;
    L.gap_extend = b->gap_extend;
    L.info = b->d_bt_info.as<mmgpu_sw_bt>();
    L.bt = b->d_bt_str.as<char>();
    // Scratch tiers (band rows | direction words per lane | blocks of 64 alignments in flight):
    //   0: rows in LDS (band <= 32),     8 K words (64 K cells)  - nearly every pair of a hit list
    //   1: rows in LDS (band <= 32),   128 K words (1 M cells)   - long alignments with a narrow band
    //   2: rows in scratch (band <= 256), 128 K words
    //   3: rows in scratch (band <= 4096),  1 M words (8 M cells), few at a time; beyond: MMGPU_BT_TOO_LARGE, the host runs banded_sw
    // A job starts at the first tier its initial band (|tlen - qlen| + 1) fits and moves up when the doubling outgrows it.
    // band 0 in BtLaunch selects the LDS form of the kernel.
    const int n_tiers = 4;
    const uint32_t tier_band[n_tiers] = {0u, 0u, 515u, 8195u}, tier_dir[n_tiers] = {8192u, 131072u, 131072u, 1048576u};
    const uint32_t tier_blocks[n_tiers] = {16384u, 256u, 256u, 48u};
    auto first_tier = [&](const BtJob &j) {
        const int64_t ql = j.q_end - j.q_start + 1, tl = j.t_end - j.t_start + 1;
        const int64_t bw = std::llabs(tl - ql) + 1, width = 2 * bw + 3, words = (2 * bw + 1 + 7) / 8 * ql;
        for (int t = 0; t < n_tiers; t++) {
            const int64_t cap = tier_band[t] ? (int64_t)tier_band[t] : 67;
            if (width <= cap && words <= (int64_t)tier_dir[t]) return t;
        }
        return n_tiers - 1;
    };
    std::vector<mmgpu_sw_bt> back((size_t)n);
    std::vector<BtJob> pending = jobs, now;
    const bool trace = getenv("MMGPU_TRACE") != nullptr;
    L.dir_pool = nullptr;
    L.dir_pool_bytes = 0;
    L.dir_cursor = nullptr;
    static const bool lane_kernel_only = getenv("MMGPU_BT_LANE_KERNEL") != nullptr;   // cross-check switch: skip the wave kernel
    if (!lane_kernel_only) {
        // ---- the wave kernel takes every job first (bt_wave_kernel.hip); what it declines (band beyond its LDS ring,
        // direction pool exhausted) goes through the tiers of the lane-per-alignment kernel below
        uint64_t want = 0;
        for (const BtJob &j : jobs) {
            const uint64_t ql = (uint64_t)(j.q_end - j.q_start + 1), tl = (uint64_t)(j.t_end - j.t_start + 1);
            const uint64_t bw0 = (ql > tl ? ql - tl : tl - ql) + 1;
            want += ql * (2 * std::min<uint64_t>(4 * bw0, 510) + 1);
        }
        const uint64_t pool = std::min<uint64_t>(std::max<uint64_t>(want, 64ull << 20), 8ull << 30);
        HIP_TRY(b->d_bt_scratch.reserve(pool + 16));
        HIP_TRY(b->d_bt_cursor.reserve(16));
        HIP_TRY(hipMemsetAsync(b->d_bt_cursor.p, 0, 16, s));
        HIP_TRY(hipMemcpyAsync(b->d_bt_jobs.p, jobs.data(), jobs.size() * sizeof(BtJob), hipMemcpyHostToDevice, s));
        L.dir_pool = b->d_bt_scratch.as<uint8_t>();
        L.dir_pool_bytes = pool;
        L.dir_cursor = b->d_bt_cursor.as<unsigned long long>();
        L.jobs = b->d_bt_jobs.as<BtJob>();
        L.n_jobs = (uint32_t)jobs.size();
        HIP_TRY(launch_sw_traceback_wave(L, s));
        HIP_TRY(hipMemcpyAsync(back.data(), b->d_bt_info.p, (size_t)n * sizeof(mmgpu_sw_bt), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        pending.clear();
        for (const BtJob &j : jobs)
            if (back[j.slot].status == MMGPU_BT_TOO_LARGE) pending.push_back(j);
        if (trace) {
            const auto t = std::chrono::steady_clock::now();
            fprintf(stderr, "[sw_traceback] wave kernel: %zu jobs, %zu declined, pool %.1f MB\n", jobs.size(), pending.size(), (double)pool / 1048576.0);
            (void)t;
        }
    }
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&]() {
        const auto t = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t - t_prev).count();
        t_prev = t;
        return ms;
    };
    if (trace) fprintf(stderr, "[sw_traceback] %u pairs asked, %zu with a start position\n", n, jobs.size());
    for (int tier = 0; tier < n_tiers && !pending.empty(); tier++) {
        now.clear();
        std::vector<BtJob> later;
        for (const BtJob &j : pending) (first_tier(j) <= tier ? now : later).push_back(j);
        if (now.empty()) continue;
        const uint32_t wpl = 3u * tier_band[tier] + tier_dir[tier];
        const size_t blocks_max = tier_blocks[tier];
        const size_t njobs = now.size();
        const size_t blocks_needed = std::min<size_t>((njobs + 63) / 64, blocks_max);
        HIP_TRY(b->d_bt_scratch.reserve(blocks_needed * (size_t)wpl * 64 * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(b->d_bt_jobs.p, now.data(), now.size() * sizeof(BtJob), hipMemcpyHostToDevice, s));
        L.scratch = b->d_bt_scratch.as<uint32_t>();
        L.words_per_lane = wpl;
        L.band_cap = tier_band[tier];
        for (size_t j0 = 0; j0 < njobs; j0 += blocks_max * 64) {
            L.jobs = b->d_bt_jobs.as<BtJob>() + j0;
            L.n_jobs = (uint32_t)std::min<size_t>(njobs - j0, blocks_max * 64);
            HIP_TRY(launch_sw_traceback(L, s));
        }
        HIP_TRY(hipMemcpyAsync(back.data(), b->d_bt_info.p, (size_t)n * sizeof(mmgpu_sw_bt), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        size_t moved = 0;
        for (const BtJob &j : now)
            if (back[j.slot].status == MMGPU_BT_TOO_LARGE && tier + 1 < n_tiers) { later.push_back(j); moved++; }
        if (trace) fprintf(stderr, "[sw_traceback] tier %d: %zu jobs, %zu moved up, %.2f ms\n", tier, now.size(), moved, lap());
        pending.swap(later);
    }
    for (uint32_t k = 0; k < n; k++)
        if (info[k].status != MMGPU_BT_NO_START) info[k] = back[k];
    if (off) HIP_TRY(hipMemcpyAsync(bt, b->d_bt_str.p, (size_t)off, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (trace) fprintf(stderr, "[sw_traceback] strings downloaded (%.1f MB), %.2f ms\n", (double)off / 1048576.0, lap());
    return MMGPU_OK;
}
