// Host side of linclust's k-mer matching stage (include/mmgpu.h, "linclust's k-mer matching stage"): the refusals, the memory bound,
// the sequence of launches with the two radix sorts between them, the fetches.  run is a sequence of named steps over one record,
// in the manner of gscan_api.hip.
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "mmgpu_internal.h"

using namespace mmgpu;

namespace {

// computeKmerCount (kmermatcher.cpp:1100-1108): the reference's bound on the records of one split, per sequence
// min(max(1, L - k + 2), (int)(kmersPerSequence + scale * L))
uint64_t kmm_record_bound(const std::vector<uint32_t> &len, const mmgpu_kmermatch_params &p) {
    uint64_t total = 0;
    for (uint32_t l : len) {
        const int seq_len = (int)l;
        const int adjusted = std::max(1, seq_len - p.k + 2);
        total += (uint64_t)std::max(0, std::min(adjusted, static_cast<int>(p.kmers_per_seq + (p.kmers_per_seq_scale * seq_len))));
    }
    return total;
}

// the parameters alone: decided before the context is looked at (a caller may probe a parameter set without a device)
int kmm_check_params(const char *who, const mmgpu_kmermatch_params *p) {
    if (!p) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (p->k < 1 || p->k > KMM_MAX_K) return fail(MMGPU_ERR_ARG, std::string(who) + ": k must be 1 .. 32");
    if (p->alph_size < 3 || p->alph_size > 21) return fail(MMGPU_ERR_ARG, std::string(who) + ": alph_size must be 3 .. 21");
    if (p->kmers_per_seq < 1) return fail(MMGPU_ERR_ARG, std::string(who) + ": kmers_per_seq must be 1 or more");
    if (!(p->kmers_per_seq_scale >= 0.0f) || !std::isfinite(p->kmers_per_seq_scale)) return fail(MMGPU_ERR_ARG, std::string(who) + ": kmers_per_seq_scale must be 0 or more");
    for (int i = 0; i < 21; i++)
        if (p->reduce[i] >= p->alph_size) return fail(MMGPU_ERR_ARG, std::string(who) + ": reduce entry outside the reduced alphabet");
    if (p->cov_mode < 0 || p->cov_mode > 5) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": cov_mode outside 0 .. 5");
    long double power = 1.0L;      // (alph_size - 1)^k as Indexer's size_t powers hold it
    for (int i = 0; i < p->k; i++) power *= (long double)(p->alph_size - 1);
    if (power >= 9223372036854775808.0L) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": (alph_size - 1)^k is 2^63 or more: the k-mer index does not fit");
    return MMGPU_OK;
}

int kmm_check_db(const char *who, const mmgpu_ctx *c) {
    if (!c->db.res || c->db.n == 0) return fail(MMGPU_ERR_STATE, std::string(who) + ": no targets loaded");
    if (c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": the context holds a shard of a multi-GPU run");
    if (c->db.alphabet != 21) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": protein sequences only (nucleotide and profile databases are not matched on the device)");
    if (c->db.max_len > KMM_MAX_LEN)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": a sequence of 32 767 residues or more (the reference then keeps int positions; not built here)");
    return MMGPU_OK;
}

// bytes of device memory a run holds at its peak for `bound` records of n sequences: four uint64 and two uint32 arrays per record (keys
// and values of both sorts, each with its double; group starts and compaction offsets), two uint16 (the diagonals and their double),
// the result (at most one entry per sequence and per record), the per-sequence rule / count / offset, and rocprim's scratch, which is
// histograms and a few bytes per block - an eighth on top covers it
uint64_t kmm_bytes_needed(uint64_t bound, uint32_t n) {
    const uint64_t per_record = 4 * 8 + 2 * 4 + 2 * 2 + sizeof(mmgpu_pf_hit);
    const uint64_t per_seq = sizeof(uint4) + 2 * 4 + 8 + sizeof(mmgpu_pf_hit);
    const uint64_t sum = bound * per_record + (uint64_t)n * per_seq;
    return sum + sum / 8 + (64u << 20);
}

// records the buffers hold: the bound, and one per sequence on top (the bound adds kmersPerSequence to the float product where the
// extraction adds kmersPerSequence - 1 and then 1: the two roundings need not agree)
uint64_t kmm_capacity(const mmgpu_kmermatch_batch_t *b) { return b->bound + b->n; }

// everything a run allocates beside the result; the blocks go back to the context's cache when the run ends (it ends synchronised)
struct KmmRun {
    const char *who;                                  // the entry point, for the messages
    mmgpu_ctx *c;
    mmgpu_kmermatch_batch_t *b;
    hipStream_t s;
    DevBuf rule, count, rec_off, tile_sum;            // per sequence; scan scratch
    DevBuf a, bb, cc, dd;                             // four uint64 per record: keys and values of the sorts and their doubles
    DevBuf u1, u2;                                    // two uint32 per record (+ 1)
    DevBuf h1, h2;                                    // two uint16 per record
    DevBuf tmp;                                       // rocprim's
    uint32_t n_records = 0, n_pairs = 0, n_kept = 0;
};

int kmm_read_u32(KmmRun &R, const uint32_t *d, uint32_t *out) {
    HIP_TRY(hipMemcpyAsync(out, d, sizeof(uint32_t), hipMemcpyDeviceToHost, R.s));
    HIP_TRY(hipStreamSynchronize(R.s));
    return MMGPU_OK;
}

int kmm_alloc(KmmRun &R) {
    const uint32_t n = R.b->n;
    const uint64_t N = kmm_capacity(R.b);
    for (DevBuf *d : {&R.rule, &R.count, &R.rec_off, &R.tile_sum, &R.a, &R.bb, &R.cc, &R.dd, &R.u1, &R.u2, &R.h1, &R.h2, &R.tmp}) d->bind(R.c->cache);
    HIP_TRY(R.rule.alloc((size_t)n * sizeof(uint4)));
    HIP_TRY(R.count.alloc((size_t)n * 4));
    HIP_TRY(R.rec_off.alloc(((size_t)n + 1) * 4));
    HIP_TRY(R.tile_sum.alloc(((size_t)kmm_scan_tiles(std::max<uint64_t>(N, n)) + 1) * 4));
    for (DevBuf *d : {&R.a, &R.bb, &R.cc, &R.dd}) HIP_TRY(d->alloc((size_t)N * 8));
    for (DevBuf *d : {&R.u1, &R.u2}) HIP_TRY(d->alloc(((size_t)N + 1) * 4));
    for (DevBuf *d : {&R.h1, &R.h2}) HIP_TRY(d->alloc((size_t)N * 2));
    return MMGPU_OK;
}

// the record count of the extraction, between its two passes
int kmm_read_n_records(KmmRun &R) {
    const int rc = kmm_read_u32(R, R.rec_off.as<uint32_t>() + R.b->n, &R.n_records);
    if (rc != MMGPU_OK) return rc;
    if (R.n_records > kmm_capacity(R.b)) return fail(MMGPU_ERR_HIP, std::string(R.who) + ": more records than computeKmerCount bounds");      // (cannot happen)
    return MMGPU_OK;
}

// stage 1 over nucleotides: the same three steps with nuclmatch_kernel.hip's two passes, the sequences longest first
int kmm_extract_nucl(KmmRun &R) {
    mmgpu_ctx *c = R.c;
    const mmgpu_kmermatch_params &p = R.b->par;
    NuclExtractArgs A{};
    A.res = c->db.res;
    A.off4 = c->db.off4;
    A.len = c->db.len;
    A.order = R.b->d_order.as<uint32_t>();
    A.n = R.b->n;
    A.k = p.k;
    A.kmers_per_seq = p.kmers_per_seq;
    A.kmers_per_seq_scale = p.kmers_per_seq_scale;
    A.seed = (unsigned long long)(long long)p.hash_shift;
    A.rule = R.rule.as<uint4>();
    A.count = R.count.as<uint32_t>();
    A.rec_off = R.rec_off.as<uint32_t>();
    A.rec_kmer = R.cc.as<unsigned long long>();
    A.rec_val = R.a.as<unsigned long long>();
    HIP_TRY(launch_nuclmatch_extract_count(A, R.s));
    HIP_TRY(launch_kmm_record_offsets(A.count, A.n, R.tile_sum.as<uint32_t>(), R.rec_off.as<uint32_t>(), R.s));
    const int rc = kmm_read_n_records(R);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(launch_nuclmatch_extract_write(A, R.s));
    return MMGPU_OK;
}

// stage 1: count, offsets, write -> records (k-mer in cc, value in a), n_records
int kmm_extract(KmmRun &R) {
    if (R.b->nucl) return kmm_extract_nucl(R);
    mmgpu_ctx *c = R.c;
    const mmgpu_kmermatch_params &p = R.b->par;
    KmmExtractArgs A{};
    A.res = c->db.res;
    A.off4 = c->db.off4;
    A.len = c->db.len;
    A.n = R.b->n;
    A.k = p.k;
    A.alph_size = p.alph_size;
    for (int i = 0; i < 21; i++) A.reduce[i] = p.reduce[i];
    A.kmers_per_seq = p.kmers_per_seq;
    A.kmers_per_seq_scale = p.kmers_per_seq_scale;
    A.seed = (unsigned long long)(long long)p.hash_shift;
    A.rule = R.rule.as<uint4>();
    A.count = R.count.as<uint32_t>();
    A.rec_off = R.rec_off.as<uint32_t>();
    A.rec_kmer = R.cc.as<unsigned long long>();
    A.rec_val = R.a.as<unsigned long long>();
    HIP_TRY(launch_kmm_extract_count(A, R.s));
    HIP_TRY(launch_kmm_record_offsets(A.count, A.n, R.tile_sum.as<uint32_t>(), R.rec_off.as<uint32_t>(), R.s));
    const int rc = kmm_read_n_records(R);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(launch_kmm_extract_write(A, R.s));
    return MMGPU_OK;
}

int kmm_sort_pairs(KmmRun &R, const char *what, hipError_t (*call)(KmmRun &, void *, size_t &)) {
    size_t bytes = 0;
    hipError_t e = call(R, nullptr, bytes);
    if (e == hipSuccess) e = R.tmp.reserve(std::max<size_t>(bytes, 16));
    if (e == hipSuccess) e = call(R, R.tmp.p, bytes);
    if (e != hipSuccess) return fail(MMGPU_ERR_HIP, std::string(R.who) + ": " + what + ": " + hipGetErrorString(e));
    return MMGPU_OK;
}

// ids of n sequences fit in this many bits
unsigned kmm_id_bits(uint32_t n) {
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < n) bits++;
    return bits;
}

// sort 1 over nucleotides: (k-mer without its strand bit, value) ascending in three stable passes.  The records of a sequence are born
// in window order, but a window taken as its reverse complement stores its position on the other strand, so the (id, position)
// bits of the value are sorted too; then the length bits, then bits 0 .. 62 of the k-mer (begin_bit 0: the merge-path hazard
// mmgpu_internal.h records needs a begin_bit above 0).  Records that agree in all of that keep the order they were born in.
// In: k-mer cc, value a.  Out: k-mer cc, value a.
int kmm_sort_records_nucl(KmmRun &R) {
    int rc = kmm_sort_pairs(R, "sort by id and position", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.a.as<unsigned long long>(), r.bb.as<unsigned long long>(), r.cc.as<unsigned long long>(),
                                         r.dd.as<unsigned long long>(), (size_t)r.n_records, 0u, KMM_ID_SHIFT + kmm_id_bits(r.b->n), r.s);
    });
    if (rc != MMGPU_OK) return rc;
    rc = kmm_sort_pairs(R, "sort by length", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.bb.as<unsigned long long>(), r.a.as<unsigned long long>(), r.dd.as<unsigned long long>(),
                                         r.cc.as<unsigned long long>(), (size_t)r.n_records, KMM_LEN_SHIFT, KMM_LEN_END, r.s);
    });
    if (rc != MMGPU_OK) return rc;
    rc = kmm_sort_pairs(R, "sort by k-mer", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.cc.as<unsigned long long>(), r.dd.as<unsigned long long>(), r.a.as<unsigned long long>(),
                                         r.bb.as<unsigned long long>(), (size_t)r.n_records, 0u, 63u, r.s);
    });
    std::swap(R.cc, R.dd);      // the k-mers are in dd and the values in bb now: the names follow the contents
    std::swap(R.a, R.bb);
    return rc;
}

// sort 1: (k-mer, value) ascending in two stable passes - by the value's length bits (the records are in (id, position) order
// already), then by the k-mer.  In: k-mer cc, value a.  Out: k-mer cc, value a.
int kmm_sort_records(KmmRun &R) {
    if (R.n_records == 0) return MMGPU_OK;
    if (R.b->nucl) return kmm_sort_records_nucl(R);
    int rc = kmm_sort_pairs(R, "sort by length", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.a.as<unsigned long long>(), r.bb.as<unsigned long long>(), r.cc.as<unsigned long long>(),
                                         r.dd.as<unsigned long long>(), (size_t)r.n_records, KMM_LEN_SHIFT, KMM_LEN_END, r.s);
    });
    if (rc != MMGPU_OK) return rc;
    return kmm_sort_pairs(R, "sort by k-mer", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.dd.as<unsigned long long>(), r.cc.as<unsigned long long>(), r.bb.as<unsigned long long>(),
                                         r.a.as<unsigned long long>(), (size_t)r.n_records, 0u, 64u, r.s);
    });
}

// group: group starts (u1), emit offsets (u2), the emitted pairs (bb) and their biased diagonals (h1) -> n_pairs
int kmm_group(KmmRun &R) {
    const mmgpu_kmermatch_params &p = R.b->par;
    KmmGroupArgs G{};
    G.kmer = R.cc.as<unsigned long long>();
    G.val = R.a.as<unsigned long long>();
    G.n_records = R.n_records;
    G.group_start = R.u1.as<uint32_t>();
    G.cov_thr = p.cov_thr;
    G.cov_mode = p.cov_mode;
    G.only_extendable = p.include_only_extendable ? 1 : 0;
    G.nucl = R.b->nucl ? 1 : 0;
    HIP_TRY(launch_kmm_group_scan(G, R.tile_sum.as<uint32_t>(), R.u2.as<uint32_t>(), R.s));
    const int rc = kmm_read_u32(R, R.u2.as<uint32_t>() + R.n_records, &R.n_pairs);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(launch_kmm_emit(G, R.u2.as<uint32_t>(), R.bb.as<unsigned long long>(), R.h1.as<uint16_t>(), R.s));
    return MMGPU_OK;
}

// sort 2: (representative, member, diagonal) in two stable passes - by the diagonal, then by the pair, whose bits above the ids of
// n sequences are 0 (a nucleotide pair's bit 63, the representative's orientation, lies above them too and is not ordered).
// In: pair bb, diagonal h1.  Out: pair bb, diagonal h1.
int kmm_sort_emitted(KmmRun &R) {
    if (R.n_pairs == 0) return MMGPU_OK;
    int rc = kmm_sort_pairs(R, "sort by diagonal", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.h1.as<uint16_t>(), r.h2.as<uint16_t>(), r.bb.as<unsigned long long>(), r.dd.as<unsigned long long>(),
                                         (size_t)r.n_pairs, 0u, 16u, r.s);
    });
    if (rc != MMGPU_OK) return rc;
    return kmm_sort_pairs(R, "sort by pair", [](KmmRun &r, void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, r.dd.as<unsigned long long>(), r.bb.as<unsigned long long>(), r.h2.as<uint16_t>(), r.h1.as<uint16_t>(),
                                         (size_t)r.n_pairs, 0u, 32u + kmm_id_bits(r.b->n), r.s);
    });
}

// vote: the kept runs (u1: their offsets, u2: their representatives), the result
int kmm_vote(KmmRun &R) {
    mmgpu_kmermatch_batch_t *b = R.b;
    HIP_TRY(launch_kmm_vote_scan(R.bb.as<unsigned long long>(), R.n_pairs, b->nucl, R.tile_sum.as<uint32_t>(), R.u1.as<uint32_t>(), R.s));
    const int rc = kmm_read_u32(R, R.u1.as<uint32_t>() + R.n_pairs, &R.n_kept);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(b->d_offsets.reserve(((size_t)b->n + 1) * 8));
    HIP_TRY(b->d_records.reserve(((size_t)b->n + R.n_kept) * sizeof(mmgpu_pf_hit)));
    HIP_TRY(launch_kmm_vote(R.bb.as<unsigned long long>(), R.h1.as<uint16_t>(), R.n_pairs, b->nucl, R.u1.as<uint32_t>(), R.n_kept, b->n, R.u2.as<uint32_t>(),
                            b->d_offsets.as<unsigned long long>(), b->d_records.as<mmgpu_pf_hit>(), R.s));
    return MMGPU_OK;
}

}  // namespace

namespace mmgpu {

int kmm_check_batch(const char *who, const mmgpu_ctx *c, const mmgpu_kmermatch_batch_t *b, bool must_have_run) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (b->db_res != c->db.res || b->n != c->db.n) return fail(MMGPU_ERR_STATE, std::string(who) + ": the targets were reloaded since the batch was prepared");
    if (must_have_run && !b->ran) return fail(MMGPU_ERR_STATE, std::string(who) + ": the batch has not been run");
    return MMGPU_OK;
}

// a checked parameter set and its record bound -> a batch over the resident database
int kmm_new_batch(const char *who, mmgpu_ctx *c, const mmgpu_kmermatch_params &par, bool nucl, uint64_t bound, mmgpu_kmermatch_batch_t *b) {
    if (bound >= (1ull << 31)) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": 2^31 records or more");
    HIP_TRY(hipSetDevice(c->device));
    b->par = par;
    b->nucl = nucl;
    b->n = c->db.n;
    b->bound = bound;
    b->db_res = c->db.res;
    b->d_offsets.bind(c->cache);
    b->d_records.bind(c->cache);
    b->d_order.bind(c->cache);
    for (hipEvent_t &e : b->ev) HIP_TRY(hipEventCreate(&e));
    return MMGPU_OK;
}

int kmm_run_impl(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b) {
    HIP_TRY(hipSetDevice(c->device));
    // the bound before any kernel: what does not fit is refused with the runtime's out-of-memory error
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (kmm_bytes_needed(kmm_capacity(b), b->n) > (uint64_t)free_b + c->cache->cached)
        return fail(MMGPU_ERR_HIP, std::string(who) + ": " + hipGetErrorString(hipErrorOutOfMemory) + ": the records of this database do not fit in free device memory");
    KmmRun R{who, c, b, c->stream};
    b->ran = false;
    int rc = kmm_alloc(R);
    int (*const steps[KMM_STAGES])(KmmRun &) = {kmm_extract, kmm_sort_records, kmm_group, kmm_sort_emitted, kmm_vote};
    HIP_TRY(hipEventRecord(b->ev[0], R.s));
    for (int i = 0; i < KMM_STAGES && rc == MMGPU_OK; i++) {
        rc = steps[i](R);
        if (rc == MMGPU_OK) HIP_TRY(hipEventRecord(b->ev[i + 1], R.s));
    }
    // the scratch goes back to the shared cache at scope exit: nothing of this run may still be in flight then
    const hipError_t e = hipStreamSynchronize(R.s);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(e);
    b->n_records = R.n_records;
    b->n_pairs = R.n_pairs;
    b->n_kept = R.n_kept;
    b->ran = true;
    return MMGPU_OK;
}

int kmm_fetch(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, mmgpu_kmermatch_counts *counts, void *offsets, void *records, hipMemcpyKind kind) {
    const int rc = kmm_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (counts) {
        counts->n_seqs = b->n;
        counts->n_entries = (uint64_t)b->n + b->n_kept;
        counts->n_records = b->n_records;
        counts->n_pairs = b->n_pairs;
    }
    if (!offsets && !records) return MMGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (offsets) HIP_TRY(hipMemcpyAsync(offsets, b->d_offsets.p, ((size_t)b->n + 1) * 8, kind, c->stream));
    if (records) HIP_TRY(hipMemcpyAsync(records, b->d_records.p, ((size_t)b->n + b->n_kept) * sizeof(mmgpu_pf_hit), kind, c->stream));
    if (kind == hipMemcpyDeviceToHost) HIP_TRY(hipStreamSynchronize(c->stream));      // (a device copy stays ordered on the stream)
    return MMGPU_OK;
}

int kmm_kernel_ms(const char *who, mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, float *ms) {
    const int rc = kmm_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!ms) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(b->ev[KMM_STAGES]));
    HIP_TRY(hipEventElapsedTime(&ms[0], b->ev[0], b->ev[KMM_STAGES]));
    for (int i = 0; i < KMM_STAGES; i++) HIP_TRY(hipEventElapsedTime(&ms[1 + i], b->ev[i], b->ev[i + 1]));
    return MMGPU_OK;
}

}  // namespace mmgpu

extern "C" int mmgpu_kmermatch_prepare(mmgpu_ctx *c, const mmgpu_kmermatch_params *par, mmgpu_kmermatch_batch_t **out) {
    const char *who = "mmgpu_kmermatch_prepare";
    if (out) *out = nullptr;
    if (!out) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    int rc = kmm_check_params(who, par);
    if (rc != MMGPU_OK) return rc;
    if (!c) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    rc = kmm_check_db(who, c);
    if (rc != MMGPU_OK) return rc;
    std::unique_ptr<mmgpu_kmermatch_batch_t> b(new mmgpu_kmermatch_batch_t());
    rc = kmm_new_batch(who, c, *par, false, kmm_record_bound(c->h_len, *par), b.get());
    if (rc != MMGPU_OK) return rc;
    *out = b.release();
    return MMGPU_OK;
}

extern "C" int mmgpu_kmermatch_run(mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b) {
    const int rc = kmm_check_batch("mmgpu_kmermatch_run", c, b, false);
    if (rc != MMGPU_OK) return rc;
    return kmm_run_impl("mmgpu_kmermatch_run", c, b);
}

extern "C" int mmgpu_kmermatch_fetch(mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, mmgpu_kmermatch_counts *counts, uint64_t *offsets, mmgpu_pf_hit *records) {
    return kmm_fetch("mmgpu_kmermatch_fetch", c, b, counts, offsets, records, hipMemcpyDeviceToHost);
}

extern "C" int mmgpu_kmermatch_fetch_device(mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, void *d_offsets, void *d_records) {
    if (!d_offsets && !d_records) return fail(MMGPU_ERR_ARG, "mmgpu_kmermatch_fetch_device: NULL argument");
    return kmm_fetch("mmgpu_kmermatch_fetch_device", c, b, nullptr, d_offsets, d_records, hipMemcpyDeviceToDevice);
}

extern "C" int mmgpu_kmermatch_last_kernel_ms(mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b, float *ms) {
    return kmm_kernel_ms("mmgpu_kmermatch_last_kernel_ms", c, b, ms);
}

extern "C" void mmgpu_kmermatch_free(mmgpu_ctx *c, mmgpu_kmermatch_batch_t *b) {
    if (!b) return;
    scan_sync_for_free(c);      // nothing of the batch is in flight
    delete b;
}
