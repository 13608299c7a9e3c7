// Host side of linclust's k-mer matching stage over a nucleotide database (include/mmgpu.h, "linclust's k-mer matching stage,
// nucleotides"): the refusals, the record bound and the length order of the launch.  The batch is kmermatch_api.hip's with its
// strand flag set, and run, fetch and the stage times are that file's.
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "mmgpu_internal.h"

using namespace mmgpu;

namespace {

constexpr int NM_MAX_K = 31;      // 2k bits of index below bit 63, which carries the strand

// computeKmerCount (kmermatcher.cpp:1100-1108) with the nucleotide scale
uint64_t nm_record_bound(const std::vector<uint32_t> &len, const mmgpu_nuclmatch_params &p) {
    uint64_t total = 0;
    for (uint32_t l : len) {
        const int seq_len = (int)l;
        const int adjusted = std::max(1, seq_len - p.k + 2);
        total += (uint64_t)std::max(0, std::min(adjusted, static_cast<int>(p.kmers_per_seq + (p.kmers_per_seq_scale * seq_len))));
    }
    return total;
}

// the parameters alone: decided before the context is looked at
int nm_check_params(const char *who, const mmgpu_nuclmatch_params *p) {
    if (!p) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (p->k < 1 || p->k > NM_MAX_K) return fail(MMGPU_ERR_ARG, std::string(who) + ": k must be 1 .. 31");
    if (p->kmers_per_seq < 1) return fail(MMGPU_ERR_ARG, std::string(who) + ": kmers_per_seq must be 1 or more");
    if (!(p->kmers_per_seq_scale >= 0.0f) || !std::isfinite(p->kmers_per_seq_scale)) return fail(MMGPU_ERR_ARG, std::string(who) + ": kmers_per_seq_scale must be 0 or more");
    if (p->cov_mode < 0 || p->cov_mode > 5) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": cov_mode outside 0 .. 5");
    if (p->cov_mode == 1)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": cov_mode 1 on a nucleotide database (the reference's target-coverage swap stores the pair without its strand; not built here)");
    return MMGPU_OK;
}

int nm_check_db(const char *who, const mmgpu_ctx *c) {
    if (!c->db.res || c->db.n == 0) return fail(MMGPU_ERR_STATE, std::string(who) + ": no targets loaded");
    if (c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": the context holds a shard of a multi-GPU run");
    if (c->db.alphabet != 5) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": nucleotide sequences only (alphabet 5; a protein database goes to mmgpu_kmermatch_prepare)");
    if (c->db.max_len > KMM_MAX_LEN)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": a sequence of 32 767 residues or more (the reference then keeps int positions; not built here)");
    return MMGPU_OK;
}

}  // namespace

extern "C" int mmgpu_nuclmatch_prepare(mmgpu_ctx *c, const mmgpu_nuclmatch_params *par, mmgpu_nuclmatch_batch_t **out) {
    const char *who = "mmgpu_nuclmatch_prepare";
    if (out) *out = nullptr;
    if (!out) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    int rc = nm_check_params(who, par);
    if (rc != MMGPU_OK) return rc;
    if (!c) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    rc = nm_check_db(who, c);
    if (rc != MMGPU_OK) return rc;
    mmgpu_kmermatch_params shared{};      // what the shared stages read
    shared.k = par->k;
    shared.alph_size = 5;
    shared.kmers_per_seq = par->kmers_per_seq;
    shared.kmers_per_seq_scale = par->kmers_per_seq_scale;
    shared.hash_shift = par->hash_shift;
    shared.cov_thr = par->cov_thr;
    shared.cov_mode = par->cov_mode;
    shared.include_only_extendable = par->include_only_extendable;
    std::unique_ptr<mmgpu_nuclmatch_batch_t> b(new mmgpu_nuclmatch_batch_t());
    rc = kmm_new_batch(who, c, shared, true, nm_record_bound(c->h_len, *par), b.get());
    if (rc != MMGPU_OK) return rc;
    // the launch order of the extraction: longest first, so that the tail of the grid is short sequences and not one of 32 766 residues
    std::vector<uint32_t> order, first_le;
    order_targets_by_length(c->h_len, order, first_le);
    HIP_TRY(upload(b->d_order, order, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the copy reads `order`)
    *out = b.release();
    return MMGPU_OK;
}

extern "C" int mmgpu_nuclmatch_run(mmgpu_ctx *c, mmgpu_nuclmatch_batch_t *b) {
    const int rc = kmm_check_batch("mmgpu_nuclmatch_run", c, b, false);
    if (rc != MMGPU_OK) return rc;
    return kmm_run_impl("mmgpu_nuclmatch_run", c, b);
}

extern "C" int mmgpu_nuclmatch_fetch(mmgpu_ctx *c, mmgpu_nuclmatch_batch_t *b, mmgpu_kmermatch_counts *counts, uint64_t *offsets, mmgpu_pf_hit *records) {
    return kmm_fetch("mmgpu_nuclmatch_fetch", c, b, counts, offsets, records, hipMemcpyDeviceToHost);
}

extern "C" int mmgpu_nuclmatch_fetch_device(mmgpu_ctx *c, mmgpu_nuclmatch_batch_t *b, void *d_offsets, void *d_records) {
    if (!d_offsets && !d_records) return fail(MMGPU_ERR_ARG, "mmgpu_nuclmatch_fetch_device: NULL argument");
    return kmm_fetch("mmgpu_nuclmatch_fetch_device", c, b, nullptr, d_offsets, d_records, hipMemcpyDeviceToDevice);
}

extern "C" int mmgpu_nuclmatch_last_kernel_ms(mmgpu_ctx *c, mmgpu_nuclmatch_batch_t *b, float *ms) {
    return kmm_kernel_ms("mmgpu_nuclmatch_last_kernel_ms", c, b, ms);
}

extern "C" void mmgpu_nuclmatch_free(mmgpu_ctx *c, mmgpu_nuclmatch_batch_t *b) {
    if (!b) return;
    scan_sync_for_free(c);      // nothing of the batch is in flight
    delete b;
}
