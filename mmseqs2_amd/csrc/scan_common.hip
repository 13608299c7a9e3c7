// What the batches of the two exhaustive scans do alike on the host (scan_api.hip, gscan_api.hip): the checks of a prepare call that
// do not depend on the kind of scan, the batch header, the matrix and list buffers, the reload / has-run check, the fetches, the
// kernel time and the read-back of the score scratch.  Every function takes the name of the entry point it serves and composes the
// message from it.
#include <string>
#include <vector>

#include "mmgpu_internal.h"

namespace mmgpu {

int scan_check_db(const char *who, const mmgpu_ctx *c, bool have_args, int alphabet) {
    if (!have_args) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument or no queries");
    if (!c->db.res || c->db.n == 0) return fail(MMGPU_ERR_STATE, std::string(who) + ": no targets loaded");
    if (c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": the context holds a shard of a multi-GPU run");
    if (alphabet != c->db.alphabet) return fail(MMGPU_ERR_ARG, std::string(who) + ": alphabet differs from the loaded targets");
    return MMGPU_OK;
}

int scan_check_size(const char *who, const mmgpu_ctx *c, uint32_t nq, uint32_t max_hits, size_t score_size) {
    if (max_hits == 0) return fail(MMGPU_ERR_ARG, std::string(who) + ": max_hits must be >= 1");
    if (max_hits > MMGPU_PF_MAX_FUSED_HITS) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": max_hits above MMGPU_PF_MAX_FUSED_HITS");
    if ((uint64_t)nq * c->db.n > (4ull << 30) / score_size) {
        const std::string unit = score_size == 1 ? "" : " x " + std::to_string(score_size) + " bytes";
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": more than 4 GiB of scores (queries x resident targets" + unit + "): send smaller batches");
    }
    return MMGPU_OK;
}

void scan_fill_header(ScanBatchCommon *b, const mmgpu_ctx *c, uint32_t nq, int alphabet, int32_t min_score, uint32_t max_hits, uint64_t serial) {
    b->nq = nq;
    b->n_targets = c->db.n;
    b->max_hits = max_hits;
    b->stride = std::min(max_hits, c->db.n);
    b->min_score = min_score;
    b->alphabet = alphabet;
    b->db_res = c->db.res;
    b->serial = serial;
}

int scan_upload_common(mmgpu_ctx *c, ScanBatchCommon *b, const int8_t *matrix) {
    hipStream_t s = c->stream;
    for (DevBuf *d : {&b->d_mat, &b->d_hits, &b->d_counts}) d->bind(c->cache);
    const std::vector<int8_t> mat(matrix, matrix + (size_t)b->alphabet * b->alphabet);
    HIP_TRY(upload(b->d_mat, mat, s));
    HIP_TRY(b->d_hits.alloc((size_t)b->nq * b->stride * sizeof(mmgpu_pf_hit)));
    HIP_TRY(b->d_counts.alloc((size_t)b->nq * sizeof(uint32_t)));
    HIP_TRY(hipStreamSynchronize(s));      // the host vectors of the caller's uploads go with this call
    return MMGPU_OK;
}

int scan_check_batch(const char *who, const mmgpu_ctx *c, const ScanBatchCommon *b, bool must_have_run) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (b->db_res != c->db.res || b->n_targets != c->db.n) return fail(MMGPU_ERR_STATE, std::string(who) + ": the targets were reloaded since the batch was prepared");
    if (must_have_run && !b->ran) return fail(MMGPU_ERR_STATE, std::string(who) + ": the batch has not been run");
    return MMGPU_OK;
}

int scan_fetch_lists(const char *who, mmgpu_ctx *c, ScanBatchCommon *b, void *hits, uint32_t hit_stride, void *counts, hipMemcpyKind kind) {
    const int rc = scan_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!hits || !counts) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (hit_stride < b->stride) return fail(MMGPU_ERR_ARG, std::string(who) + ": hit_stride below min(max_hits, resident targets)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy2DAsync(hits, (size_t)hit_stride * sizeof(mmgpu_pf_hit), b->d_hits.p, (size_t)b->stride * sizeof(mmgpu_pf_hit),
                             (size_t)b->stride * sizeof(mmgpu_pf_hit), b->nq, kind, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, b->d_counts.p, (size_t)b->nq * sizeof(uint32_t), kind, c->stream));
    if (kind == hipMemcpyDeviceToHost) HIP_TRY(hipStreamSynchronize(c->stream));      // (a device copy stays ordered on the stream)
    return MMGPU_OK;
}

int scan_kernel_ms(const char *who, mmgpu_ctx *c, ScanBatchCommon *b, float *ms) {
    const int rc = scan_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!ms) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(b->ev1));
    HIP_TRY(hipEventElapsedTime(ms, b->ev0, b->ev1));
    return MMGPU_OK;
}

int scan_debug_scores(const char *who, const char *kind, mmgpu_ctx *c, ScanBatchCommon *b, uint64_t mmgpu_ctx::*serial, DevBuf mmgpu_ctx::*scratch,
                      size_t score_size, uint32_t query, void *out, size_t cap) {
    const int rc = scan_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (c->*serial != b->serial) return fail(MMGPU_ERR_STATE, std::string(who) + ": another " + kind + " batch has run on the context since");
    if (!out || query >= b->nq || cap < b->n_targets) return fail(MMGPU_ERR_ARG, std::string(who) + ": bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t row = (size_t)b->n_targets * score_size;
    HIP_TRY(hipMemcpyAsync(out, (c->*scratch).as<uint8_t>() + (size_t)query * row, row, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MMGPU_OK;
}

void scan_sync_for_free(mmgpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
}

}  // namespace mmgpu
