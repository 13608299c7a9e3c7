// Host side of the exhaustive ungapped scan (include/mmgpu.h, "exhaustive ungapped scan"): the scan's own validation, the per-query bias
// of sequence and of profile queries, the job lists, launches of scan_kernel.hip.  prepare and run are sequences of named steps over one
// record each, in the manner of sw_prepare_impl (mmgpu_api.hip).  What a batch holds and does like the gapped scan's - header, common
// checks, list buffers, fetches, kernel time, score read-back - is scan_common.hip's; the entry points here name themselves and call it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mmgpu_internal.h"

using namespace mmgpu;

struct mmgpu_scan_batch_t : ScanBatchCommon {
    DevBuf d_qres, d_qcb, d_qoff, d_qcap, d_qprof, d_qprof_off, d_qprof_letters, d_qident, d_qwin, d_order, d_jobs, d_park_off;
    uint32_t class_begin[SCAN_CLASSES + 1] = {};   // jobs of class k: d_jobs[class_begin[k] .. class_begin[k + 1])
    uint32_t multi_grid = 0;              // persistent workgroups of the multi-tile launch
    uint64_t park_words = 0;              // dwords of boundary lines they need
};

namespace {

std::atomic<uint64_t> g_scan_serial{0};

// what prepare builds on the host before anything is uploaded
struct ScanPrepare {
    mmgpu_ctx *c;
    const mmgpu_scan_params *par;
    const mmgpu_scan_query *qs;
    uint32_t nq;
    std::vector<uint8_t> qres;
    std::vector<int8_t> qcb, qprof;      // qprof: the profile queries' tables, one after the other
    std::vector<uint64_t> qprof_off;     // [nq] offset into qprof, SCAN_NO_PROFILE for a sequence query
    std::vector<uint32_t> qprof_letters; // [nq]
    std::vector<uint32_t> qoff, qident, qwin, order, first_le;   // first_le[L]: position of the first target of length <= L in `order`
    std::vector<int32_t> qcap;
    std::vector<ScanJob> jobs;
    std::vector<uint64_t> park_off;
};

int scan_check_call(const ScanPrepare &S) {
    const char *who = "mmgpu_scan_prepare";
    int rc = scan_check_db(who, S.c, S.par && S.qs && S.nq && S.par->mat, S.par ? S.par->alphabet : 0);
    if (rc != MMGPU_OK) return rc;
    if (S.par->alphabet > 32) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_scan_prepare: sequence queries over a protein database only (alphabet <= 32)");
    return scan_check_size(who, S.c, S.nq, S.par->max_hits, sizeof(uint8_t));
}

// the two range checks of a query whose bias is B and whose highest profile score is p_max, and its cap (ssw_init, :1397-1406)
int scan_cap_of(int B, int p_max, int32_t *cap) {
    if (255 - B <= 0) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: the bias leaves no score range (255 - B <= 0)");
    if (p_max + B > 255) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: a profile score plus the bias exceeds 255 (the reference's byte profile wraps)");
    *cap = 255 - B;
    return MMGPU_OK;
}

// a profile query: its table goes into the pool, B comes from the table alone (StripedSmithWaterman.cpp:1376-1385, :1397-1406);
// q and comp_bias are not read, the residue pools get zeros so that q_off keeps giving every query's length
int scan_marshal_profile(ScanPrepare &S, const mmgpu_scan_query &Q, int32_t *cap) {
    if (Q.profile_letters == 0 || Q.profile_letters > (uint32_t)S.par->alphabet)
        return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: profile_letters must be 1 .. alphabet for a profile query");
    const size_t n = (size_t)Q.profile_letters * Q.qlen;
    int p_min = 0, p_max = -128;
    for (size_t k = 0; k < n; k++) {
        p_min = std::min<int>(p_min, Q.profile[k]);
        p_max = std::max<int>(p_max, Q.profile[k]);
    }
    const int rc = scan_cap_of(std::abs(p_min), std::max(p_max, 0), cap);      // (the letters without a row score 0)
    if (rc != MMGPU_OK) return rc;
    S.qprof_off.push_back(S.qprof.size());
    S.qprof_letters.push_back(Q.profile_letters);
    S.qprof.insert(S.qprof.end(), Q.profile, Q.profile + n);
    S.qres.insert(S.qres.end(), Q.qlen, 0);
    S.qcb.insert(S.qcb.end(), Q.qlen, 0);
    return MMGPU_OK;
}

struct ScanMatRange {
    int mat_min = 0;
    std::vector<int> col_max;      // best score a query letter can meet
};

int scan_marshal_sequence(ScanPrepare &S, const mmgpu_scan_query &Q, const ScanMatRange &M, int32_t *cap) {
    if (!Q.q) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: empty query");
    int cb_min = 0, p_max = -32768;
    for (uint32_t k = 0; k < Q.qlen; k++) {
        if (Q.q[k] >= S.par->alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: query letter outside the alphabet");
        const int cb = Q.comp_bias ? Q.comp_bias[k] : 0;
        cb_min = std::min(cb_min, cb);
        p_max = std::max(p_max, M.col_max[Q.q[k]] + cb);
    }
    const int rc = scan_cap_of(std::abs(M.mat_min) + std::abs(cb_min), p_max, cap);
    if (rc != MMGPU_OK) return rc;
    S.qprof_off.push_back(SCAN_NO_PROFILE);
    S.qprof_letters.push_back(0);
    S.qres.insert(S.qres.end(), Q.q, Q.q + Q.qlen);
    if (Q.comp_bias) S.qcb.insert(S.qcb.end(), Q.comp_bias, Q.comp_bias + Q.qlen);
    else S.qcb.insert(S.qcb.end(), Q.qlen, 0);
    return MMGPU_OK;
}

// residues or profile, bias, window and identity of every query; B and 255 - B as ssw_init derives them
// (StripedSmithWaterman.cpp:1397-1406)
int scan_marshal_queries(ScanPrepare &S) {
    const int alphabet = S.par->alphabet;
    const int8_t *mat = S.par->mat;
    ScanMatRange M;
    for (int i = 0; i < alphabet * alphabet; i++) M.mat_min = std::min<int>(M.mat_min, mat[i]);
    M.col_max.assign(alphabet, -128);
    for (int x = 0; x < alphabet; x++)
        for (int a = 0; a < alphabet; a++) M.col_max[a] = std::max<int>(M.col_max[a], mat[x * alphabet + a]);
    S.qoff.assign(1, 0);
    uint64_t total = 0;
    for (uint32_t i = 0; i < S.nq; i++) {
        const mmgpu_scan_query &Q = S.qs[i];
        if (Q.qlen == 0) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: empty query");
        if (Q.min_tlen > Q.max_tlen) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: min_tlen above max_tlen");
        total += Q.qlen;
        if (total > 0x7FFFFFFFull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_scan_prepare: more than 2 GiB of query residues in one batch");
        int32_t cap = 0;
        const int rc = Q.profile ? scan_marshal_profile(S, Q, &cap) : scan_marshal_sequence(S, Q, M, &cap);
        if (rc != MMGPU_OK) return rc;
        S.qoff.push_back((uint32_t)total);
        S.qcap.push_back(cap);
        S.qident.push_back(Q.identity_id);
        S.qwin.push_back(Q.min_tlen);
        S.qwin.push_back(Q.max_tlen);
    }
    return MMGPU_OK;
}

void scan_order_targets(ScanPrepare &S) { order_targets_by_length(S.c->h_len, S.order, S.first_le); }

// jobs by class; one-tile classes: SCAN_JOB_TARGETS consecutive list positions of one query, multi-tile: one round.  Inside a class
// the jobs with the longest targets come first (they run longest; the multi-tile slots are sized by their first job).
void scan_cut_jobs(ScanPrepare &S, mmgpu_scan_batch_t *b) {
    const uint32_t n = (uint32_t)S.order.size();
    std::vector<ScanJob> by_class[SCAN_CLASSES];
    for (uint32_t q = 0; q < S.nq; q++) {
        const uint32_t qlen = S.qoff[q + 1] - S.qoff[q];
        int cls = SCAN_MULTI;
        for (int k = 0; k < SCAN_MULTI; k++)
            if (qlen <= 16u * (uint32_t)scan_class_rows(k)) { cls = k; break; }
        const uint32_t lo = S.qwin[2 * q], hi = S.qwin[2 * q + 1];
        uint32_t begin, end;
        window_slice(S.first_le, n, lo, hi, &begin, &end);
        const uint32_t step = cls == SCAN_MULTI ? (uint32_t)SCAN_ROUND : (uint32_t)SCAN_JOB_TARGETS;
        for (uint32_t p = begin; p < end; p += std::min(step, end - p)) by_class[cls].push_back(ScanJob{q, p, std::min(end, p + step), 0});
    }
    b->class_begin[0] = 0;
    for (int k = 0; k < SCAN_CLASSES; k++) {
        std::stable_sort(by_class[k].begin(), by_class[k].end(), [](const ScanJob &a, const ScanJob &z) { return a.begin < z.begin; });
        S.jobs.insert(S.jobs.end(), by_class[k].begin(), by_class[k].end());
        b->class_begin[k + 1] = (uint32_t)S.jobs.size();
    }
    // persistent workgroups of the multi-tile launch and their boundary lines: workgroup w runs jobs w, w + grid, ..; the first is its
    // longest (positions ascend = lengths descend)
    const uint32_t n_multi = b->class_begin[SCAN_MULTI + 1] - b->class_begin[SCAN_MULTI];
    b->multi_grid = std::min<uint32_t>(n_multi, 2u * (uint32_t)std::max(S.c->compute_units, 1));
    uint64_t words = 0;
    for (uint32_t w = 0; w < b->multi_grid; w++) {
        const ScanJob &j = S.jobs[b->class_begin[SCAN_MULTI] + w];
        S.park_off.push_back(words);
        words += (uint64_t)(SCAN_ROUND / 2) * scan_park_row_words(S.c->h_len[S.order[j.begin]]);
    }
    b->park_words = words;
}

int scan_upload(ScanPrepare &S, mmgpu_scan_batch_t *b) {
    mmgpu_ctx *c = S.c;
    hipStream_t s = c->stream;
    for (DevBuf *d : {&b->d_qres, &b->d_qcb, &b->d_qoff, &b->d_qcap, &b->d_qprof, &b->d_qprof_off, &b->d_qprof_letters, &b->d_qident,
                      &b->d_qwin, &b->d_order, &b->d_jobs, &b->d_park_off})
        d->bind(c->cache);
    HIP_TRY(upload(b->d_qres, S.qres, s));
    HIP_TRY(upload(b->d_qcb, S.qcb, s));
    HIP_TRY(upload(b->d_qoff, S.qoff, s));
    HIP_TRY(upload(b->d_qcap, S.qcap, s));
    HIP_TRY(upload(b->d_qprof, S.qprof, s));
    HIP_TRY(upload(b->d_qprof_off, S.qprof_off, s));
    HIP_TRY(upload(b->d_qprof_letters, S.qprof_letters, s));
    HIP_TRY(upload(b->d_qident, S.qident, s));
    HIP_TRY(upload(b->d_qwin, S.qwin, s));
    HIP_TRY(upload(b->d_order, S.order, s));
    HIP_TRY(upload(b->d_jobs, S.jobs, s));
    HIP_TRY(upload(b->d_park_off, S.park_off, s));
    return scan_upload_common(c, b, S.par->mat);
}

int scan_prepare_impl(mmgpu_ctx *c, const mmgpu_scan_params *par, const mmgpu_scan_query *qs, uint32_t nq, mmgpu_scan_batch_t **out) {
    ScanPrepare S{c, par, qs, nq};
    int rc = scan_check_call(S);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = scan_marshal_queries(S);
    if (rc != MMGPU_OK) return rc;
    std::unique_ptr<mmgpu_scan_batch_t> b(new mmgpu_scan_batch_t());
    scan_fill_header(b.get(), c, nq, par->alphabet, par->min_score, par->max_hits, ++g_scan_serial);
    scan_order_targets(S);
    scan_cut_jobs(S, b.get());
    rc = scan_upload(S, b.get());
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
    *out = b.release();
    return MMGPU_OK;
}

// the context's scratch: score bytes of the largest batch so far, boundary lines of the multi-tile workgroups
int scan_reserve_scratch(mmgpu_ctx *c, const mmgpu_scan_batch_t *b) {
    const size_t score_bytes = (size_t)b->nq * b->n_targets;
    if (score_bytes > c->scan_scores.bytes || b->park_words * 4 > c->scan_park.bytes) HIP_TRY(hipStreamSynchronize(c->stream));   // a grown buffer frees the old one
    HIP_TRY(c->scan_scores.reserve(score_bytes));
    HIP_TRY(c->scan_park.reserve((size_t)b->park_words * 4));
    return MMGPU_OK;
}

int scan_launch_classes(mmgpu_ctx *c, mmgpu_scan_batch_t *b) {
    ScanLaunch L;
    L.q_res = b->d_qres.as<uint8_t>();
    L.q_cb = b->d_qcb.as<int8_t>();
    L.q_off = b->d_qoff.as<uint32_t>();
    L.q_cap = b->d_qcap.as<int32_t>();
    L.q_prof = b->d_qprof.as<int8_t>();
    L.q_prof_off = b->d_qprof_off.as<uint64_t>();
    L.q_prof_letters = b->d_qprof_letters.as<uint32_t>();
    L.t_res = c->db.res;
    L.t_off4 = c->db.off4;
    L.t_len = c->db.len;
    L.order = b->d_order.as<uint32_t>();
    L.n_targets = b->n_targets;
    L.mat = b->d_mat.as<int8_t>();
    L.alphabet = b->alphabet;
    L.scores = c->scan_scores.as<uint8_t>();
    L.park = c->scan_park.as<uint32_t>();
    L.park_off = b->d_park_off.as<uint64_t>();
    // targets outside a query's window are not scored: their bytes read 0
    HIP_TRY(hipMemsetAsync(L.scores, 0, (size_t)b->nq * b->n_targets, c->stream));
    for (int k = 0; k < SCAN_CLASSES; k++) {
        L.jobs = b->d_jobs.as<ScanJob>() + b->class_begin[k];
        L.n_jobs = b->class_begin[k + 1] - b->class_begin[k];
        HIP_TRY(launch_scan(L, k, k == SCAN_MULTI ? b->multi_grid : L.n_jobs, c->stream));
    }
    return MMGPU_OK;
}

int scan_launch_select(mmgpu_ctx *c, mmgpu_scan_batch_t *b) {
    ScanSelectArgs A;
    A.scores = c->scan_scores.as<uint8_t>();
    A.t_len = c->db.len;
    A.n_targets = b->n_targets;
    A.q_ident = b->d_qident.as<uint32_t>();
    A.q_win = b->d_qwin.as<uint32_t>();
    A.min_score = b->min_score;
    A.max_hits = b->max_hits;
    A.hits = b->d_hits.as<mmgpu_pf_hit>();
    A.stride = b->stride;
    A.counts = b->d_counts.as<uint32_t>();
    HIP_TRY(launch_scan_select(A, b->nq, c->stream));
    return MMGPU_OK;
}

}  // namespace

extern "C" int mmgpu_scan_prepare(mmgpu_ctx *c, const mmgpu_scan_params *par, const mmgpu_scan_query *qs, uint32_t nq,
                                  mmgpu_scan_batch_t **out) {
    if (out) *out = nullptr;
    if (!c || !out) return fail(MMGPU_ERR_ARG, "mmgpu_scan_prepare: NULL argument");
    return scan_prepare_impl(c, par, qs, nq, out);
}

extern "C" int mmgpu_scan_run(mmgpu_ctx *c, mmgpu_scan_batch_t *b) {
    int rc = scan_check_batch("mmgpu_scan_run", c, b, false);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = scan_reserve_scratch(c, b);
    if (rc != MMGPU_OK) return rc;
    c->scan_serial = b->serial;
    HIP_TRY(hipEventRecord(b->ev0, c->stream));
    rc = scan_launch_classes(c, b);
    if (rc != MMGPU_OK) return rc;
    rc = scan_launch_select(c, b);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipEventRecord(b->ev1, c->stream));
    b->ran = true;
    return MMGPU_OK;
}

extern "C" int mmgpu_scan_fetch(mmgpu_ctx *c, mmgpu_scan_batch_t *b, mmgpu_pf_hit *hits, uint32_t hit_stride, uint32_t *counts) {
    return scan_fetch_lists("mmgpu_scan_fetch", c, b, hits, hit_stride, counts, hipMemcpyDeviceToHost);
}

extern "C" int mmgpu_scan_fetch_device(mmgpu_ctx *c, mmgpu_scan_batch_t *b, void *d_hits, uint32_t hit_stride, void *d_counts) {
    return scan_fetch_lists("mmgpu_scan_fetch_device", c, b, d_hits, hit_stride, d_counts, hipMemcpyDeviceToDevice);
}

extern "C" int mmgpu_scan_last_kernel_ms(mmgpu_ctx *c, mmgpu_scan_batch_t *b, float *ms) {
    return scan_kernel_ms("mmgpu_scan_last_kernel_ms", c, b, ms);
}

extern "C" void mmgpu_scan_free(mmgpu_ctx *c, mmgpu_scan_batch_t *b) {
    if (!b) return;
    scan_sync_for_free(c);
    delete b;
}

extern "C" int mmgpu_scan_batch(mmgpu_ctx *c, const mmgpu_scan_params *par, const mmgpu_scan_query *qs, uint32_t nq, mmgpu_pf_hit *hits,
                                uint32_t hit_stride, uint32_t *counts) {
    mmgpu_scan_batch_t *b = nullptr;
    int rc = mmgpu_scan_prepare(c, par, qs, nq, &b);
    if (rc != MMGPU_OK) return rc;
    rc = mmgpu_scan_run(c, b);
    if (rc == MMGPU_OK) rc = mmgpu_scan_fetch(c, b, hits, hit_stride, counts);
    mmgpu_scan_free(c, b);
    return rc;
}

extern "C" int mmgpu_scan_debug_scores(mmgpu_ctx *c, mmgpu_scan_batch_t *b, uint32_t query, uint8_t *out, size_t cap) {
    return scan_debug_scores("mmgpu_scan_debug_scores", "scan", c, b, &mmgpu_ctx::scan_serial, &mmgpu_ctx::scan_scores, sizeof(uint8_t),
                             query, out, cap);
}
