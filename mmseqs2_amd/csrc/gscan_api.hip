// Host side of the exhaustive gapped scan (include/mmgpu.h, "exhaustive gapped scan"): the scan's own validation, the window slices and
// chunks, one dense alignment batch per chunk (sw_prepare_dense: the checks, queries, job rules and kernels of mmgpu_sw_prepare), launches
// of gscan_kernel.hip around them.  prepare and run are sequences of named steps over one record each, in the manner of scan_api.hip.
// What a batch holds and does like the ungapped scan's is scan_common.hip's; the entry points here name themselves and call it.  Its
// own: the alignment batches, which only release(ctx) can free.
#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "mmgpu_internal.h"

using namespace mmgpu;

struct mmgpu_gscan_batch_t : ScanBatchCommon {
    bool any_profile = false;
    // a chunk: queries [q_first, q_first + nq) and their alignment batch over the shared lists and records
    struct Chunk {
        uint32_t q_first = 0, nq = 0;
        uint64_t pairs = 0;
        mmgpu_sw_batch_t *sw = nullptr;
        std::array<hipEvent_t, 4> ev = {};      // before the planner, before the alignment kernels, before the selection, after it
    };
    std::vector<Chunk> chunks;
    DevBuf d_qres, d_qcb, d_qoff, d_qprof, d_qprof_off, d_qident, d_qwin, d_qminev, d_order, d_qbegin, d_qcount, d_qslot, d_ident_score;
    DevBuf d_hit_target, d_hit_out, d_out;      // the largest chunk's lists and records, reused by every chunk
    hipEvent_t ev_ident = nullptr;      // behind the identity kernel
    // the alignment batches and their events go here, not in a destructor: freeing an alignment batch needs the context
    void release(mmgpu_ctx *c) {
        for (Chunk &k : chunks) {
            if (k.sw) mmgpu_sw_free(c, k.sw);
            for (hipEvent_t e : k.ev)
                if (e) (void)hipEventDestroy(e);
        }
        chunks.clear();
        if (ev_ident) (void)hipEventDestroy(ev_ident);
        ev_ident = nullptr;
    }
};

namespace {

std::atomic<uint64_t> g_gscan_serial{0};

struct GscanBatchFree {
    mmgpu_ctx *c;
    void operator()(mmgpu_gscan_batch_t *b) const {
        b->release(c);
        delete b;
    }
};

// what prepare builds on the host before anything is uploaded
struct GscanPrepare {
    mmgpu_ctx *c;
    const mmgpu_gscan_params *par;
    const mmgpu_gscan_query *qs;
    uint32_t nq;
    mmgpu_gscan_batch_t *b = nullptr;
    std::vector<uint32_t> order, first_le;
    std::vector<uint64_t> len_prefix;                 // [n + 1] residues of order[0 .. k)
    std::vector<uint32_t> qbegin, qcount, qslot, qident, qwin;
    std::vector<int32_t> qminev;
    std::vector<mmgpu_sw_query> sw_queries;
    uint64_t max_chunk_pairs = 0;
    // the identity kernel's copy of the queries, in the alignment batch's layout
    std::vector<uint8_t> qres;
    std::vector<int8_t> qcb, qprof;
    std::vector<uint32_t> qoff, qprof_off;
};

int gscan_check_call(const GscanPrepare &S) {
    const char *who = "mmgpu_gscan_prepare";
    const int rc = scan_check_db(who, S.c, S.par && S.qs && S.nq && S.par->mat, S.par ? S.par->alphabet : 0);
    if (rc != MMGPU_OK) return rc;
    return scan_check_size(who, S.c, S.nq, S.par->max_hits, sizeof(int32_t));
}

// every query's slice of the length-ordered id list and its identity target: inside the window it must have the query's length
// (SmithWaterman::scoreIdentical exits otherwise), outside it the query has none
int gscan_slices(GscanPrepare &S) {
    const std::vector<uint32_t> &len = S.c->h_len;
    const uint32_t n = (uint32_t)len.size();
    order_targets_by_length(len, S.order, S.first_le);
    S.len_prefix.assign((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; k++) S.len_prefix[k + 1] = S.len_prefix[k] + len[S.order[k]];
    for (uint32_t i = 0; i < S.nq; i++) {
        const mmgpu_gscan_query &Q = S.qs[i];
        if (Q.qlen == 0 || !Q.q) return fail(MMGPU_ERR_ARG, "mmgpu_gscan_prepare: empty query");
        if (Q.min_tlen > Q.max_tlen) return fail(MMGPU_ERR_ARG, "mmgpu_gscan_prepare: min_tlen above max_tlen");
        uint32_t begin, end;
        window_slice(S.first_le, n, Q.min_tlen, Q.max_tlen, &begin, &end);
        uint32_t ident = Q.identity_id;
        if (ident != 0xFFFFFFFFu) {
            if (ident >= n) return fail(MMGPU_ERR_ARG, "mmgpu_gscan_prepare: identity_id out of range");
            if (len[ident] < Q.min_tlen || len[ident] > Q.max_tlen) ident = 0xFFFFFFFFu;
            else if (len[ident] != Q.qlen)
                return fail(MMGPU_ERR_ARG, "mmgpu_gscan_prepare: the identity target's length differs from the query's (the reference's scoreIdentical exits)");
        }
        S.qbegin.push_back(begin);
        S.qcount.push_back(end - begin);
        S.qident.push_back(ident);
        S.qwin.push_back(Q.min_tlen);
        S.qwin.push_back(Q.max_tlen);
        S.qminev.push_back(Q.min_evalue_score);
        mmgpu_sw_query W;
        memset(&W, 0, sizeof(W));
        W.q = Q.q;
        W.qlen = Q.qlen;
        W.comp_bias = Q.comp_bias;
        W.profile = Q.profile;
        W.profile_letters = Q.profile_letters;
        S.sw_queries.push_back(W);
        S.b->any_profile |= Q.profile != nullptr;
    }
    return MMGPU_OK;
}

// consecutive chunks of whole queries with at most pair_budget pairs each; a query whose slice alone is larger is a chunk of its own
void gscan_cut_chunks(GscanPrepare &S) {
    const uint64_t budget = std::min<uint64_t>(S.par->pair_budget ? S.par->pair_budget : GSCAN_PAIR_BUDGET, 0xFFFFFFF0ull);
    S.qslot.assign(S.nq, 0);
    mmgpu_gscan_batch_t::Chunk cur;
    for (uint32_t i = 0; i < S.nq; i++) {
        if (cur.nq && cur.pairs + S.qcount[i] > budget) {
            S.b->chunks.push_back(cur);
            cur = mmgpu_gscan_batch_t::Chunk();
            cur.q_first = i;
        }
        S.qslot[i] = (uint32_t)cur.pairs;
        cur.pairs += S.qcount[i];
        cur.nq++;
    }
    S.b->chunks.push_back(cur);
    for (const auto &k : S.b->chunks) S.max_chunk_pairs = std::max(S.max_chunk_pairs, k.pairs);
}

// one alignment batch per chunk, over the shared lists and records
int gscan_prepare_chunks(GscanPrepare &S) {
    mmgpu_gscan_batch_t *b = S.b;
    for (DevBuf *d : {&b->d_hit_target, &b->d_hit_out, &b->d_out}) d->bind(S.c->cache);
    const size_t slots = (size_t)std::max<uint64_t>(S.max_chunk_pairs, 1);
    HIP_TRY(b->d_hit_target.alloc(slots * 4));
    HIP_TRY(b->d_hit_out.alloc(slots * 4));
    HIP_TRY(b->d_out.alloc(slots * sizeof(mmgpu_sw_hit)));
    mmgpu_sw_params P;
    P.mat = S.par->mat;
    P.alphabet = S.par->alphabet;
    P.gap_open = S.par->gap_open;
    P.gap_extend = S.par->gap_extend;
    for (auto &k : b->chunks) {
        SwDenseLists D;
        D.begin = S.qbegin.data() + k.q_first;
        D.count = S.qcount.data() + k.q_first;
        D.order = S.order.data();
        D.len_prefix = S.len_prefix.data();
        D.d_hit_target = b->d_hit_target.as<uint32_t>();
        D.d_hit_out = b->d_hit_out.as<uint32_t>();
        D.d_out = b->d_out.as<mmgpu_sw_hit>();
        const int rc = sw_prepare_dense(S.c, &P, S.sw_queries.data() + k.q_first, k.nq, D, &k.sw);
        if (rc != MMGPU_OK) return rc;
        for (hipEvent_t &e : k.ev) HIP_TRY(hipEventCreate(&e));
    }
    return MMGPU_OK;
}

// (after gscan_prepare_chunks: the alignment batches have validated letters and profiles)
void gscan_marshal_identity(GscanPrepare &S) {
    const int alphabet = S.par->alphabet;
    S.qoff.assign(1, 0);
    for (uint32_t i = 0; i < S.nq; i++) {
        const mmgpu_gscan_query &Q = S.qs[i];
        S.qres.insert(S.qres.end(), Q.q, Q.q + Q.qlen);
        if (Q.comp_bias && !Q.profile) S.qcb.insert(S.qcb.end(), Q.comp_bias, Q.comp_bias + Q.qlen);
        else S.qcb.insert(S.qcb.end(), Q.qlen, 0);
        S.qoff.push_back((uint32_t)S.qres.size());
        if (!Q.profile) {
            S.qprof_off.push_back(0xFFFFFFFFu);
            continue;
        }
        // the rows ssw_init keeps (StripedSmithWaterman.cpp:1386-1391): the X row and everything past profile_letters score 0
        S.qprof_off.push_back((uint32_t)S.qprof.size());
        const uint32_t rows = std::min<uint32_t>(Q.profile_letters, (uint32_t)alphabet - 1);
        S.qprof.insert(S.qprof.end(), Q.profile, Q.profile + (size_t)rows * Q.qlen);
        S.qprof.insert(S.qprof.end(), (size_t)((uint32_t)alphabet - rows) * Q.qlen, 0);
    }
}

int gscan_upload(GscanPrepare &S) {
    mmgpu_ctx *c = S.c;
    mmgpu_gscan_batch_t *b = S.b;
    hipStream_t s = c->stream;
    for (DevBuf *d : {&b->d_qres, &b->d_qcb, &b->d_qoff, &b->d_qprof, &b->d_qprof_off, &b->d_qident, &b->d_qwin, &b->d_qminev, &b->d_order,
                      &b->d_qbegin, &b->d_qcount, &b->d_qslot, &b->d_ident_score})
        d->bind(c->cache);
    HIP_TRY(upload(b->d_qres, S.qres, s));
    HIP_TRY(upload(b->d_qcb, S.qcb, s));
    HIP_TRY(upload(b->d_qoff, S.qoff, s));
    HIP_TRY(upload(b->d_qprof, S.qprof, s));
    HIP_TRY(upload(b->d_qprof_off, S.qprof_off, s));
    HIP_TRY(upload(b->d_qident, S.qident, s));
    HIP_TRY(upload(b->d_qwin, S.qwin, s));
    HIP_TRY(upload(b->d_qminev, S.qminev, s));
    HIP_TRY(upload(b->d_order, S.order, s));
    HIP_TRY(upload(b->d_qbegin, S.qbegin, s));
    HIP_TRY(upload(b->d_qcount, S.qcount, s));
    HIP_TRY(upload(b->d_qslot, S.qslot, s));
    HIP_TRY(b->d_ident_score.alloc((size_t)b->nq * sizeof(int32_t)));
    return scan_upload_common(c, b, S.par->mat);
}

int gscan_prepare_impl(mmgpu_ctx *c, const mmgpu_gscan_params *par, const mmgpu_gscan_query *qs, uint32_t nq, mmgpu_gscan_batch_t **out) {
    GscanPrepare S{c, par, qs, nq};
    int rc = gscan_check_call(S);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mmgpu_gscan_batch_t, GscanBatchFree> b(new mmgpu_gscan_batch_t(), GscanBatchFree{c});
    S.b = b.get();
    scan_fill_header(b.get(), c, nq, par->alphabet, par->min_score, par->max_hits, ++g_gscan_serial);
    rc = gscan_slices(S);
    if (rc != MMGPU_OK) return rc;
    gscan_cut_chunks(S);
    rc = gscan_prepare_chunks(S);
    if (rc != MMGPU_OK) return rc;
    gscan_marshal_identity(S);
    rc = gscan_upload(S);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev_ident));
    HIP_TRY(hipEventCreate(&b->ev1));
    *out = b.release();
    return MMGPU_OK;
}

int gscan_launch_identity(mmgpu_ctx *c, mmgpu_gscan_batch_t *b) {
    GscanIdentArgs A;
    A.q_res = b->d_qres.as<uint8_t>();
    A.q_cb = b->d_qcb.as<int8_t>();
    A.q_off = b->d_qoff.as<uint32_t>();
    A.q_prof = b->any_profile ? b->d_qprof.as<int8_t>() : nullptr;
    A.q_prof_off = b->d_qprof_off.as<uint32_t>();
    A.q_ident = b->d_qident.as<uint32_t>();
    A.t_res = c->db.res;
    A.t_off4 = c->db.off4;
    A.mat = b->d_mat.as<int8_t>();
    A.alphabet = b->alphabet;
    A.ident_score = b->d_ident_score.as<int32_t>();
    HIP_TRY(launch_gscan_identity(A, b->nq, c->stream));
    return MMGPU_OK;
}

// planner, alignment kernels, selection of one chunk; the next chunk overwrites the lists and records only behind this one's
// selection (everything is ordered on the context's stream: the alignment groups fork from and join it)
int gscan_launch_chunk(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, mmgpu_gscan_batch_t::Chunk &k) {
    hipStream_t s = c->stream;
    HIP_TRY(hipEventRecord(k.ev[0], s));
    GscanPlanArgs P;
    P.order = b->d_order.as<uint32_t>();
    P.q_begin = b->d_qbegin.as<uint32_t>();
    P.q_count = b->d_qcount.as<uint32_t>();
    P.q_slot = b->d_qslot.as<uint32_t>();
    P.q_first = k.q_first;
    P.n_queries = k.nq;
    P.hit_target = b->d_hit_target.as<uint32_t>();
    P.hit_out = b->d_hit_out.as<uint32_t>();
    if (k.pairs) HIP_TRY(launch_gscan_plan(P, s));
    HIP_TRY(hipEventRecord(k.ev[1], s));
    if (k.pairs)
        if (int rc = sw_run_dense(c, k.sw)) return rc;
    HIP_TRY(hipEventRecord(k.ev[2], s));
    GscanSelectArgs A;
    A.out = b->d_out.as<mmgpu_sw_hit>();
    A.order = P.order;
    A.q_begin = P.q_begin;
    A.q_count = P.q_count;
    A.q_slot = P.q_slot;
    A.q_ident = b->d_qident.as<uint32_t>();
    A.ident_score = b->d_ident_score.as<int32_t>();
    A.q_min_ev = b->d_qminev.as<int32_t>();
    A.t_len = c->db.len;
    A.q_win = b->d_qwin.as<uint32_t>();
    A.scores = c->gscan_scores.as<int32_t>();
    A.n_targets = b->n_targets;
    A.q_first = k.q_first;
    A.min_score = b->min_score;
    A.max_hits = b->max_hits;
    A.hits = b->d_hits.as<mmgpu_pf_hit>();
    A.stride = b->stride;
    A.counts = b->d_counts.as<uint32_t>();
    HIP_TRY(launch_gscan_select(A, k.nq, s));
    HIP_TRY(hipEventRecord(k.ev[3], s));
    return MMGPU_OK;
}

}  // namespace

extern "C" int mmgpu_gscan_prepare(mmgpu_ctx *c, const mmgpu_gscan_params *par, const mmgpu_gscan_query *qs, uint32_t nq,
                                   mmgpu_gscan_batch_t **out) {
    if (out) *out = nullptr;
    if (!c || !out) return fail(MMGPU_ERR_ARG, "mmgpu_gscan_prepare: NULL argument");
    return gscan_prepare_impl(c, par, qs, nq, out);
}

extern "C" int mmgpu_gscan_run(mmgpu_ctx *c, mmgpu_gscan_batch_t *b) {
    int rc = scan_check_batch("mmgpu_gscan_run", c, b, false);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t score_bytes = (size_t)b->nq * b->n_targets * sizeof(int32_t);
    if (score_bytes > c->gscan_scores.bytes) HIP_TRY(hipStreamSynchronize(c->stream));   // a grown buffer frees the old one
    HIP_TRY(c->gscan_scores.reserve(score_bytes));
    c->gscan_serial = b->serial;
    HIP_TRY(hipEventRecord(b->ev0, c->stream));
    rc = gscan_launch_identity(c, b);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipEventRecord(b->ev_ident, c->stream));
    for (auto &k : b->chunks) {
        rc = gscan_launch_chunk(c, b, k);
        if (rc != MMGPU_OK) return rc;
    }
    HIP_TRY(hipEventRecord(b->ev1, c->stream));
    b->ran = true;
    return MMGPU_OK;
}

extern "C" int mmgpu_gscan_fetch(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, mmgpu_pf_hit *hits, uint32_t hit_stride, uint32_t *counts) {
    return scan_fetch_lists("mmgpu_gscan_fetch", c, b, hits, hit_stride, counts, hipMemcpyDeviceToHost);
}

extern "C" int mmgpu_gscan_fetch_device(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, void *d_hits, uint32_t hit_stride, void *d_counts) {
    return scan_fetch_lists("mmgpu_gscan_fetch_device", c, b, d_hits, hit_stride, d_counts, hipMemcpyDeviceToDevice);
}

extern "C" int mmgpu_gscan_last_kernel_ms(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, float *ms) {
    return scan_kernel_ms("mmgpu_gscan_last_kernel_ms", c, b, ms);
}

extern "C" int mmgpu_gscan_stage_ms(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, float ms[4], uint32_t *n_chunks) {
    int rc = scan_check_batch("mmgpu_gscan_stage_ms", c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!ms) return fail(MMGPU_ERR_ARG, "mmgpu_gscan_stage_ms: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(b->ev1));
    ms[0] = ms[1] = ms[2] = ms[3] = 0;
    HIP_TRY(hipEventElapsedTime(&ms[2], b->ev0, b->ev_ident));
    for (const auto &k : b->chunks) {
        const int stage[3] = {0, 1, 3};      // planner, alignment kernels, selection
        for (int z = 0; z < 3; z++) {
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, k.ev[z], k.ev[z + 1]));
            ms[stage[z]] += t;
        }
    }
    if (n_chunks) *n_chunks = (uint32_t)b->chunks.size();
    return MMGPU_OK;
}

extern "C" void mmgpu_gscan_free(mmgpu_ctx *c, mmgpu_gscan_batch_t *b) {
    if (!b) return;
    scan_sync_for_free(c);
    b->release(c);
    delete b;
}

extern "C" int mmgpu_gscan_batch(mmgpu_ctx *c, const mmgpu_gscan_params *par, const mmgpu_gscan_query *qs, uint32_t nq, mmgpu_pf_hit *hits,
                                 uint32_t hit_stride, uint32_t *counts) {
    mmgpu_gscan_batch_t *b = nullptr;
    int rc = mmgpu_gscan_prepare(c, par, qs, nq, &b);
    if (rc != MMGPU_OK) return rc;
    rc = mmgpu_gscan_run(c, b);
    if (rc == MMGPU_OK) rc = mmgpu_gscan_fetch(c, b, hits, hit_stride, counts);
    mmgpu_gscan_free(c, b);
    return rc;
}

extern "C" int mmgpu_gscan_debug_scores(mmgpu_ctx *c, mmgpu_gscan_batch_t *b, uint32_t query, int32_t *out, size_t cap) {
    return scan_debug_scores("mmgpu_gscan_debug_scores", "gapped scan", c, b, &mmgpu_ctx::gscan_serial, &mmgpu_ctx::gscan_scores, sizeof(int32_t),
                             query, out, cap);
}
