// Host side of the ungapped diagonal rescoring (include/mmgpu.h, "ungapped diagonal rescoring"): the validation of a batch, the
// padded copy of its queries, the per-hit query index cut from the CSR offsets, the launch of rescore_kernel.hip, the fetches - and
// mmgpu_host_rescore_accept, the acceptance rule of rescorediagonal.cpp:255-330 on the host.  prepare is a sequence of named steps
// over one record, in the manner of gscan_api.hip.
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mmgpu_internal.h"

using namespace mmgpu;

struct mmgpu_rescore_batch_t {
    uint32_t nq = 0, n_hits = 0, n_targets = 0;
    int mode = 0, alphabet = 0;
    const uint8_t *db_res = nullptr;      // the resident database the batch was prepared against (a reload invalidates the batch)
    bool ran = false;
    bool db_queries = false;              // mmgpu_kmermatch_rescore_prepare: the queries are the resident sequences themselves
    DevBuf d_qres, d_qoff4, d_qlen, d_mat, d_hit_query, d_pairs, d_out;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // around the last run
    ~mmgpu_rescore_batch_t() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace {

// what prepare builds on the host before anything is uploaded
struct RescorePrepare {
    mmgpu_ctx *c;
    const mmgpu_rescore_params *par;
    const mmgpu_rescore_query *qs;
    uint32_t nq;
    const uint64_t *hit_off;
    const mmgpu_rescore_pair *pairs;
    std::vector<uint8_t> qres;              // every query on a 4-byte boundary, RESCORE_SLACK bytes behind the last
    std::vector<uint32_t> qoff4, qlen, hit_query;
};

int rescore_check_call(const RescorePrepare &S) {
    const char *who = "mmgpu_rescore_prepare";
    if (!S.par || !S.qs || !S.nq || !S.hit_off || !S.par->mat) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument or no queries");
    if (!S.c->db.res || S.c->db.n == 0) return fail(MMGPU_ERR_STATE, std::string(who) + ": no targets loaded");
    if (S.c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": the context holds a shard of a multi-GPU run");
    if (S.par->alphabet != 21 || S.c->db.alphabet != 21)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": protein sequences only (alphabet 21, parameters and resident targets alike)");
    if (S.par->mode == 3 || S.par->mode == 4)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": --rescore-mode 3 and 4 trim a leading or trailing '*', which numeric residues cannot tell from X");
    if (S.par->mode < 0 || S.par->mode > 4) return fail(MMGPU_ERR_ARG, std::string(who) + ": unknown mode");
    return MMGPU_OK;
}

int rescore_check_lists(RescorePrepare &S) {
    const char *who = "mmgpu_rescore_prepare";
    if (S.hit_off[0] != 0) return fail(MMGPU_ERR_ARG, std::string(who) + ": hit_off[0] must be 0");
    for (uint32_t i = 0; i < S.nq; i++)
        if (S.hit_off[i + 1] < S.hit_off[i]) return fail(MMGPU_ERR_ARG, std::string(who) + ": hit_off does not ascend");
    const uint64_t total = S.hit_off[S.nq];
    if (total >= (1ull << 31)) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": 2^31 hits or more: send smaller batches");
    if (total && !S.pairs) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    for (uint64_t h = 0; h < total; h++)
        if (S.pairs[h].target >= S.c->db.n) return fail(MMGPU_ERR_ARG, std::string(who) + ": target id outside the database");
    S.hit_query.resize((size_t)total);
    for (uint32_t i = 0; i < S.nq; i++)
        for (uint64_t h = S.hit_off[i]; h < S.hit_off[i + 1]; h++) S.hit_query[(size_t)h] = i;
    return MMGPU_OK;
}

int rescore_marshal_queries(RescorePrepare &S) {
    const char *who = "mmgpu_rescore_prepare";
    uint64_t bytes = RESCORE_SLACK;
    for (uint32_t i = 0; i < S.nq; i++) {
        if (S.qs[i].qlen == 0 || !S.qs[i].q) return fail(MMGPU_ERR_ARG, std::string(who) + ": empty query");
        bytes += ((uint64_t)S.qs[i].qlen + 3) / 4 * 4;
    }
    if (bytes >= (1ull << 32)) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": 4 GiB of query residues or more: send smaller batches");
    S.qres.assign((size_t)bytes, 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < S.nq; i++) {
        const mmgpu_rescore_query &Q = S.qs[i];
        for (uint32_t p = 0; p < Q.qlen; p++)
            if (Q.q[p] >= (uint32_t)S.par->alphabet) return fail(MMGPU_ERR_ARG, std::string(who) + ": query letter outside the alphabet");
        memcpy(S.qres.data() + at, Q.q, Q.qlen);
        S.qoff4.push_back((uint32_t)(at / 4));
        S.qlen.push_back(Q.qlen);
        at += ((uint64_t)Q.qlen + 3) / 4 * 4;
    }
    return MMGPU_OK;
}

int rescore_upload(RescorePrepare &S, mmgpu_rescore_batch_t *b) {
    mmgpu_ctx *c = S.c;
    hipStream_t s = c->stream;
    for (DevBuf *d : {&b->d_qres, &b->d_qoff4, &b->d_qlen, &b->d_mat, &b->d_hit_query, &b->d_pairs, &b->d_out}) d->bind(c->cache);
    const std::vector<int8_t> mat(S.par->mat, S.par->mat + (size_t)S.par->alphabet * S.par->alphabet);
    const std::vector<mmgpu_rescore_pair> pairs(S.pairs, S.pairs + (S.pairs ? b->n_hits : 0));
    HIP_TRY(upload(b->d_qres, S.qres, s));
    HIP_TRY(upload(b->d_qoff4, S.qoff4, s));
    HIP_TRY(upload(b->d_qlen, S.qlen, s));
    HIP_TRY(upload(b->d_mat, mat, s));
    HIP_TRY(upload(b->d_hit_query, S.hit_query, s));
    HIP_TRY(upload(b->d_pairs, pairs, s));
    HIP_TRY(b->d_out.alloc(std::max<size_t>(b->n_hits, 1) * sizeof(mmgpu_rescore_hit)));
    HIP_TRY(hipStreamSynchronize(s));      // the host vectors go with this call
    return MMGPU_OK;
}

int rescore_prepare_impl(mmgpu_ctx *c, const mmgpu_rescore_params *par, const mmgpu_rescore_query *qs, uint32_t nq, const uint64_t *hit_off,
                         const mmgpu_rescore_pair *pairs, mmgpu_rescore_batch_t **out) {
    RescorePrepare S{c, par, qs, nq, hit_off, pairs};
    int rc = rescore_check_call(S);
    if (rc != MMGPU_OK) return rc;
    rc = rescore_check_lists(S);
    if (rc != MMGPU_OK) return rc;
    rc = rescore_marshal_queries(S);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mmgpu_rescore_batch_t> b(new mmgpu_rescore_batch_t());
    b->nq = nq;
    b->n_hits = (uint32_t)hit_off[nq];
    b->n_targets = c->db.n;
    b->mode = par->mode;
    b->alphabet = par->alphabet;
    b->db_res = c->db.res;
    rc = rescore_upload(S, b.get());
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
    *out = b.release();
    return MMGPU_OK;
}

int rescore_check_batch(const char *who, const mmgpu_ctx *c, const mmgpu_rescore_batch_t *b, bool must_have_run) {
    if (!c || !b) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (b->db_res != c->db.res || b->n_targets != c->db.n) return fail(MMGPU_ERR_STATE, std::string(who) + ": the targets were reloaded since the batch was prepared");
    if (must_have_run && !b->ran) return fail(MMGPU_ERR_STATE, std::string(who) + ": the batch has not been run");
    return MMGPU_OK;
}

int rescore_fetch(const char *who, mmgpu_ctx *c, mmgpu_rescore_batch_t *b, void *out, hipMemcpyKind kind) {
    const int rc = rescore_check_batch(who, c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!out && b->n_hits) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    if (b->n_hits) HIP_TRY(hipMemcpyAsync(out, b->d_out.p, (size_t)b->n_hits * sizeof(mmgpu_rescore_hit), kind, c->stream));
    if (kind == hipMemcpyDeviceToHost) HIP_TRY(hipStreamSynchronize(c->stream));      // (a device copy stays ordered on the stream)
    return MMGPU_OK;
}

// Util::computeSeqId (Util.cpp:597-607)
float rescore_seq_id(int seq_id_mode, int ids, int qlen, int tlen, int aln_len) {
    switch (seq_id_mode) {
    case 1: return static_cast<float>(ids) / static_cast<float>(std::min(qlen, tlen));
    case 2: return static_cast<float>(ids) / static_cast<float>(std::max(qlen, tlen));
    case 0: return static_cast<float>(ids) / static_cast<float>(aln_len);
    }
    return 0.0f;
}

// SmithWaterman::computeCov (StripedSmithWaterman.cpp:1762-1764)
float rescore_cov(unsigned start, unsigned end, unsigned len) {
    return (std::min(len, std::max(start, end)) - std::min(start, end) + 1) / (float)len;
}

// Util::hasCoverage (Util.cpp:561-576)
bool rescore_has_coverage(float thr, int cov_mode, float q_cov, float t_cov) {
    switch (cov_mode) {
    case 0: return q_cov >= thr && t_cov >= thr;
    case 2: return q_cov >= thr;
    case 1: return t_cov >= thr;
    default: return true;
    }
}

}  // namespace

extern "C" int mmgpu_rescore_prepare(mmgpu_ctx *c, const mmgpu_rescore_params *par, const mmgpu_rescore_query *qs, uint32_t nq, const uint64_t *hit_off,
                                     const mmgpu_rescore_pair *pairs, mmgpu_rescore_batch_t **out) {
    if (out) *out = nullptr;
    if (!c || !out) return fail(MMGPU_ERR_ARG, "mmgpu_rescore_prepare: NULL argument");
    return rescore_prepare_impl(c, par, qs, nq, hit_off, pairs, out);
}

// the hit list of a k-mer matching batch, handed over on the device: hit_query and the pairs are cut from its CSR by a kernel
extern "C" int mmgpu_kmermatch_rescore_prepare(mmgpu_ctx *c, const mmgpu_rescore_params *par, mmgpu_kmermatch_batch_t *km, mmgpu_rescore_batch_t **out) {
    const char *who = "mmgpu_kmermatch_rescore_prepare";
    if (out) *out = nullptr;
    if (!c || !out || !km || !par || !par->mat) return fail(MMGPU_ERR_ARG, std::string(who) + ": NULL argument");
    if (!c->db.res || c->db.n == 0) return fail(MMGPU_ERR_STATE, std::string(who) + ": no targets loaded");
    if (c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": the context holds a shard of a multi-GPU run");
    if (par->alphabet != 21 || c->db.alphabet != 21)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": protein sequences only (alphabet 21, parameters and resident targets alike)");
    if (par->mode == 3 || par->mode == 4)
        return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": --rescore-mode 3 and 4 trim a leading or trailing '*', which numeric residues cannot tell from X");
    if (par->mode < 0 || par->mode > 4) return fail(MMGPU_ERR_ARG, std::string(who) + ": unknown mode");
    if (km->db_res != c->db.res || km->n != c->db.n) return fail(MMGPU_ERR_STATE, std::string(who) + ": the targets were reloaded since the k-mer matching batch was prepared");
    if (!km->ran) return fail(MMGPU_ERR_STATE, std::string(who) + ": the k-mer matching batch has not been run");
    const uint64_t total = (uint64_t)km->n + km->n_kept;
    if (total >= (1ull << 31)) return fail(MMGPU_ERR_UNSUPPORTED, std::string(who) + ": 2^31 hits or more");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mmgpu_rescore_batch_t> b(new mmgpu_rescore_batch_t());
    b->nq = c->db.n;
    b->n_hits = (uint32_t)total;
    b->n_targets = c->db.n;
    b->mode = par->mode;
    b->alphabet = par->alphabet;
    b->db_res = c->db.res;
    b->db_queries = true;
    for (DevBuf *d : {&b->d_mat, &b->d_hit_query, &b->d_pairs, &b->d_out}) d->bind(c->cache);
    const std::vector<int8_t> mat(par->mat, par->mat + (size_t)par->alphabet * par->alphabet);
    HIP_TRY(upload(b->d_mat, mat, c->stream));
    HIP_TRY(b->d_hit_query.alloc((size_t)b->n_hits * sizeof(uint32_t)));
    HIP_TRY(b->d_pairs.alloc((size_t)b->n_hits * sizeof(mmgpu_rescore_pair)));
    HIP_TRY(b->d_out.alloc((size_t)b->n_hits * sizeof(mmgpu_rescore_hit)));
    HIP_TRY(launch_kmm_handover(km->d_offsets.as<unsigned long long>(), km->n, km->d_records.as<mmgpu_pf_hit>(), b->n_hits, b->d_hit_query.as<uint32_t>(),
                                b->d_pairs.as<mmgpu_rescore_pair>(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // the host copy of the matrix goes with this call
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
    *out = b.release();
    return MMGPU_OK;
}

extern "C" int mmgpu_rescore_run(mmgpu_ctx *c, mmgpu_rescore_batch_t *b) {
    const int rc = rescore_check_batch("mmgpu_rescore_run", c, b, false);
    if (rc != MMGPU_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    RescoreArgs A;
    A.q_res = b->db_queries ? c->db.res : b->d_qres.as<uint8_t>();      // (the database's tail slack exceeds RESCORE_SLACK)
    A.q_off4 = b->db_queries ? c->db.off4 : b->d_qoff4.as<uint32_t>();
    A.q_len = b->db_queries ? c->db.len : b->d_qlen.as<uint32_t>();
    A.t_res = c->db.res;
    A.t_off4 = c->db.off4;
    A.t_len = c->db.len;
    A.mat = b->d_mat.as<int8_t>();
    A.alphabet = b->alphabet;
    A.hit_query = b->d_hit_query.as<uint32_t>();
    A.pairs = b->d_pairs.as<mmgpu_rescore_pair>();
    A.n_hits = b->n_hits;
    A.out = b->d_out.as<mmgpu_rescore_hit>();
    HIP_TRY(hipEventRecord(b->ev0, c->stream));
    HIP_TRY(launch_rescore(A, b->mode, c->stream));
    HIP_TRY(hipEventRecord(b->ev1, c->stream));
    b->ran = true;
    return MMGPU_OK;
}

extern "C" int mmgpu_rescore_fetch(mmgpu_ctx *c, mmgpu_rescore_batch_t *b, mmgpu_rescore_hit *out) {
    return rescore_fetch("mmgpu_rescore_fetch", c, b, out, hipMemcpyDeviceToHost);
}

extern "C" int mmgpu_rescore_fetch_device(mmgpu_ctx *c, mmgpu_rescore_batch_t *b, void *d_out) {
    return rescore_fetch("mmgpu_rescore_fetch_device", c, b, d_out, hipMemcpyDeviceToDevice);
}

extern "C" int mmgpu_rescore_last_kernel_ms(mmgpu_ctx *c, mmgpu_rescore_batch_t *b, float *ms) {
    const int rc = rescore_check_batch("mmgpu_rescore_last_kernel_ms", c, b, true);
    if (rc != MMGPU_OK) return rc;
    if (!ms) return fail(MMGPU_ERR_ARG, "mmgpu_rescore_last_kernel_ms: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(b->ev1));
    HIP_TRY(hipEventElapsedTime(ms, b->ev0, b->ev1));
    return MMGPU_OK;
}

extern "C" void mmgpu_rescore_free(mmgpu_ctx *c, mmgpu_rescore_batch_t *b) {
    if (!b) return;
    scan_sync_for_free(c);      // nothing of the batch is in flight
    delete b;
}

extern "C" int mmgpu_rescore_batch(mmgpu_ctx *c, const mmgpu_rescore_params *par, const mmgpu_rescore_query *qs, uint32_t nq, const uint64_t *hit_off,
                                   const mmgpu_rescore_pair *pairs, mmgpu_rescore_hit *out) {
    mmgpu_rescore_batch_t *b = nullptr;
    int rc = mmgpu_rescore_prepare(c, par, qs, nq, hit_off, pairs, &b);
    if (rc != MMGPU_OK) return rc;
    rc = mmgpu_rescore_run(c, b);
    if (rc == MMGPU_OK) rc = mmgpu_rescore_fetch(c, b, out);
    mmgpu_rescore_free(c, b);
    return rc;
}

// rescorediagonal.cpp:247-330, statement for statement: the reference's variable names, its types (float coverages and score per
// column, double seqId and evalue, int lengths), its order of evaluation
extern "C" int mmgpu_host_rescore_accept(const mmgpu_rescore_hit *rec, uint32_t qlen, uint32_t tlen, int is_identity, double evalue_of_score,
                                         const mmgpu_rescore_accept_params *par, mmgpu_rescore_verdict *out) {
    if (!rec || !par || !out || qlen == 0 || tlen == 0) return fail(MMGPU_ERR_ARG, "mmgpu_host_rescore_accept: NULL argument or empty sequence");
    if (par->mode < MMGPU_RESCORE_HAMMING || par->mode > MMGPU_RESCORE_ALIGNMENT) return fail(MMGPU_ERR_ARG, "mmgpu_host_rescore_accept: mode must be 0, 1 or 2");
    const int origQueryLen = (int)qlen, dbLen = (int)tlen;
    const unsigned int distanceToDiagonal = (unsigned int)std::abs(rec->diagonal);
    const int diagonalLen = (int)rec->diag_len;
    const int distance = rec->score;
    const int diagonal = rec->diagonal;
    double seqId = 0;
    double evalue = 0.0;
    int alnLen = 0;
    float targetCov = static_cast<float>(diagonalLen) / static_cast<float>(dbLen);
    float queryCov = static_cast<float>(diagonalLen) / static_cast<float>(origQueryLen);
    int qStartPos = 0, qEndPos = 0, dbStartPos = 0, dbEndPos = 0;
    if (par->mode == MMGPU_RESCORE_HAMMING) {
        const int idCnt = (static_cast<float>(distance));
        seqId = rescore_seq_id(par->seq_id_mode, idCnt, origQueryLen, dbLen, diagonalLen);
        alnLen = diagonalLen;
    } else {
        evalue = evalue_of_score;
        if (par->mode == MMGPU_RESCORE_ALIGNMENT) {
            alnLen = (rec->end - rec->start) + 1;
            if (diagonal >= 0) {
                qStartPos = rec->start + distanceToDiagonal;
                qEndPos = rec->end + distanceToDiagonal;
                dbStartPos = rec->start;
                dbEndPos = rec->end;
            } else {
                qStartPos = rec->start;
                qEndPos = rec->end;
                dbStartPos = rec->start + distanceToDiagonal;
                dbEndPos = rec->end + distanceToDiagonal;
            }
            if (evalue <= par->evalue_thr || is_identity) seqId = rescore_seq_id(par->seq_id_mode, (int)rec->ident, origQueryLen, dbLen, alnLen);
            queryCov = rescore_cov(qStartPos, qEndPos, origQueryLen);
            targetCov = rescore_cov(dbStartPos, dbEndPos, dbLen);
        }
    }
    const float currScorePerCol = static_cast<float>(distance) / static_cast<float>(diagonalLen);
    const bool hasCov = rescore_has_coverage(par->cov_thr, par->cov_mode, queryCov, targetCov);
    const bool hasSeqId = seqId >= (par->seq_id_thr - FLT_EPSILON);
    const bool hasEvalue = (evalue <= par->evalue_thr);
    const bool hasAlnLen = (alnLen >= par->min_aln_len);
    const bool hasToFilter = (par->filter_hits != 0 && currScorePerCol >= par->score_per_col_thr);
    out->accepted = (is_identity || hasToFilter || (hasAlnLen && hasCov && hasSeqId && hasEvalue)) ? 1 : 0;
    out->aln_len = alnLen;
    out->seq_id = (float)seqId;
    out->q_cov = queryCov;
    out->t_cov = targetCov;
    out->q_start = qStartPos;
    out->q_end = qEndPos;
    out->t_start = dbStartPos;
    out->t_end = dbEndPos;
    return MMGPU_OK;
}
