// Host side of the prefilter's k-mer index: the host builders of its tables (score matrices, index), the index made resident from
// host arrays or built in HBM (ix_kernels.hip), and what is derived from it on the device.  See include/mmgpu.h for the contract.
#include <atomic>
#include <cstring>

#include "pf_index.h"

using namespace mmgpu;

// spaced_seed_<k> of Sequence.h:20-50 as bit masks (bit i = pattern position i) and their lengths
static const uint32_t SPACED_BITS[16] = {0, 0, 0, 0, 0x17u, 0xA13u, 0x32Bu, 0x66Bu, 0xCEBu, 0x366Bu, 0x6D6Bu, 0x1B66Bu, 0x6B66Bu, 0xD6CEBu,
                                         0x1B6CEBu, 0x6D1BD7u};
static const uint8_t SPACED_LEN[16] = {0, 0, 0, 0, 5, 12, 10, 11, 12, 14, 15, 17, 19, 20, 21, 23};

static int window_pattern(int k, int spaced, uint8_t *pat) {     // k in [4, 15]
    if (!spaced) {
        for (int i = 0; i < k; i++) pat[i] = (uint8_t)i;
        return k;
    }
    const int n = SPACED_LEN[k];
    int c = 0;
    for (int i = 0; i < n; i++)
        if ((SPACED_BITS[k] >> i) & 1u) pat[c++] = (uint8_t)i;
    return n;
}

// ---------------------------------------------------------------------------------------------------------
// ExtendedSubstitutionMatrix::calcScoreMatrix (src/prefiltering/ExtendedSubstitutionMatrix.cpp:20-71).  Row r lists
// every span-mer by descending score; the reference uses std::stable_sort over the cartesian-product enumeration
// (first residue slowest, :103-128).  Scores are small integers, so a stable counting sort per row does the same.
extern "C" int mmgpu_host_score_matrix(const int16_t *submat, int alphabet, int span, int16_t *score, uint32_t *index) {
    return mmgpu_host_score_matrix_rows(submat, alphabet, span, 0, score, index);
}

// the same into rows of row_stride elements (ScoreMatrix::rowSize: the reference pads its rows for SIMD loads, :24-25; the
// padding elements are the caller's); row_stride 0 = (alphabet - 1)^span, no padding
extern "C" int mmgpu_host_score_matrix_rows(const int16_t *submat, int alphabet, int span, size_t row_stride, int16_t *score, uint32_t *index) {
    if (!submat || !score || !index) return fail(MMGPU_ERR_ARG, "mmgpu_host_score_matrix: NULL argument");
    if (alphabet < 3 || alphabet > 32 || span < 1 || span > 3) return fail(MMGPU_ERR_ARG, "mmgpu_host_score_matrix: bad alphabet/span");
    const int ka = alphabet - 1;
    size_t n = 1;
    for (int i = 0; i < span; i++) n *= (size_t)ka;
    const size_t stride = row_stride ? row_stride : n;
    if (stride < n) return fail(MMGPU_ERR_ARG, "mmgpu_host_score_matrix_rows: row_stride smaller than the row");
    // enumeration e -> (index in int2index order, residues)
    std::vector<uint32_t> e2idx(n);
    std::vector<uint8_t> e2res(n * (size_t)span);
    for (size_t e = 0; e < n; e++) {
        size_t t = e;
        for (int p = span - 1; p >= 0; p--) {
            e2res[e * span + p] = (uint8_t)(t % (size_t)ka);
            t /= (size_t)ka;
        }
        size_t idx = 0, pw = 1;
        for (int p = 0; p < span; p++) {
            idx += e2res[e * span + p] * pw;
            pw *= (size_t)ka;
        }
        e2idx[e] = (uint32_t)idx;
    }
    int lo = 0, hi = 0;
    for (int a = 0; a < ka; a++)
        for (int b = 0; b < ka; b++) {
            lo = std::min<int>(lo, submat[a * alphabet + b]);
            hi = std::max<int>(hi, submat[a * alphabet + b]);
        }
    const int smin = lo * span, smax = hi * span, range = smax - smin + 1;
    parallel_for(n, [&](size_t r0, size_t r1) {
        std::vector<int16_t> sc(n);
        std::vector<uint32_t> cursor((size_t)range + 1);
        for (size_t e = r0; e < r1; e++) {
            const uint8_t *a = &e2res[e * span];
            std::fill(cursor.begin(), cursor.end(), 0u);
            for (size_t f = 0; f < n; f++) {
                const uint8_t *b = &e2res[f * span];
                int s = 0;
                for (int p = 0; p < span; p++) s += submat[a[p] * alphabet + b[p]];
                sc[f] = (int16_t)s;
                cursor[(size_t)(smax - s) + 1]++;   // bucket 0 = highest score
            }
            for (int z = 0; z < range; z++) cursor[(size_t)z + 1] += cursor[z];
            int16_t *srow = score + (size_t)e2idx[e] * stride;
            uint32_t *irow = index + (size_t)e2idx[e] * stride;
            for (size_t f = 0; f < n; f++) {
                const uint32_t o = cursor[(size_t)(smax - sc[f])]++;
                srow[o] = sc[f];
                irow[o] = e2idx[f];
            }
        }
    });
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// IndexTable::addKmerCount / addSequence / sortDBSeqLists (src/prefiltering/IndexTable.h:135-191,350-403) as
// IndexBuilder::fillDatabase drives them with masking off (IndexBuilder.cpp:118-166,226-270).
namespace {
struct KmerWindows {
    int k, ka, alphabet, plen, thr;
    uint8_t pat[16];
    int8_t self[32];   // (char) subMatrix[a][a], IndexBuilder.cpp:11-22
    // unique k-mers of one target with their first position, sorted by k-mer; key = kmer << 16 | pos
    void extract(const uint8_t *s, uint64_t len, std::vector<uint64_t> &buf) const {
        buf.clear();
        for (uint64_t i = 0; i + (uint64_t)plen <= len; i++) {
            uint64_t idx = 0, pw = 1;
            int sc = 0;
            bool x = false;
            for (int p = 0; p < k; p++) {
                const uint8_t r = s[i + pat[p]];
                if (r >= ka) { x = true; break; }
                idx += r * pw;
                pw *= (uint64_t)ka;
                sc += self[r];
            }
            if (x || (thr > 0 && sc < thr)) continue;
            buf.push_back((idx << 16) | (i & 0xFFFFu));
        }
        std::sort(buf.begin(), buf.end());
        size_t w = 0;
        uint64_t prev = ~0ull;
        for (size_t z = 0; z < buf.size(); z++) {
            if ((buf[z] >> 16) != prev) buf[w++] = buf[z];
            prev = buf[z] >> 16;
        }
        buf.resize(w);
    }
};
}  // namespace

extern "C" int mmgpu_host_index_build(const uint8_t *residues, const uint64_t *seq_off, uint32_t n, const int16_t *kmer_submat,
                                      int alphabet, int k, int spaced, int kmer_thr, uint64_t *offsets, uint32_t *ids,
                                      uint16_t *pos, uint64_t *n_entries) {
    if (!residues || !seq_off || !kmer_submat || !offsets || !n_entries)
        return fail(MMGPU_ERR_ARG, "mmgpu_host_index_build: NULL argument");
    if ((k < 5 || k > 7) || alphabet < 3 || alphabet > 32) return fail(MMGPU_ERR_ARG, "mmgpu_host_index_build: bad k/alphabet");
    if ((ids == nullptr) != (pos == nullptr)) return fail(MMGPU_ERR_ARG, "mmgpu_host_index_build: ids and pos go together");
    KmerWindows W;
    W.k = k;
    W.ka = alphabet - 1;
    W.alphabet = alphabet;
    W.thr = kmer_thr;
    W.plen = window_pattern(k, spaced, W.pat);
    for (int a = 0; a < alphabet; a++) W.self[a] = (int8_t)(char)kmer_submat[a * alphabet + a];
    uint64_t table = 1;
    for (int i = 0; i < k; i++) table *= (uint64_t)W.ka;
    std::vector<std::atomic<uint32_t>> cnt(table);
    for (auto &c : cnt) c.store(0, std::memory_order_relaxed);
    parallel_for(n, [&](size_t a, size_t b) {
        std::vector<uint64_t> buf;
        for (size_t t = a; t < b; t++) {
            W.extract(residues + seq_off[t], seq_off[t + 1] - seq_off[t], buf);
            for (uint64_t v : buf) cnt[v >> 16].fetch_add(1, std::memory_order_relaxed);
        }
    });
    uint64_t run = 0;
    for (uint64_t z = 0; z < table; z++) {
        offsets[z] = run;
        run += cnt[z].load(std::memory_order_relaxed);
    }
    offsets[table] = run;
    *n_entries = run;
    if (!ids) return MMGPU_OK;
    for (auto &c : cnt) c.store(0, std::memory_order_relaxed);
    parallel_for(n, [&](size_t a, size_t b) {
        std::vector<uint64_t> buf;
        for (size_t t = a; t < b; t++) {
            W.extract(residues + seq_off[t], seq_off[t + 1] - seq_off[t], buf);
            for (uint64_t v : buf) {
                const uint64_t o = offsets[v >> 16] + cnt[v >> 16].fetch_add(1, std::memory_order_relaxed);
                ids[o] = (uint32_t)t;
                pos[o] = (uint16_t)(v & 0xFFFFu);
            }
        }
    });
    // sortDBSeqLists: every list by (seqId, position); one entry per (k-mer, target), so seqId alone decides
    parallel_for(table, [&](size_t a, size_t b) {
        std::vector<uint64_t> tmp;
        for (size_t z = a; z < b; z++) {
            const uint64_t o0 = offsets[z], o1 = offsets[z + 1];
            if (o1 - o0 < 2) continue;
            tmp.resize(o1 - o0);
            for (uint64_t e = o0; e < o1; e++) tmp[e - o0] = ((uint64_t)ids[e] << 16) | pos[e];
            std::sort(tmp.begin(), tmp.end());
            for (uint64_t e = o0; e < o1; e++) {
                ids[e] = (uint32_t)(tmp[e - o0] >> 16);
                pos[e] = (uint16_t)(tmp[e - o0] & 0xFFFFu);
            }
        }
    });
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// tables every QueryMatcher gets (score matrices, cumulative counts, ungapped matrix): shared by the three ways of obtaining
// the index (host arrays / built in HBM / read from a database file).  `from_host` = validate and copy the host index as well.
namespace {
int fail_who(int code, const char *who, const std::string &body) { return fail(code, std::string(who) + ": " + body); }

// what can be told from the descriptor's own fields; *kbase_out: base of the k-mer index
int check_descriptor(const char *who, const DeviceDb &db, const mmgpu_pf_index *ix, bool from_host, int *kbase_out) {
    if (!ix) return fail_who(MMGPU_ERR_ARG, who, "NULL argument");
    if (!db.res) return fail_who(MMGPU_ERR_STATE, who, "load the targets (SequenceLookup) first");
    const bool tables = ix->score3 != nullptr && ix->index3 != nullptr;    // without them: exact k-mer matching only
    if (tables && (ix->kmer_size < 5 || ix->kmer_size > 7)) return fail_who(MMGPU_ERR_UNSUPPORTED, who, "similar k-mers need k = 5, 6 or 7");
    if (ix->kmer_size < 4 || ix->kmer_size > 15) return fail_who(MMGPU_ERR_UNSUPPORTED, who, "k must be in [4, 15]");
    if (tables && ix->kmer_size != 6 && (!ix->score2 || !ix->index2)) return fail_who(MMGPU_ERR_ARG, who, "k = 5 and k = 7 need the 2-mer ScoreMatrix");
    if (ix->alphabet != db.alphabet) return fail_who(MMGPU_ERR_ARG, who, "alphabet differs from the loaded targets");
    if (ix->alphabet < 2 || ix->alphabet > 32) return fail_who(MMGPU_ERR_ARG, who, "alphabet must be in [2, 32]");
    if (!ix->ungapped_mat) return fail_who(MMGPU_ERR_ARG, who, "NULL table");
    const int kbase = (from_host && ix->kmer_alphabet > 0) ? ix->kmer_alphabet : ix->alphabet - 1;
    if (kbase < ix->alphabet - 1 || kbase > ix->alphabet) return fail_who(MMGPU_ERR_ARG, who, "kmer_alphabet must be alphabet - 1 or alphabet");
    double tb = 1;
    for (int i = 0; i < ix->kmer_size; i++) tb *= (double)kbase;
    if (tb > 2147483648.0) return fail_who(MMGPU_ERR_UNSUPPORTED, who, "more than 2^31 k-mers");
    if (from_host) {
        if (!ix->offsets) return fail_who(MMGPU_ERR_ARG, who, "NULL table");
        if (!ix->entries6 && !(ix->entry_ids && ix->entry_pos) && ix->n_entries) return fail_who(MMGPU_ERR_ARG, who, "no index entries");
        if (ix->n_entries >= 0xFFFFFFFFull) return fail_who(MMGPU_ERR_UNSUPPORTED, who, ">= 2^32 index entries per shard");
    }
    const size_t ka = (size_t)(ix->alphabet - 1);
    if (tables && ix->row3 < ka * ka * ka) return fail_who(MMGPU_ERR_ARG, who, "row3 smaller than kalph^3");
    if (tables && ix->kmer_size != 6 && ix->row2 < ka * ka) return fail_who(MMGPU_ERR_ARG, who, "row2 smaller than kalph^2");
    *kbase_out = kbase;
    return MMGPU_OK;
}

void fill_header(PfIndex *P, const mmgpu_pf_index *ix, int kbase, bool from_host) {
    P->k = ix->kmer_size;
    P->alphabet = ix->alphabet;
    P->kalph = ix->alphabet - 1;
    P->kbase = kbase;
    P->spaced = ix->spaced;
    P->pattern_len = window_pattern(P->k, P->spaced, P->pat);
    P->n3 = (uint32_t)(P->kalph * P->kalph * P->kalph);
    P->table = 1;
    for (int i = 0; i < P->k; i++) P->table *= (uint64_t)P->kbase;
    P->n_entries = from_host ? ix->n_entries : 0;
    P->has_tables = ix->score3 != nullptr && ix->index3 != nullptr;
    P->h_mat.assign(ix->ungapped_mat, ix->ungapped_mat + ix->alphabet * ix->alphabet);
}

// cumulative counts per row: #entries with score >= c is one lookup instead of a binary search in the row.  `name`: score3 / score2
int build_cum(const char *who, const char *name, const int16_t *score, size_t row_stride, size_t n, std::vector<uint16_t> &cum, uint32_t *w_out,
              int32_t *min_out) {
    // (sorted before the table is sized: its width is first column - last column, which unsorted rows make anything)
    int lo = 32767, hi = -32768;
    for (size_t r = 0; r < n; r++) {
        const int16_t *row = score + r * row_stride;
        for (size_t z = 1; z < n; z++)
            if (row[z] > row[z - 1]) return fail_who(MMGPU_ERR_ARG, who, std::string(name) + " rows are not sorted by descending score");
        lo = std::min<int>(lo, row[n - 1]);
        hi = std::max<int>(hi, row[0]);
    }
    const uint32_t w = (uint32_t)(hi - lo + 2);
    cum.assign(n * (size_t)w, 0);
    for (size_t r = 0; r < n; r++) {
        const int16_t *row = score + r * row_stride;
        size_t j = 0;   // rows are sorted descending: walk thresholds from high to low
        for (int k = (int)w - 1; k >= 0; k--) {
            const int c = lo + k;
            while (j < n && row[j] >= c) j++;
            cum[r * w + (size_t)k] = (uint16_t)j;
        }
    }
    *w_out = w;
    *min_out = lo;
    return MMGPU_OK;
}

int convert_offsets(const char *who, const mmgpu_pf_index *ix, uint64_t table, std::vector<uint32_t> &off32) {
    off32.resize(table + 1);
    std::atomic<bool> bad_off(false);
    parallel_for((size_t)table + 1, [&](size_t a, size_t b) {
        for (size_t z = a; z < b; z++) {
            if (ix->offsets[z] > ix->n_entries || (z && ix->offsets[z] < ix->offsets[z - 1])) bad_off = true;
            off32[z] = (uint32_t)ix->offsets[z];
        }
    });
    return bad_off ? fail_who(MMGPU_ERR_ARG, who, "offsets not monotone / out of range") : MMGPU_OK;
}

int convert_entries(const char *who, const mmgpu_pf_index *ix, uint32_t n_targets, std::vector<uint64_t> &ent) {
    const size_t ne = (size_t)ix->n_entries;
    ent.resize(std::max<size_t>(ne, 1));
    const uint8_t *e6 = (const uint8_t *)ix->entries6;
    std::atomic<bool> bad_ent(false);
    parallel_for(ne, [&](size_t a, size_t b) {
        for (size_t e = a; e < b; e++) {
            uint32_t id;
            uint16_t pj;
            if (ix->entry_ids) {
                id = ix->entry_ids[e];
                pj = ix->entry_pos[e];
            } else {
                memcpy(&id, e6 + e * 6, 4);
                memcpy(&pj, e6 + e * 6 + 4, 2);
            }
            if (id >= n_targets) bad_ent = true;
            ent[e] = (uint64_t)id | ((uint64_t)pj << 32);
        }
    });
    return bad_ent ? fail_who(MMGPU_ERR_ARG, who, "index entry names a target that is not loaded") : MMGPU_OK;
}

// one n x n score table (rows of row_stride elements on the host) with its cumulative counts
hipError_t upload_score_table(const int16_t *score, const uint32_t *index, size_t row_stride, size_t n, const std::vector<uint16_t> &cum, DevBuf &d_s,
                              DevBuf &d_i, DevBuf &d_cum) {
    hipError_t e = d_s.alloc(n * n * sizeof(int16_t));
    if (e == hipSuccess) e = d_i.alloc(n * n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy2D(d_s.p, n * sizeof(int16_t), score, row_stride * sizeof(int16_t), n * sizeof(int16_t), n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy2D(d_i.p, n * sizeof(uint32_t), index, row_stride * sizeof(uint32_t), n * sizeof(uint32_t), n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = upload(d_cum, cum, nullptr);
    return e;
}
}  // namespace

namespace mmgpu {

int pf_index_check(const char *who, const DeviceDb &db, const mmgpu_pf_index *ix, bool from_host, PfIndexDraft &D) {
    int kbase = 0;
    if (int e = check_descriptor(who, db, ix, from_host, &kbase)) return e;
    D.ix = ix;
    D.P.reset(new PfIndex());
    PfIndex *P = D.P.get();
    fill_header(P, ix, kbase, from_host);
    if (P->has_tables)
        if (int e = build_cum(who, "score3", ix->score3, ix->row3, P->n3, D.cum3, &P->cum_w, &P->score_min)) return e;
    if (P->has_tables && P->k != 6)      // k = 5: (2, 3), k = 7: (2, 2, 3) - KmerGenerator::setDivideStrategy
        if (int e = build_cum(who, "score2", ix->score2, ix->row2, (size_t)P->kalph * P->kalph, D.cum2, &P->cum2_w, &P->score2_min)) return e;
    if (from_host) {
        if (int e = convert_offsets(who, ix, P->table, D.off32)) return e;
        if (int e = convert_entries(who, ix, db.n, D.ent)) return e;
    }
    return MMGPU_OK;
}

int pf_index_upload(const char *who, PfIndexDraft &D, std::unique_ptr<PfIndex> &out) {
    PfIndex *P = D.P.get();
    const mmgpu_pf_index *ix = D.ix;
    hipError_t e = hipSuccess;
    if (P->has_tables) e = upload_score_table(ix->score3, ix->index3, ix->row3, P->n3, D.cum3, P->d_s3, P->d_i3, P->d_cum3);
    if (e == hipSuccess && P->has_tables && P->k != 6)
        e = upload_score_table(ix->score2, ix->index2, ix->row2, (size_t)P->kalph * P->kalph, D.cum2, P->d_s2, P->d_i2, P->d_cum2);
    if (e == hipSuccess && !D.off32.empty()) e = upload(P->d_offsets, D.off32, nullptr);
    if (e == hipSuccess && !D.ent.empty()) e = upload(P->d_entries, D.ent, nullptr);
    if (e == hipSuccess) e = upload(P->d_mat, P->h_mat, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();      // the draft's host arrays die with the caller's scope
    if (e != hipSuccess) return fail_who(MMGPU_ERR_HIP, who, std::string("upload failed: ") + hipGetErrorString(e));
    out = std::move(D.P);
    return MMGPU_OK;
}

// Sparse indexes (a shard of a multi-GPU run holds 1/N of the entries over the same k-mer space; small databases): most similar
// k-mers of a query have no list.  The bit table is consulted by pf_kmers_kernel when fewer than 60 % of the k-mers have one
// similar-k-mer searches with k = 6 only (the table of k = 7 has 1.3e9 k-mers).
hipError_t pf_index_bitmap(PfIndex *P, hipStream_t s) {
    P->use_bitmap = false;
    if (!P->has_tables || P->k != 6 || P->table > (1ull << 28)) return hipSuccess;
    DevBuf d_cnt;
    hipError_t rc = P->d_nonempty.alloc(((P->table + 31) / 32 + 1) * 4);
    if (rc == hipSuccess) rc = d_cnt.alloc(8);
    if (rc == hipSuccess) rc = hipMemsetAsync(d_cnt.p, 0, 8, s);
    if (rc == hipSuccess) rc = launch_pf_bitmap(P->d_offsets.as<uint32_t>(), P->table, P->d_nonempty.as<uint32_t>(), d_cnt.as<unsigned long long>(), s);
    unsigned long long n = 0;
    if (rc == hipSuccess) rc = hipMemcpyAsync(&n, d_cnt.p, 8, hipMemcpyDeviceToHost, s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(s);
    if (rc != hipSuccess) return rc;
    P->nonempty_frac = P->table ? (double)n / (double)P->table : 1.0;
    P->use_bitmap = P->nonempty_frac < 0.6;
    if (!P->use_bitmap) P->d_nonempty.release();
    return hipSuccess;
}

// the compact offset table of the similar-k-mer kernels (k = 6 and k = 7 with score tables; not for exact matching, whose one
// look-up per window does not pay for it).  MMGPU_PF_COFS=0 keeps the look-ups on the full table (A/B runs).
hipError_t pf_index_cofs(PfIndex *P, hipStream_t s) {
    P->use_cofs = false;
    if (!P->has_tables || P->n_entries >= (1ull << 31) || P->table > (1ull << 31) || pf_env().cofs_off) return hipSuccess;
    hipError_t rc = P->d_cofs.alloc(pf_cofs_bytes(P->table));
    if (rc == hipSuccess) rc = launch_pf_cofs(P->d_offsets.as<uint32_t>(), P->table, P->d_cofs.p, s);
    if (rc == hipSuccess) P->use_cofs = true;
    return rc;
}

void pf_index_free(mmgpu_ctx *c) {
    if (c && c->pf) {
        delete c->pf;
        c->pf = nullptr;
    }
}

}  // namespace mmgpu

extern "C" int mmgpu_pf_load_index(mmgpu_ctx *c, const mmgpu_pf_index *ix) {
    const char *who = "mmgpu_pf_load_index";
    if (!c) return fail(MMGPU_ERR_ARG, "mmgpu_pf_load_index: NULL argument");
    PfIndexDraft D;
    if (int e = pf_index_check(who, c->db, ix, true, D)) return e;
    HIP_TRY(hipSetDevice(c->device));
    pf_index_free(c);      // (after every check, before the new tables are allocated: both may not fit)
    std::unique_ptr<PfIndex> P;
    if (int e = pf_index_upload(who, D, P)) return e;
    HIP_TRY(pf_index_bitmap(P.get(), c->stream));
    HIP_TRY(pf_index_cofs(P.get(), c->stream));
    c->pf = P.release();
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// IndexBuilder::fillDatabase on the device (ix_kernels.hip): count, scan, scatter, sort every list by seqId.
namespace {
struct IxBuild {
    mmgpu_ctx *c;
    PfIndex *P;
    hipStream_t s;
    IxArgs A;
    uint64_t n_entries = 0;
    std::vector<uint64_t> chbase;      // first entry of every scan chunk (host copy: stays until the stream has passed its upload)
    DevBuf d_counts, d_scratch, d_chunk_off, d_chunk_tot, d_chunk_base, d_tmp, d_long, d_nlong;

    // k-mers per table slot, one entry per (k-mer, target)
    int count(const int16_t *kmer_submat, int kmer_thr) {
        HIP_TRY(d_counts.alloc(P->table * 4));
        HIP_TRY(P->d_offsets.alloc((P->table + 1) * 4));
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, P->table * 4, s));
        memset(&A, 0, sizeof(A));
        A.t_res = c->pf_res();
        A.t_off4 = c->db.off4;
        A.t_len = c->db.len;
        A.n_targets = c->db.n;
        A.k = P->k;
        A.pattern_len = P->pattern_len;
        A.kmer_thr = kmer_thr;
        A.kalph = (uint32_t)P->kalph;
        memcpy(A.pat, P->pat, sizeof(A.pat));
        for (int a = 0; a < P->alphabet && a < 32; a++) A.self_score[a] = (int8_t)(char)kmer_submat[a * P->alphabet + a];
        A.counts = d_counts.as<uint32_t>();
        if ((int)c->db.max_len - P->pattern_len + 1 > 4096) {
            // one uint32 per residue slot of the packed target array
            uint64_t slots = 0;
            for (uint32_t l : c->h_len) slots += ((uint64_t)l + 3) / 4 * 4;
            HIP_TRY(d_scratch.alloc((slots + 64) * 4));
        }
        A.scratch = d_scratch.as<uint32_t>();
        HIP_TRY(launch_ix_target(A, false, s));
        return MMGPU_OK;
    }
    // offsets = exclusive scan of the counts: 64 K chunks, chunk totals summed on the host
    int scan_offsets() {
        const uint64_t table = P->table;
        const uint32_t CH = 65536;
        const uint32_t nch = (uint32_t)((table + CH - 1) / CH);
        std::vector<uint32_t> choff(nch + 1);
        for (uint32_t z = 0; z <= nch; z++) choff[z] = (uint32_t)std::min<uint64_t>((uint64_t)z * CH, table);
        std::vector<uint64_t> chtot(nch);
        chbase.resize(nch);
        HIP_TRY(upload(d_chunk_off, choff, s));
        HIP_TRY(d_chunk_tot.alloc((size_t)nch * 8));
        HIP_TRY(d_chunk_base.alloc((size_t)nch * 8));
        HIP_TRY(launch_pf_scan(d_counts.as<uint32_t>(), d_chunk_off.as<uint32_t>(), nch, nullptr, nullptr, d_chunk_tot.as<uint64_t>(), s));
        HIP_TRY(hipMemcpyAsync(chtot.data(), d_chunk_tot.p, (size_t)nch * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t run = 0;
        for (uint32_t z = 0; z < nch; z++) { chbase[z] = run; run += chtot[z]; }
        if (run >= 0xFFFFFFFFull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_pf_build_index: >= 2^32 index entries per shard");
        n_entries = P->n_entries = run;
        HIP_TRY(hipMemcpyAsync(d_chunk_base.p, chbase.data(), (size_t)nch * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_pf_scan(d_counts.as<uint32_t>(), d_chunk_off.as<uint32_t>(), nch, d_chunk_base.as<uint64_t>(), P->d_offsets.as<uint32_t>(), nullptr, s));
        return MMGPU_OK;
    }
    // the entries in arrival order, into d_tmp
    int scatter() {
        HIP_TRY(d_tmp.alloc(std::max<uint64_t>(n_entries, 1) * 8));
        HIP_TRY(P->d_entries.alloc(std::max<uint64_t>(n_entries, 1) * 8));
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, P->table * 4, s));
        A.offsets = P->d_offsets.as<uint32_t>();
        A.entries = d_tmp.as<uint64_t>();
        HIP_TRY(launch_ix_target(A, true, s));
        return MMGPU_OK;
    }
    // every list by seqId into the index: the short ones in one launch, which lists the long ones for a second
    int sort_lists() {
        IxSortArgs S;
        S.table = P->table;
        S.offsets = P->d_offsets.as<uint32_t>();
        S.src = d_tmp.as<uint64_t>();
        S.dst = P->d_entries.as<uint64_t>();
        S.long_cap = (uint32_t)(n_entries / 17 + 1);
        HIP_TRY(d_long.alloc((size_t)S.long_cap * 4));
        HIP_TRY(d_nlong.alloc(4));
        HIP_TRY(hipMemsetAsync(d_nlong.p, 0, 4, s));
        S.long_lists = d_long.as<uint32_t>();
        S.n_long = d_nlong.as<uint32_t>();
        HIP_TRY(launch_ix_sort_short(S, s));
        uint32_t n_long = 0;
        HIP_TRY(hipMemcpyAsync(&n_long, d_nlong.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(launch_ix_sort_long(S, std::min(n_long, S.long_cap), s));
        HIP_TRY(hipStreamSynchronize(s));
        return MMGPU_OK;
    }
};

}  // namespace

extern "C" int mmgpu_pf_build_index(mmgpu_ctx *c, const mmgpu_pf_index *ix, const int16_t *kmer_submat, int kmer_thr) {
    const char *who = "mmgpu_pf_build_index";
    if (!c || !kmer_submat) return fail(MMGPU_ERR_ARG, "mmgpu_pf_build_index: NULL argument");
    PfIndexDraft D;
    if (int e = pf_index_check(who, c->db, ix, false, D)) return e;
    HIP_TRY(hipSetDevice(c->device));
    pf_index_free(c);      // (after every check, before the new tables are allocated: both may not fit)
    std::unique_ptr<PfIndex> P;
    if (int e = pf_index_upload(who, D, P)) return e;
    IxBuild B{c, P.get(), c->stream};
    if (int e = B.count(kmer_submat, kmer_thr)) return e;
    if (int e = B.scan_offsets()) return e;
    if (int e = B.scatter()) return e;
    if (int e = B.sort_lists()) return e;
    HIP_TRY(pf_index_bitmap(P.get(), c->stream));
    HIP_TRY(pf_index_cofs(P.get(), c->stream));
    c->pf = P.release();
    return MMGPU_OK;
}

// test hook: the resident index as the host builder would return it
extern "C" int mmgpu_pf_debug_index(mmgpu_ctx *c, uint64_t *offsets, uint32_t *ids, uint16_t *pos, uint64_t *n_entries) {
    if (!c || !c->pf || !n_entries) return fail(MMGPU_ERR_ARG, "mmgpu_pf_debug_index: no index");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const PfIndex &P = *c->pf;
    *n_entries = P.n_entries;
    if (offsets) {
        std::vector<uint32_t> o(P.table + 1);
        HIP_TRY(hipMemcpy(o.data(), P.d_offsets.p, (P.table + 1) * 4, hipMemcpyDeviceToHost));
        for (uint64_t z = 0; z <= P.table; z++) offsets[z] = o[z];
    }
    if (ids && pos && P.n_entries) {
        std::vector<uint64_t> e(P.n_entries);
        HIP_TRY(hipMemcpy(e.data(), P.d_entries.p, P.n_entries * 8, hipMemcpyDeviceToHost));
        for (uint64_t z = 0; z < P.n_entries; z++) { ids[z] = (uint32_t)e[z]; pos[z] = (uint16_t)(e[z] >> 32); }
    }
    return MMGPU_OK;
}
