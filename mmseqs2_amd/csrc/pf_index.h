// What a context holds of a target database - the resident targets, their masked view, the k-mer index - as one record with one
// owner, and the prefilter index itself.  Shared by db_api.hip (targets, masked view), pf_index_api.hip (index and its tables),
// db_file.hip (the persisted layout) and pf_api.hip (the batches that read the index).
#ifndef MMGPU_PF_INDEX_H
#define MMGPU_PF_INDEX_H

#include "mmgpu_internal.h"

namespace mmgpu {

struct PfIndex {
    int k = 0, alphabet = 0, kalph = 0, spaced = 0;
    int kbase = 0;               // base of the k-mer index (kalph, or the full alphabet for a handed-over index of profile targets)
    uint8_t pat[16] = {0};
    int pattern_len = 0;
    bool has_tables = false;   // similar-k-mer score tables present (false: exact k-mer matching only)
    uint32_t n3 = 0;
    uint64_t table = 0, n_entries = 0;
    DevBuf d_s3, d_i3, d_cum3, d_s2, d_i2, d_cum2, d_offsets, d_entries, d_mat;
    DevBuf d_cofs;               // compact offset table (pf_cofs_kernel): what the similar-k-mer kernels look lists up in
    bool use_cofs = false;
    DevBuf d_nonempty;           // one bit per k-mer (pf_bitmap_kernel), used when the index is sparse
    bool use_bitmap = false;
    double nonempty_frac = 1.0;  // k-mers with a list / all k-mers
    uint32_t cum_w = 0, cum2_w = 0;
    int32_t score_min = 0, score2_min = 0;
    std::vector<int8_t> h_mat;   // ungapped matrix (host copy for the self score)
    // Large working buffers, shared by all batches of this context (grow-only; batches run one at a time on the
    // context's stream): index lists, split tiles, candidates, survivors.
    DevBuf w_lists, w_split, w_split_hi, w_bin_off, w_cand, w_surv, w_tile_q, w_tile_idx;
    const void *w_owner = nullptr;   // batch whose last run the working buffers hold (debug fetch)
};

// The environment's test hooks of the prefilter, read in this one place, once per call that uses them (they are not part of
// mmgpu_pf_params: that is the ABI and the server's wire format)
struct PfEnv {
    bool has_max_db_matches = false, has_sort_cap = false, has_stage_gb = false;
    uint64_t max_db_matches = 0;   // MMGPU_PF_MAX_DB_MATCHES (at least 64): a small database reaches the overflow path / a shard its share
    uint64_t sort_cap = 0;         // MMGPU_PF_SORT_CAP: a small database reaches the select kernel's candidate cap
    double stage_gb = 0;           // MMGPU_PF_STAGE_GB: budget of the candidate + survivor arrays of a stage chunk
    bool cofs_off = false;         // MMGPU_PF_COFS=0: the similar-k-mer kernels look lists up in the full offset table (A/B runs)
};
inline PfEnv pf_env() {
    PfEnv E;
    if (const char *e = getenv("MMGPU_PF_MAX_DB_MATCHES")) { E.has_max_db_matches = true; E.max_db_matches = std::max<uint64_t>(64, strtoull(e, nullptr, 10)); }
    if (const char *e = getenv("MMGPU_PF_SORT_CAP")) { E.has_sort_cap = true; E.sort_cap = strtoull(e, nullptr, 10); }
    if (const char *e = getenv("MMGPU_PF_STAGE_GB")) { E.has_stage_gb = true; E.stage_gb = atof(e); }
    if (const char *e = getenv("MMGPU_PF_COFS")) E.cofs_off = e[0] == '0';
    return E;
}

// The resident state of a context, or one under construction: the record owns what it holds and frees it when it dies.  A
// context's own copy of these fields (mmgpu_ctx::db, pf_masked_res, pf, h_len, mean_len, shard.on) changes hands only through
// resident_swap; the shard's id tables stay with the context (mmgpu_pf_set_shard rewrites them).
struct ResidentDb {
    DeviceDb db;
    uint8_t *masked = nullptr;     // the prefilter's view (mmgpu_ctx::pf_masked_res)
    PfIndex *pf = nullptr;
    std::vector<uint32_t> h_len;
    uint32_t mean_len = 0;
    bool shard_on = false;
    ResidentDb() = default;
    ResidentDb(const ResidentDb &) = delete;
    ResidentDb &operator=(const ResidentDb &) = delete;
    ~ResidentDb() { delete pf; dev_free(masked); dev_free(db.res); dev_free(db.off4); dev_free(db.len); }
};
// The context's state and the record's change places.  With an empty record this detaches the context's state and leaves the context
// empty and consistent (no targets, no masked view, no index, no lengths, shard flag off); with an empty context it attaches the
// record's; with both full the context takes the new state and the record the old one, to free it or to swap it back.
void resident_swap(mmgpu_ctx *c, ResidentDb &r);

// pf_index_api.hip.  `who` is the entry point's name, the head of every message.
// The index's header and tables (score matrices, cumulative counts, ungapped matrix; from_host: the caller's offsets and entries as
// well) over the targets `db`, in two halves: every check of the arguments, on the host alone; then the uploads.  Neither touches a
// context: the caller frees the index it replaces between the two (both may not fit), and makes the result resident.
struct PfIndexDraft {
    const mmgpu_pf_index *ix = nullptr;
    std::unique_ptr<PfIndex> P;            // header filled, no device buffer yet
    std::vector<uint16_t> cum3, cum2;      // cumulative counts of the score rows
    std::vector<uint32_t> off32;           // from_host: the caller's offsets and entries in the device's formats
    std::vector<uint64_t> ent;
};
int pf_index_check(const char *who, const DeviceDb &db, const mmgpu_pf_index *ix, bool from_host, PfIndexDraft &D);
int pf_index_upload(const char *who, PfIndexDraft &D, std::unique_ptr<PfIndex> &out);
// what is derived from the offsets on the device: the non-empty bit table and the compact offset table
hipError_t pf_index_bitmap(PfIndex *P, hipStream_t s);
hipError_t pf_index_cofs(PfIndex *P, hipStream_t s);

}  // namespace mmgpu
#endif
