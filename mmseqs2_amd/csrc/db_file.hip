// Persisted device layout.  The reference prepares a database for its GPU path ahead of time
// (`makepaddedseqdb`, src/util/makepaddedseqdb.cpp: sequences padded and ordered for the device) and keeps precomputed prefilter
// indexes on disk (`createindex`; PrefilteringIndexReader.cpp reads them back).  Here it is ONE file with what a context has
// resident, in the layout it has on the device: targets (4-byte aligned residues, offsets, lengths), the prefilter's masked view
// when there is one, and the k-mer index (uint32 offsets, 8-byte entries).  mmgpu_db_load brings it back without the host
// touching a sequence: no SequenceLookup fill, no masking, no index build.  What is NOT in the file: the similar-k-mer score
// tables (they belong to the matrix, the caller hands them over as for mmgpu_pf_build_index) and anything derived on the device in
// milliseconds (compact offset table, non-empty bit table).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cstring>
#include <thread>

#include "pf_index.h"

using namespace mmgpu;

namespace {

struct DbFileHeader {
    char magic[8];                 // "MMGPUDB1"
    uint32_t version, header_bytes;
    uint64_t source_fp, index_fp;  // the caller's fingerprints: of the source database; of what the index depends on beyond it
    uint32_t n, alphabet, max_len, mean_len;
    uint64_t total_residues, res_bytes;
    uint32_t has_masked, has_index;
    int32_t k, spaced, kbase, pad0;
    uint64_t table, n_entries;
    uint64_t at[6], file_bytes;    // where every section starts: off4, len, res, masked, offsets, entries (DbSection)
    uint64_t sum[6];               // version 2: checksum of every section (db_kernels.hip), in the same order
};
constexpr uint32_t DB_VERSION = 2;
const char DB_MAGIC[8] = {'M', 'M', 'G', 'P', 'U', 'D', 'B', '1'};

uint64_t align4k(uint64_t x) { return (x + 4095ull) & ~4095ull; }

// The sections of a file, in the order of the header's at[] and sum[]: the section's size as the header's counts give it, and whether
// the file has it.  Saving, reading the header and loading all walk this table.
enum { SEC_OFF4, SEC_LEN, SEC_RES, SEC_MASKED, SEC_OFFSETS, SEC_ENTRIES, DB_SECTIONS };
struct DbSection {
    uint64_t bytes;
    bool present;
};
typedef std::array<DbSection, DB_SECTIONS> DbSections;
DbSections db_sections(const DbFileHeader &h) {
    const uint64_t nn = std::max<uint32_t>(h.n, 1);
    return {{{nn * 4, true}, {nn * 4, true}, {h.res_bytes, true}, {h.res_bytes, h.has_masked != 0}, {(h.table + 1) * 4, h.has_index != 0},
             {h.n_entries * 8, h.has_index != 0}}};
}

// device -> file, through a pinned staging buffer
int write_section(FILE *f, uint64_t at, const void *dev, size_t bytes) {
    if (fseeko(f, (off_t)at, SEEK_SET) != 0) return fail(MMGPU_ERR_ARG, "mmgpu_db_save: seek failed");
    const size_t chunk = 64ull << 20;
    PinnedStage stage;
    HIP_TRY(stage.reserve(std::min(chunk, std::max<size_t>(bytes, 1)), false));
    for (size_t o = 0; o < bytes; o += chunk) {
        const size_t m = std::min(chunk, bytes - o);
        if (hipMemcpy(stage.p, static_cast<const uint8_t *>(dev) + o, m, hipMemcpyDeviceToHost) != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_db_save: device read failed");
        if (fwrite(stage.p, 1, m, f) != m) return fail(MMGPU_ERR_ARG, "mmgpu_db_save: write failed (disk full?)");
    }
    return MMGPU_OK;
}

// file -> device: DB_READERS host threads, each with a pinned buffer of its own, take the chunks of a section in turn - pread (the
// kernel copies out of the page cache, no fault per page as through a mapping), then the copy engine moves the chunk while the
// thread reads its next one.  (One thread per chunk, not all threads on every chunk: starting 64 threads for each 32 MB chunk was
// most of the 0.24 s the 2.97 GB of a 1 M-target database took.)
constexpr int DB_READERS = 8;
constexpr size_t DB_CHUNK = 16ull << 20;
int upload_section(int device, void *dev, int fd, uint64_t at, size_t bytes, const UploadRing &ring) {
    const size_t n_chunks = (bytes + DB_CHUNK - 1) / DB_CHUNK;
    std::atomic<int> bad{0};
    auto reader = [&](int t) {
        if (hipSetDevice(device) != hipSuccess) { bad = 2; return; }
        for (size_t j = (size_t)t; j < n_chunks && !bad; j += DB_READERS) {
            const size_t o = j * DB_CHUNK, m = std::min(DB_CHUNK, bytes - o);
            if (ring.wait((size_t)t) != hipSuccess) { bad = 2; return; }
            uint8_t *stage = ring.slots[(size_t)t].p;
            for (size_t a = 0; a < m;) {
                const ssize_t got = pread(fd, stage + a, m - a, (off_t)(at + o + a));
                if (got <= 0) { bad = 1; return; }
                a += (size_t)got;
            }
            if (hipMemcpyAsync(static_cast<uint8_t *>(dev) + o, stage, m, hipMemcpyHostToDevice, ring.up.s) != hipSuccess ||
                ring.sent((size_t)t) != hipSuccess) { bad = 2; return; }
        }
    };
    const int nt = (int)std::min<size_t>(DB_READERS, n_chunks);
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(reader, t);
    if (nt > 0) reader(0);
    for (auto &x : th) x.join();
    if (bad == 1) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: short read (file truncated?)");
    if (bad) return fail(MMGPU_ERR_HIP, "mmgpu_db_load: upload failed");
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the header of the context's state, every section on a 4 KB boundary
DbSections save_fill_header(const mmgpu_ctx *c, uint64_t source_fp, uint64_t index_fp, bool with_index, DbFileHeader &h) {
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, DB_MAGIC, 8);
    h.version = DB_VERSION;
    h.header_bytes = (uint32_t)sizeof(h);
    h.source_fp = source_fp;
    h.index_fp = with_index ? index_fp : 0;
    h.n = c->db.n;
    h.alphabet = (uint32_t)c->db.alphabet;
    h.max_len = c->db.max_len;
    h.mean_len = c->mean_len;
    h.total_residues = c->db.total_residues;
    h.res_bytes = c->db.res_bytes;
    h.has_masked = c->pf_masked_res ? 1u : 0u;
    h.has_index = with_index ? 1u : 0u;
    if (with_index) {
        const PfIndex *P = c->pf;
        h.k = P->k; h.spaced = P->spaced; h.kbase = P->kbase;
        h.table = P->table; h.n_entries = P->n_entries;
    }
    const DbSections S = db_sections(h);
    uint64_t at = align4k(sizeof(h));
    for (int k = 0; k < DB_SECTIONS; k++) {
        if (!S[k].present) continue;
        h.at[k] = at;
        at = align4k(at + std::max<uint64_t>(S[k].bytes, 1));      // (an empty section takes a page too)
    }
    h.file_bytes = at;
    return S;
}

// header and sections into path.tmp, which takes the file's name when it is complete
int save_write_file(const char *path, const void *const *dev, const DbFileHeader &h, const DbSections &S) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(MMGPU_ERR_ARG, std::string("mmgpu_db_save: cannot create ") + tmp);
    int rc = MMGPU_OK;
    if (fwrite(&h, sizeof(h), 1, f) != 1) rc = fail(MMGPU_ERR_ARG, "mmgpu_db_save: write failed");
    for (int k = 0; k < DB_SECTIONS && rc == MMGPU_OK; k++)
        if (S[k].present && S[k].bytes) rc = write_section(f, h.at[k], dev[k], S[k].bytes);
    if (rc == MMGPU_OK && (ftruncate(fileno(f), (off_t)h.file_bytes) != 0)) rc = fail(MMGPU_ERR_ARG, "mmgpu_db_save: cannot size the file");
    if (fclose(f) != 0 && rc == MMGPU_OK) rc = fail(MMGPU_ERR_ARG, "mmgpu_db_save: close failed");
    if (rc == MMGPU_OK && rename(tmp.c_str(), path) != 0) rc = fail(MMGPU_ERR_ARG, std::string("mmgpu_db_save: cannot rename to ") + path);
    if (rc != MMGPU_OK) (void)remove(tmp.c_str());
    return rc;
}

}  // namespace

extern "C" int mmgpu_db_save(mmgpu_ctx *c, const char *path, uint64_t source_fingerprint, uint64_t index_fingerprint) {
    if (!c || !path) return fail(MMGPU_ERR_ARG, "mmgpu_db_save: NULL argument");
    if (!c->db.res) return fail(MMGPU_ERR_STATE, "mmgpu_db_save: no targets loaded");
    if (c->shard.on) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_db_save: the context holds a shard of a multi-GPU run (save the unsplit database)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const PfIndex *P = c->pf;
    const bool with_index = P != nullptr && index_fingerprint != 0 && P->d_offsets.p && P->kbase == P->kalph;
    DbFileHeader h;
    const DbSections S = save_fill_header(c, source_fingerprint, index_fingerprint, with_index, h);
    const void *dev[DB_SECTIONS] = {c->db.off4, c->db.len, c->db.res, c->pf_masked_res, with_index ? P->d_offsets.p : nullptr,
                                    with_index ? P->d_entries.p : nullptr};
    DevBuf d_sum;      // the sections' checksums, taken where they lie
    HIP_TRY(d_sum.alloc(8));
    for (int k = 0; k < DB_SECTIONS; k++)
        if (S[k].present) HIP_TRY(db_section_checksum(dev[k], S[k].bytes, d_sum.as<unsigned long long>(), &h.sum[k], c->stream));
    return save_write_file(path, dev, h, S);
}

static int db_read_header(const char *path, DbFileHeader *h, int *fd_out) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(MMGPU_ERR_STATE, std::string("mmgpu_db: cannot open ") + path);
    struct stat st;
    bool ok = read(fd, h, sizeof(*h)) == (ssize_t)sizeof(*h) && memcmp(h->magic, DB_MAGIC, 8) == 0 && h->version == DB_VERSION &&
              h->header_bytes == sizeof(*h) && fstat(fd, &st) == 0 && (uint64_t)st.st_size >= h->file_bytes;
    // sizes that cannot overflow the sums first, then every section inside the file
    ok = ok && h->table < (1ull << 40) && h->n_entries < (1ull << 40) && h->alphabet >= 1 && h->alphabet <= 255;
    if (ok) {
        const DbSections S = db_sections(*h);
        for (int k = 0; k < DB_SECTIONS; k++)
            ok = ok && (!S[k].present || (h->at[k] >= sizeof(*h) && S[k].bytes <= h->file_bytes && h->at[k] <= h->file_bytes - S[k].bytes));
    }
    if (!ok) {
        close(fd);
        return fail(MMGPU_ERR_STATE, std::string("mmgpu_db: not a database file of this library version: ") + path);
    }
    if (fd_out) *fd_out = fd; else close(fd);
    return MMGPU_OK;
}

extern "C" int mmgpu_db_probe(const char *path, mmgpu_db_info *info) {
    if (!path || !info) return fail(MMGPU_ERR_ARG, "mmgpu_db_probe: NULL argument");
    DbFileHeader h;
    const int rc = db_read_header(path, &h, nullptr);
    if (rc != MMGPU_OK) return rc;
    memset(info, 0, sizeof(*info));
    info->source_fingerprint = h.source_fp;
    info->index_fingerprint = h.index_fp;
    info->n_targets = h.n;
    info->alphabet = h.alphabet;
    info->total_residues = h.total_residues;
    info->has_masked_view = (int32_t)h.has_masked;
    info->has_index = (int32_t)h.has_index;
    info->kmer_size = h.k;
    info->spaced = h.spaced;
    info->n_entries = h.n_entries;
    info->file_bytes = h.file_bytes;
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// One call of mmgpu_db_load.  The file's content becomes a resident state of its own (`nb`), beside what the context holds; the
// context takes it, and lets go of its own, only when all of it has been uploaded and checked: a file that turns out damaged - in
// the targets or in the index - leaves the context as it was, and what was uploaded goes with this record.
namespace {
struct DbLoad {
    mmgpu_ctx *c;
    const mmgpu_pf_index *tables;
    bool want_index = false;
    int fd = -1;
    DbFileHeader h;
    DbSections S;
    ResidentDb nb;
    std::unique_ptr<PfIndex> P;      // the file's index until it is complete (then nb's)
    DevBuf d_chk;
    UploadRing ring;      // (last: its stream has drained before a failure frees what it copies into)
    ~DbLoad() { if (fd >= 0) close(fd); }

    int read_and_match(const char *path, uint64_t source_fp, uint64_t index_fp) {
        if (int e = db_read_header(path, &h, &fd)) return e;
        if (h.source_fp != source_fp) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: the file was made from another database (source fingerprint differs)");
        want_index = index_fp != 0;
        if (want_index && (!h.has_index || h.index_fp != index_fp)) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: the file holds no index built with these parameters (index fingerprint differs)");
        if (want_index && !tables) return fail(MMGPU_ERR_ARG, "mmgpu_db_load: the index needs the caller's score tables");
        if (want_index && (tables->kmer_size != h.k || tables->spaced != h.spaced || tables->alphabet != (int)h.alphabet)) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: k-mer size / pattern / alphabet differ from the file's index");
        S = db_sections(h);
        // (the masked view serves the prefilter only: a caller that asks for the targets alone gets them alone)
        if (!want_index) S[SEC_MASKED].present = S[SEC_OFFSETS].present = S[SEC_ENTRIES].present = false;
        return MMGPU_OK;
    }
    int upload_sec(int k, void *dev) { return upload_section(c->device, dev, fd, h.at[k], (size_t)S[k].bytes, ring); }
    bool section_ok(int k, const void *dev) {
        uint64_t sum = 0;
        return db_section_checksum(dev, (size_t)S[k].bytes, d_chk.as<unsigned long long>(), &sum, ring.up.s) == hipSuccess && sum == h.sum[k];
    }
    int upload_targets() {
        HIP_TRY(ring.open(DB_READERS));
        for (PinnedStage &x : ring.slots) HIP_TRY(x.reserve(DB_CHUNK));
        DeviceDb &db = nb.db;
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.res, (size_t)S[SEC_RES].bytes));
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.off4, (size_t)S[SEC_OFF4].bytes));
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.len, (size_t)S[SEC_LEN].bytes));
        if (int e = upload_sec(SEC_OFF4, db.off4)) return e;
        if (int e = upload_sec(SEC_LEN, db.len)) return e;
        if (int e = upload_sec(SEC_RES, db.res)) return e;
        if (S[SEC_MASKED].present) {
            HIP_TRY(dev_malloc_ctx(c, (void **)&nb.masked, (size_t)S[SEC_MASKED].bytes));
            if (int e = upload_sec(SEC_MASKED, nb.masked)) return e;
        }
        db.n = h.n;
        db.res_bytes = (size_t)h.res_bytes;
        db.max_len = h.max_len;
        db.total_residues = h.total_residues;
        db.alphabet = (int)h.alphabet;
        nb.mean_len = h.mean_len;
        nb.h_len.resize(h.n);
        if (h.n && pread(fd, nb.h_len.data(), (size_t)h.n * 4, (off_t)h.at[SEC_LEN]) != (ssize_t)((size_t)h.n * 4)) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: short read (file truncated?)");
        HIP_TRY(hipStreamSynchronize(ring.up.s));
        return MMGPU_OK;
    }
    // what arrived is what was saved, and it has the properties the kernels rely on
    int verify_targets() {
        HIP_TRY(d_chk.alloc(8));
        const DeviceDb &db = nb.db;
        if (!section_ok(SEC_OFF4, db.off4) || !section_ok(SEC_LEN, db.len) || !section_ok(SEC_RES, db.res) || (nb.masked && !section_ok(SEC_MASKED, nb.masked)))
            return fail(MMGPU_ERR_STATE, "mmgpu_db_load: a section's checksum differs from the one in the header (damaged file)");
        uint32_t bad = 0;
        HIP_TRY(db_validate_layout(db.off4, db.len, h.n, h.res_bytes, h.max_len, nullptr, 0, nullptr, 0, d_chk.as<uint32_t>(), &bad, ring.up.s));
        if (bad) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: a target of the file lies outside its residue block");
        return MMGPU_OK;
    }
    // the caller's tables, the file's offsets and entries, and the same checks for them
    int load_index() {
        const char *who = "mmgpu_db_load";
        PfIndexDraft D;
        if (int e = pf_index_check(who, nb.db, tables, false, D)) return e;
        if (D.P->table != h.table || D.P->kbase != h.kbase) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: k-mer table size differs from the file's index");
        if (int e = pf_index_upload(who, D, P)) return e;
        P->n_entries = h.n_entries;
        if (P->d_offsets.alloc((size_t)S[SEC_OFFSETS].bytes) != hipSuccess || P->d_entries.alloc(std::max<uint64_t>(P->n_entries, 1) * 8) != hipSuccess)
            return fail(MMGPU_ERR_HIP, "mmgpu_db_load: out of device memory for the index");
        if (int e = upload_sec(SEC_OFFSETS, P->d_offsets.p)) return e;
        if (P->n_entries)
            if (int e = upload_sec(SEC_ENTRIES, P->d_entries.p)) return e;
        if (hipStreamSynchronize(ring.up.s) != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_db_load: upload failed");
        if (!section_ok(SEC_OFFSETS, P->d_offsets.p) || !section_ok(SEC_ENTRIES, P->d_entries.p))
            return fail(MMGPU_ERR_STATE, "mmgpu_db_load: the index's checksum differs from the one in the header (damaged file)");
        uint32_t bad = 0;
        if (db_validate_layout(nb.db.off4, nb.db.len, h.n, h.res_bytes, h.max_len, P->d_offsets.as<uint32_t>(), P->table, P->d_entries.as<uint64_t>(), P->n_entries,
                               d_chk.as<uint32_t>(), &bad, ring.up.s) != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_db_load: layout check failed");
        if (bad) return fail(MMGPU_ERR_STATE, "mmgpu_db_load: the file's index is not a k-mer index over these targets (offsets not monotone / entry out of range)");
        if (pf_index_bitmap(P.get(), c->stream) != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_db_load: bit table failed");
        if (pf_index_cofs(P.get(), c->stream) != hipSuccess) return fail(MMGPU_ERR_HIP, "mmgpu_db_load: compact offset table failed");
        nb.pf = P.release();
        return MMGPU_OK;
    }
    // the context takes the new state; the old one goes once nothing on the context's stream reads it any more
    void commit() {
        (void)hipStreamSynchronize(c->stream);
        resident_swap(c, nb);      // (nb holds the old state now, and frees it with this record)
    }
};

}  // namespace

extern "C" int mmgpu_db_load(mmgpu_ctx *c, const char *path, uint64_t source_fingerprint, uint64_t index_fingerprint, const mmgpu_pf_index *tables) {
    if (!c || !path) return fail(MMGPU_ERR_ARG, "mmgpu_db_load: NULL argument");
    DbLoad L{c, tables};
    if (int e = L.read_and_match(path, source_fingerprint, index_fingerprint)) return e;
    HIP_TRY(hipSetDevice(c->device));
    if (int e = L.upload_targets()) return e;
    if (int e = L.verify_targets()) return e;
    if (L.want_index)
        if (int e = L.load_index()) return e;
    L.commit();
    return MMGPU_OK;
}
