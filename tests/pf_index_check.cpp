// pf_index_check (mmseqs2_amd/csrc/pf_index.h), the host half of mmgpu_pf_load_index / mmgpu_pf_build_index / mmgpu_db_load: every
// refusal comes before anything is sized from the tables' contents, touches no device, and is headed by the entry point's name.
#include "pf_index.h"
#include <cstdio>
using namespace mmgpu;

static int expect(const char *what, int rc, int want_rc, const char *want_msg) {
    if (rc == want_rc && (!want_msg || std::string(mmgpu_last_error()) == want_msg)) return 0;
    printf("FAIL %s: rc %d '%s', expected rc %d '%s'\n", what, rc, mmgpu_last_error(), want_rc, want_msg ? want_msg : "");
    return 1;
}

int main() {
    const int alphabet = 21, ka = 20;
    const size_t n3 = (size_t)ka * ka * ka, n2 = (size_t)ka * ka;
    std::vector<int16_t> sub(alphabet * alphabet, -1);
    for (int a = 0; a < alphabet; a++) sub[a * alphabet + a] = 4;
    std::vector<int16_t> s3(n3 * n3), s2(n2 * n2);
    std::vector<uint32_t> i3(n3 * n3), i2(n2 * n2);
    if (mmgpu_host_score_matrix(sub.data(), alphabet, 3, s3.data(), i3.data()) || mmgpu_host_score_matrix(sub.data(), alphabet, 2, s2.data(), i2.data())) return 2;
    std::vector<int16_t> rev3(s3), rev2(s2);      // every row ascending
    for (size_t r = 0; r < n3; r++) std::reverse(rev3.begin() + r * n3, rev3.begin() + (r + 1) * n3);
    for (size_t r = 0; r < n2; r++) std::reverse(rev2.begin() + r * n2, rev2.begin() + (r + 1) * n2);
    std::vector<int8_t> um(alphabet * alphabet, 1);
    DeviceDb db;
    db.res = (uint8_t *)16;      // "targets are loaded": never dereferenced by the check
    db.alphabet = alphabet;
    db.n = 10;
    mmgpu_pf_index ok;
    memset(&ok, 0, sizeof(ok));
    ok.kmer_size = 6; ok.alphabet = alphabet; ok.spaced = 1;
    ok.score3 = s3.data(); ok.index3 = i3.data(); ok.row3 = n3; ok.ungapped_mat = um.data();
    int bad = 0;
    {
        PfIndexDraft D;
        bad += expect("sorted rows", pf_index_check("mmgpu_pf_build_index", db, &ok, false, D), MMGPU_OK, nullptr);
        if (!D.P || D.P->table != 64000000ull || D.P->cum_w != 17 || D.P->score_min != -3 || D.cum3.size() != n3 * 17) { printf("FAIL header\n"); bad++; }
    }
    PfIndexDraft D;
    mmgpu_pf_index ix = ok;
    ix.score3 = rev3.data();
    bad += expect("score3 ascending", pf_index_check("mmgpu_pf_load_index", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_pf_load_index: score3 rows are not sorted by descending score");
    bad += expect("score3 ascending", pf_index_check("mmgpu_pf_build_index", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_pf_build_index: score3 rows are not sorted by descending score");
    ix = ok; ix.kmer_size = 7; ix.score2 = rev2.data(); ix.index2 = i2.data(); ix.row2 = n2;
    bad += expect("score2 ascending", pf_index_check("mmgpu_db_load", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_db_load: score2 rows are not sorted by descending score");
    ix.score2 = s2.data(); ix.row2 = n2 - 1;
    bad += expect("row2 short", pf_index_check("mmgpu_pf_build_index", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_pf_build_index: row2 smaller than kalph^2");
    ix = ok; ix.row3 = n3 - 1;
    bad += expect("row3 short", pf_index_check("mmgpu_pf_build_index", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_pf_build_index: row3 smaller than kalph^3");
    ix = ok; ix.ungapped_mat = nullptr;
    bad += expect("no ungapped matrix", pf_index_check("mmgpu_pf_build_index", db, &ix, false, D), MMGPU_ERR_ARG, "mmgpu_pf_build_index: NULL table");
    ix = ok; ix.kmer_size = 3; ix.score3 = nullptr;
    bad += expect("k = 3", pf_index_check("mmgpu_pf_build_index", db, &ix, false, D), MMGPU_ERR_UNSUPPORTED, "mmgpu_pf_build_index: k must be in [4, 15]");
    ix = ok; ix.kmer_size = 4; ix.score3 = nullptr;      // host index, exact matching: offsets and entries are checked too
    const uint64_t table = 160000;
    std::vector<uint64_t> off(table + 1, 0);
    std::vector<uint32_t> ids = {3, 10};      // the second names a target that is not loaded
    std::vector<uint16_t> pos = {0, 0};
    for (uint64_t z = 6; z <= table; z++) off[z] = 2;
    ix.offsets = off.data(); ix.entry_ids = ids.data(); ix.entry_pos = pos.data(); ix.n_entries = 2;
    bad += expect("entry out of range", pf_index_check("mmgpu_pf_load_index", db, &ix, true, D), MMGPU_ERR_ARG, "mmgpu_pf_load_index: index entry names a target that is not loaded");
    ids[1] = 9;
    bad += expect("host index", pf_index_check("mmgpu_pf_load_index", db, &ix, true, D), MMGPU_OK, nullptr);
    off[7] = 1;
    bad += expect("offsets descend", pf_index_check("mmgpu_pf_load_index", db, &ix, true, D), MMGPU_ERR_ARG, "mmgpu_pf_load_index: offsets not monotone / out of range");
    if (!bad) printf("OK\n");
    return bad ? 1 : 0;
}
