// Host side of the resident target database: what a context holds and who owns it (ResidentDb, pf_index.h), the targets made
// resident from host arrays, and the prefilter's tantan-masked view of them (tantan_kernel.hip).  The k-mer index over the targets
// is pf_index_api.hip's, the persisted file db_file.hip's.  See include/mmgpu.h for the contract.
#include <atomic>
#include <cmath>
#include <cstring>

#include "pf_index.h"

using namespace mmgpu;

namespace mmgpu {
void resident_swap(mmgpu_ctx *c, ResidentDb &r) {
    std::swap(c->db, r.db);
    std::swap(c->pf_masked_res, r.masked);
    std::swap(c->pf, r.pf);
    c->h_len.swap(r.h_len);
    std::swap(c->mean_len, r.mean_len);
    std::swap(c->shard.on, r.shard_on);
}

// the resident targets, their masked view, the index over them and the shard flag of a context go
void db_release(mmgpu_ctx *c) {
    ResidentDb gone;
    resident_swap(c, gone);
}
}  // namespace mmgpu

// ---------------------------------------------------------------------------------------------------------
// Layout in HBM: 64 B of padding, every target at a 4-byte boundary (pad letters = the "no letter" code), max_len + 64 B of
// padding behind the last.  The device buffer is filled with the pad code, then the targets travel in chunks: the host threads
// pack chunk j + 1 into one of two pinned staging buffers while the copy engine moves chunk j (a pageable 280 MB buffer packed
// first and copied then cost 0.14 s for the 1 M targets of configs[2], 2 GB/s).
namespace {
struct LoadTargets {
    const uint8_t *residues;
    const uint64_t *offsets;
    uint32_t n;
    int alphabet;
    std::vector<uint32_t> off4, len;
    uint64_t end4 = 16;      // 64 bytes of padding in front: the reverse scan reads up to 3 bytes before a target (sw_kernel.hip)
    uint32_t max_len = 0;
    uint64_t total = 0;
    size_t bytes = 0;
    ResidentDb nb;
    UploadRing ring;         // (after nb: the stream has drained before a failure frees the buffers it copies into)

    // the arguments' checks and where every target goes (no device call)
    int layout() {
        off4.resize(std::max<uint32_t>(n, 1));
        len.resize(std::max<uint32_t>(n, 1));
        for (uint32_t i = 0; i < n; i++) {
            if (offsets[i + 1] < offsets[i]) return fail(MMGPU_ERR_ARG, "mmgpu_load_targets: offsets not monotone");
            const uint64_t l = offsets[i + 1] - offsets[i];
            if (l > 65535) return fail(MMGPU_ERR_ARG, "mmgpu_load_targets: sequence longer than 65535 (Parameters.h:271)");
            if (end4 > 0xFFFFFFFFull) return fail(MMGPU_ERR_UNSUPPORTED, "mmgpu_load_targets: more than 16 GiB of residues per shard");
            off4[i] = (uint32_t)end4;
            len[i] = (uint32_t)l;
            max_len = std::max<uint32_t>(max_len, (uint32_t)l);
            total += l;
            end4 += (l + 3) / 4;
        }
        bytes = (size_t)end4 * 4 + max_len + 64;
        return MMGPU_OK;
    }
    int allocate(mmgpu_ctx *c) {
        DeviceDb &db = nb.db;
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.res, bytes));
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.off4, off4.size() * sizeof(uint32_t)));
        HIP_TRY(dev_malloc_ctx(c, (void **)&db.len, len.size() * sizeof(uint32_t)));
        HIP_TRY(ring.open(2));
        hipStream_t up = ring.up.s;
        HIP_TRY(hipMemsetAsync(db.res, alphabet, bytes, up));
        HIP_TRY(hipMemcpyAsync(db.off4, off4.data(), off4.size() * sizeof(uint32_t), hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(db.len, len.data(), len.size() * sizeof(uint32_t), hipMemcpyHostToDevice, up));
        return MMGPU_OK;
    }
    int pack_and_upload() {
        hipStream_t up = ring.up.s;
        const size_t chunk_bytes = (size_t)std::min<uint64_t>(32ull << 20, std::max<uint64_t>((uint64_t)(end4 - 16) * 4, 4096));
        std::atomic<bool> bad_res(false);
        for (uint32_t first = 0, j = 0; first < n; j++) {
            // targets [first, last): at most chunk_bytes of packed residues (one target alone may exceed it by < 64 KB: staged is sized for that)
            const uint64_t base = (uint64_t)off4[first] * 4;
            uint32_t lo = first + 1, hi = n;        // largest last with packed end <= base + chunk_bytes
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                const uint64_t end_mid = mid < n ? (uint64_t)off4[mid] * 4 : (uint64_t)end4 * 4;
                if (end_mid - base <= chunk_bytes) lo = mid; else hi = mid - 1;
            }
            const uint32_t last = lo;
            const uint64_t end = last < n ? (uint64_t)off4[last] * 4 : (uint64_t)end4 * 4;
            const size_t k = j & 1;
            if (!ring.slots[k].p) HIP_TRY(ring.slots[k].reserve(chunk_bytes + 65536 + 64));
            else HIP_TRY(ring.wait(k));      // the copy out of this buffer two chunks ago
            uint8_t *dst = ring.slots[k].p;
            parallel_for((size_t)(last - first), [&, first, base, dst](size_t a, size_t b) {
                for (size_t i = first + a; i < first + b; i++) {
                    const uint8_t *src = residues + offsets[i];
                    uint8_t *out = dst + ((uint64_t)off4[i] * 4 - base);
                    const uint32_t l = len[i];
                    uint8_t top = 0;
                    for (uint32_t x = 0; x < l; x++) top = std::max(top, src[x]);
                    if (top >= alphabet) bad_res = true;
                    memcpy(out, src, l);
                    for (uint32_t x = l; x < ((l + 3) & ~3u); x++) out[x] = (uint8_t)alphabet;
                }
            });
            HIP_TRY(hipMemcpyAsync(nb.db.res + base, dst, end - base, hipMemcpyHostToDevice, up));
            HIP_TRY(ring.sent(k));
            first = last;
        }
        HIP_TRY(hipStreamSynchronize(up));
        if (bad_res) return fail(MMGPU_ERR_ARG, "mmgpu_load_targets: residue code >= alphabet");
        return MMGPU_OK;
    }
    void adopt(mmgpu_ctx *c) {
        nb.db.n = n;
        nb.db.res_bytes = bytes;
        nb.db.max_len = max_len;
        nb.db.total_residues = total;
        nb.db.alphabet = alphabet;
        nb.h_len.assign(len.begin(), len.begin() + n);
        nb.mean_len = n ? (uint32_t)(total / n) : 0;
        resident_swap(c, nb);
    }
};

}  // namespace

extern "C" int mmgpu_load_targets(mmgpu_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n,
                                  int alphabet) {
    if (!c || !residues || !offsets) return fail(MMGPU_ERR_ARG, "mmgpu_load_targets: NULL argument");
    if (alphabet < 2 || alphabet > 254) return fail(MMGPU_ERR_ARG, "mmgpu_load_targets: bad alphabet size");
    LoadTargets L{residues, offsets, n, alphabet};
    if (int e = L.layout()) return e;      // (up to here a refused call leaves the context as it was)
    HIP_TRY(hipSetDevice(c->device));
    // the old database goes before the new one is allocated (both may not fit), and with it what belongs to it: the masked view,
    // the prefilter index built / loaded for it, the shard flag
    db_release(c);
    if (int e = L.allocate(c)) return e;
    if (int e = L.pack_and_upload()) return e;
    L.adopt(c);
    return MMGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// tantan masking of the resident targets for the prefilter (tantan_kernel.hip): what IndexBuilder::fillDatabase does to every
// target before it counts k-mers (IndexBuilder.cpp:148, Masker.cpp:14-57 with maskTantan only).  The alignment kernels keep
// reading the unmasked residues.
namespace {
struct MaskTargets {
    mmgpu_ctx *c;
    hipStream_t s;
    uint32_t n, n_waves;
    TantanArgs A;
    std::vector<uint32_t> order;                  // targets by length, longest first: 64 consecutive ones share a wavefront and end together
    std::vector<uint64_t> pbase, sbase;           // [n_waves] where a wavefront's forward probabilities / scale factors start
    uint64_t pcur = 0, scur = 0;                  // ... and where the last one's end
    std::vector<double> lr, b2f;
    std::vector<uint32_t> chunk_first;            // wavefronts [chunk_first[k], chunk_first[k + 1])
    uint64_t chunk_p = 0, chunk_s = 0;            // the largest chunk's scratch (floats, doubles)
    DevBuf d_order, d_pbase, d_sbase, d_lr, d_b2f, d_probs, d_scales, d_count;

    void order_and_bases() {
        std::vector<uint32_t> first_le;
        order_targets_by_length(c->h_len, order, first_le);      // (lengths are at most 65535: mmgpu_load_targets / db_validate_layout)
        pbase.resize(std::max<uint32_t>(n_waves, 1));
        sbase.resize(std::max<uint32_t>(n_waves, 1));
        for (uint32_t w = 0; w < n_waves; w++) {
            const uint64_t longest = c->h_len[order[(size_t)w * 64]];      // the first of a wavefront is its longest
            pbase[w] = pcur;
            sbase[w] = scur;
            pcur += longest * 64;
            scur += (longest / 16 + 1) * 64;
        }
    }
    // Tantan's constructor (tantan.cpp:94-131) with the Masker's constants (Masker.cpp:22-31)
    void tantan_constants() {
        const double decay = 0.9;
        const int max_offset = 50;
        A.repeat_prob = 0.005;
        A.repeat_end_prob = 0.05;
        b2f.resize(max_offset);
        const double first_prob = (decay < 1 || decay > 1) ? (1 - decay) / (1 - std::pow(decay, max_offset)) : 1.0 / max_offset;   // :38-44
        double p = A.repeat_prob * first_prob;
        for (int i = 0; i < max_offset; i++) {
            b2f[i] = p;
            p *= decay;
        }
    }
    // The forward probabilities (4 B per residue) and scale factors (0.5 B) are scratch: wavefronts run in chunks whose scratch stays
    // below MMGPU_TANTAN_SCRATCH_MB (default 8 GB; a quarter of the free memory if that is less) - one chunk for 1 M targets, several
    // for a shard near the 16 G-residue limit, which would otherwise ask for 70 GB on top of the masked copy.
    void cut_chunks() {
        uint64_t budget = (getenv("MMGPU_TANTAN_SCRATCH_MB") ? strtoull(getenv("MMGPU_TANTAN_SCRATCH_MB"), nullptr, 10) : 8192ull) << 20;
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) budget = std::min<uint64_t>(budget, std::max<uint64_t>(mem_free / 4, 64ull << 20));
        auto p_end = [&](uint32_t w) { return w < n_waves ? pbase[w] : pcur; };
        auto s_end = [&](uint32_t w) { return w < n_waves ? sbase[w] : scur; };
        chunk_first.assign(1, 0);
        for (uint32_t w0 = 0; w0 < n_waves;) {
            uint32_t w1 = w0 + 1;      // (a single wavefront over the budget runs alone)
            while (w1 < n_waves && (p_end(w1 + 1) - pbase[w0]) * 4 + (s_end(w1 + 1) - sbase[w0]) * 8 <= budget) w1++;
            chunk_p = std::max(chunk_p, p_end(w1) - pbase[w0]);
            chunk_s = std::max(chunk_s, s_end(w1) - sbase[w0]);
            chunk_first.push_back(w1);
            w0 = w1;
        }
    }
    int upload_inputs(const double *likelihood_ratios, int alphabet, double min_mask_prob, int mask_letter) {
        for (DevBuf *d : {&d_order, &d_pbase, &d_sbase, &d_lr, &d_b2f, &d_probs, &d_scales, &d_count}) d->bind(c->cache);
        HIP_TRY(upload(d_order, order, s));
        HIP_TRY(upload(d_pbase, pbase, s));
        HIP_TRY(upload(d_sbase, sbase, s));
        lr.assign(likelihood_ratios, likelihood_ratios + (size_t)alphabet * alphabet);
        HIP_TRY(upload(d_lr, lr, s));
        HIP_TRY(upload(d_b2f, b2f, s));
        A.t_res = c->db.res;
        A.out_res = c->pf_masked_res;
        A.t_off4 = c->db.off4;
        A.t_len = c->db.len;
        A.lr = d_lr.as<double>();
        A.b2f = d_b2f.as<double>();
        A.alphabet = alphabet;
        A.min_mask_prob = min_mask_prob;
        A.mask_letter = (uint8_t)mask_letter;
        return MMGPU_OK;
    }
    // the chunks one after the other over one scratch allocation, and the number of residues they masked
    int run_chunks(uint64_t *n_masked) {
        HIP_TRY(d_probs.alloc(std::max<uint64_t>(chunk_p, 1) * sizeof(float)));
        HIP_TRY(d_scales.alloc(std::max<uint64_t>(chunk_s, 1) * sizeof(double)));
        HIP_TRY(d_count.alloc(8));
        HIP_TRY(hipMemsetAsync(d_count.p, 0, 8, s));
        A.n_masked = d_count.as<unsigned long long>();
        for (size_t k = 0; k + 1 < chunk_first.size(); k++) {      // (same stream: a chunk's scratch is free again when the next one starts)
            const uint32_t w0 = chunk_first[k], w1 = chunk_first[k + 1];
            A.order = d_order.as<uint32_t>() + (size_t)w0 * 64;
            A.n = std::min<uint32_t>(n - w0 * 64, (w1 - w0) * 64);
            // the bases stay absolute: the scratch pointers are moved back by the chunk's first base instead
            A.probs = d_probs.as<float>() - pbase[w0];
            A.scales = d_scales.as<double>() - sbase[w0];
            A.wave_prob_base = d_pbase.as<uint64_t>() + w0;
            A.wave_scale_base = d_sbase.as<uint64_t>() + w0;
            HIP_TRY(launch_tantan_mask(A, s));
        }
        unsigned long long masked = 0;
        HIP_TRY(hipMemcpyAsync(&masked, d_count.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));      // (the host vectors the uploads read die after this)
        if (n_masked) *n_masked = masked;
        return MMGPU_OK;
    }
};

}  // namespace

extern "C" int mmgpu_pf_mask_targets(mmgpu_ctx *c, const double *likelihood_ratios, int alphabet, double min_mask_prob, int mask_letter,
                                     uint64_t *n_masked) {
    if (!c) return fail(MMGPU_ERR_ARG, "mmgpu_pf_mask_targets: NULL argument");
    if (!c->db.res) return fail(MMGPU_ERR_STATE, "mmgpu_pf_mask_targets: no targets loaded");
    if (!likelihood_ratios) {      // back to the unmasked view (--mask 0 after --mask 1 on a resident database): the masked copy and its index go
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        pf_index_free(c);
        dev_free(c->pf_masked_res);
        c->pf_masked_res = nullptr;
        if (n_masked) *n_masked = 0;
        return MMGPU_OK;
    }
    if (alphabet != c->db.alphabet || alphabet > 32) return fail(MMGPU_ERR_ARG, "mmgpu_pf_mask_targets: alphabet differs from the loaded targets (or exceeds 32)");
    if (mask_letter < 0 || mask_letter >= alphabet) return fail(MMGPU_ERR_ARG, "mmgpu_pf_mask_targets: mask letter outside the alphabet");
    HIP_TRY(hipSetDevice(c->device));
    pf_index_free(c);      // an index built from the unmasked residues does not describe the masked ones
    if (!c->pf_masked_res) HIP_TRY(dev_malloc_ctx(c, (void **)&c->pf_masked_res, c->db.res_bytes));
    HIP_TRY(hipMemcpyAsync(c->pf_masked_res, c->db.res, c->db.res_bytes, hipMemcpyDeviceToDevice, c->stream));
    MaskTargets M{c, c->stream, c->db.n, (c->db.n + 63) / 64};
    M.order_and_bases();
    M.tantan_constants();
    if (int e = M.upload_inputs(likelihood_ratios, alphabet, min_mask_prob, mask_letter)) return e;
    M.cut_chunks();
    return M.run_chunks(n_masked);
}

// test hook: the prefilter's (masked) view of the resident targets back on the host, in the caller's layout
extern "C" int mmgpu_pf_debug_masked_targets(mmgpu_ctx *c, const uint64_t *offsets, uint32_t n, uint8_t *residues) {
    if (!c || !offsets || !residues) return fail(MMGPU_ERR_ARG, "mmgpu_pf_debug_masked_targets: NULL argument");
    if (!c->db.res || n != c->db.n) return fail(MMGPU_ERR_STATE, "mmgpu_pf_debug_masked_targets: not the resident target set");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint8_t> packed(c->db.res_bytes);
    HIP_TRY(hipMemcpy(packed.data(), c->pf_res(), packed.size(), hipMemcpyDeviceToHost));
    std::vector<uint32_t> off4(std::max<uint32_t>(n, 1));
    HIP_TRY(hipMemcpy(off4.data(), c->db.off4, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) memcpy(residues + offsets[i], packed.data() + (size_t)off4[i] * 4, (size_t)(offsets[i + 1] - offsets[i]));
    return MMGPU_OK;
}
