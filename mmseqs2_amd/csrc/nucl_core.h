// Nucleotide alignment step, what its two device forms share and the 16-lane LDS form (nucl_kernel.hip; the one-wavefront form
// is nucl_wave.h, included after this file by nucl_wave_kernel.hip):
//   * the views of a pair's sequences, the ungapped seed (pick_seed);
//   * the pieces of ksw_extz2_sse that do not depend on where the DP state lives, as functions (ksw_begin ... ksw_zdrop_step)
//     and the band of the backtrack (band_of);
//   * ksw_extz2 / ksw_walk with the state in LDS, 16 lanes per alignment (LdsForm);
//   * align_pairs<F>: the one loop over the pairs of a call, for F = LdsForm and F = nuclw::WaveForm.
// The host lane emulator of the tests (tests/nucl_emu.cpp) compiles this very code with NG cooperative contexts standing in
// for the lanes and checks it against the reference's vectors without a GPU.  The includer supplies:
//   NUCL_NG, NUCL_NS             lanes per alignment (16: LdsForm, 64: nuclw::WaveForm) and the namespace of that instantiation
//   NUCL_HD                      function qualifiers
//   NUCL_LANE()                  lane of the group, 0..NG-1
//   NUCL_SHFL(v, src) / NUCL_SHFL_XOR(v, mask) / NUCL_SHFL_U64(v, src)   exchange inside the group (src is taken modulo NG)
//   NUCL_SYNC()                  phase boundary: LDS written by one lane is read by another.  On the GPU the lanes of a
//                                group run in lock step, so this only pins the order of the LDS operations; the
//                                emulator switches contexts here.
//   NUCL_SYNC_MEM()              the same for the scratch in global memory (direction bytes, backtrack letters)
//   NUCL_ATOMIC_ADD_U32 / _U64   work queue and output cursor
#ifndef MMGPU_NUCL_CORE_H
#define MMGPU_NUCL_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/mmgpu.h"

namespace mmgpu {

// everything the kernel needs, device pointers only
struct NuclLaunch {
    const mmgpu_nucl_pair *pairs;
    const uint32_t *order;         // processing order (longest first): pair index
    uint32_t n_pairs;
    const uint8_t *q_res;          // queries, numeric, concatenated
    const uint32_t *q_off;         // [nq + 1]
    const uint8_t *t_res;
    const uint32_t *t_off4;
    const uint32_t *t_len;
    int8_t mat[25];
    uint8_t rev_lookup[8];
    int gapo, gape, zdrop;
    int past_end_q, past_end_t;
    int wrapped;                   // --wrapped-scoring: every query is its sequence written twice
    uint8_t *pscratch;             // direction bytes, one slice per 16-lane group of the grid
    uint64_t pscratch_stride;
    char *wscratch;                // backtrack letters, one slice per group
    uint64_t wscratch_stride;
    mmgpu_nucl_hit *out;
    char *bt;
    unsigned long long *bt_cursor;
    unsigned long long bt_cap;
    uint32_t *next_pair;           // work queue head
};

#ifdef NUCL_HD

#ifndef NUCL_NG
#define NUCL_NG 16
#endif
#ifndef NUCL_NS
#define NUCL_NS nucl
#endif

namespace NUCL_NS {

constexpr int NG = NUCL_NG;         // lanes per alignment
constexpr int WIN = 256;          // window of target positions kept in LDS (power of two, >= 16 blocks)
constexpr int KSW_NEG_INF = -0x40000000;
constexpr int KSW_W = 64;          // band of the reference's calls (BandedNucleotideAligner.cpp:176,193,203)

struct GroupLds {                  // per alignment
    uint8_t u[WIN], v[WIN], x[WIN], y[WIN], s[WIN];
    int32_t H[WIN];
};

// A sequence as one ksw call sees it.  idx = reversed ? L - (off + k) : off + k walks the aligned strand, whose
// element L (one past the end) is `past` - the reference's reversed copies are shifted by one because seq_reverse is
// called with L instead of L - 1 (BandedNucleotideAligner.cpp:61,68,93).
struct SeqView {
    const uint8_t *base;
    const uint8_t *rl;     // reverse-complement table, or null: the strand is base[] itself
    int L, off, past;
    bool reversed;
    NUCL_HD uint8_t strand(int idx) const {
        if (idx >= L) return (uint8_t)past;
        return rl ? rl[base[L - 1 - idx]] : base[idx];
    }
    NUCL_HD uint8_t get(int k) const { return strand(reversed ? L - (off + k) : off + k); }
};

struct Ez {
    int max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score;
};

NUCL_HD int8_t s8(int v) { return (int8_t)(uint8_t)v; }

NUCL_HD int group_lane() { return NUCL_LANE(); }

// (H, order) maximum over the 16 lanes of the group: larger H wins, equal H the smaller order
NUCL_HD void group_best(int &h, unsigned &o) {
#pragma unroll
    for (int d = 1; d < NG; d <<= 1) {
        const int h2 = NUCL_SHFL_XOR(h, d);
        const unsigned o2 = NUCL_SHFL_XOR(o, d);
        if (h2 > h || (h2 == h && o2 < o)) { h = h2; o = o2; }
    }
}

// ---- ksw_extz2_sse (lib/ksw2/ksw2_extz2_sse.cpp:44-285) without KSW_EZ_APPROX_MAX / _RIGHT / _GENERIC_SC (the flags the
// reference's caller never sets): the pieces that do not depend on where u, v, x, y, s and H live.  ksw_extz2 below and both walks
// are written with them; nuclw::ksw_extz2_wave states them once more in its own loop, for its speed (see there).

// What a call leaves where it computes nothing.  false: it computes nothing - a sequence is empty, or a mismatch costs more than
// two gaps, which the 8-bit differences cannot hold.
NUCL_HD bool ksw_begin(Ez &ez, int qlen, int tlen, const int8_t *mat, int qe) {
    ez.max_q = ez.max_t = ez.mqe_t = ez.mte_q = -1;
    ez.max = 0;
    ez.score = ez.mqe = ez.mte = KSW_NEG_INF;
    ez.zdropped = 0;
    if (qlen <= 0 || tlen <= 0) return false;
    int min_sc = mat[1];
    for (int t = 1; t < 25; ++t) min_sc = min_sc < mat[t] ? min_sc : mat[t];
    return !(-min_sc > 2 * qe);
}

// direction bytes per anti-diagonal of a call: the band's at most KSW_W + 1 cells, whole blocks, one more
NUCL_HD int ksw_n_col(int qlen, int tlen) {
    const int n = qlen < tlen ? qlen : tlen;
    return (((n < KSW_W + 1 ? n : KSW_W + 1) + 15) / 16 + 1) * 16;
}

// first / last target position of anti-diagonal r inside the band; st > en: the band has left the matrix
NUCL_HD void ksw_band(int r, int qlen, int tlen, int &st, int &en) {
    st = 0;
    en = tlen - 1;
    if (st < r - qlen + 1) st = r - qlen + 1;
    if (en > r) en = r;
    if (st < (r - KSW_W + 1) >> 1) st = (r - KSW_W + 1) >> 1;
    if (en > (r + KSW_W) >> 1) en = (r + KSW_W) >> 1;
}

// ... block-aligned: what the reference stores in off[] / off_end[]
NUCL_HD void band_of(int r, int qlen, int tlen, int &st, int &en) {
    ksw_band(r, qlen, tlen, st, en);
    st = st / 16 * 16;
    en = (en + 16) / 16 * 16 - 1;
}

// the reference scores whole groups of 16 from st0 (:135-145): the last position the score pass of band [st0, en0] writes
NUCL_HD int ksw_last_scored(int st0, int en0) { return st0 + ((en0 - st0) / 16 + 1) * 16 - 1; }

// one past the last block that has to hold defined contents on that anti-diagonal, en: the band's block-aligned end
NUCL_HD int ksw_blocks_needed(int last_scored, int en, int tlen_) {
    int need = (last_scored + 1 + 15) / 16;
    need = need < en / 16 + 1 ? en / 16 + 1 : need;
    return need > tlen_ ? tlen_ : need;
}

// score byte of a cell (:135-145); letter 4 (N) is a wildcard
NUCL_HD uint8_t ksw_score(uint8_t a, uint8_t b, int8_t sc_mch, int8_t sc_mis) {
    int8_t sc = a == b ? sc_mch : sc_mis;
    if (a == (uint8_t)4 || b == (uint8_t)4) sc = 0;
    return (uint8_t)sc;
}

// x[t-1], v[t-1] as the cell d = t - st of the aligned band sees them: cell 0 takes what enters from the left (x1, v1), and
// _mm_cvtsi32_si128 of a negative carry-in also sets bytes 1..3 of the first block's shifted vectors (:151-152).  The signs
// are the caller's, taken once per anti-diagonal: compared in here, the wave form's loop comes out five instructions longer.
NUCL_HD void ksw_carry_in(int d, int8_t x1, int8_t v1, bool x1_neg, bool v1_neg, int8_t &xt1, int8_t &vt1) {
    if (d == 0) { xt1 = x1; vt1 = v1; }
    if (d >= 1 && d <= 3) {
        if (x1_neg) xt1 = (int8_t)0xFF;
        if (v1_neg) vt1 = (int8_t)0xFF;
    }
}

// One cell (:153-200): u, y of the position go in and come out, v and x come out; returns the direction byte (WITH_P).
template <bool WITH_P>
NUCL_HD uint8_t ksw_cell(int8_t sc, int8_t xt1, int8_t vt1, uint8_t &u, uint8_t &v, uint8_t &x, uint8_t &y, int q, int qe,
                            uint8_t max_sc_u) {
    int8_t z = s8(sc + s8(qe * 2));
    int8_t a = s8(xt1 + vt1);
    const int8_t ut = (int8_t)u;
    int8_t b = s8((int8_t)y + ut);
    uint8_t d = 0;
    if (WITH_P) d = a > z ? 1 : 0;
    z = z > a ? z : a;
    if (WITH_P && b > z) d = 2;
    uint8_t zu = (uint8_t)z > (uint8_t)b ? (uint8_t)z : (uint8_t)b;
    zu = zu < max_sc_u ? zu : max_sc_u;
    z = (int8_t)zu;
    u = (uint8_t)s8(z - vt1);
    v = (uint8_t)s8(z - ut);
    z = s8(z - q);
    a = s8(a - z);
    b = s8(b - z);
    x = (uint8_t)(a > 0 ? a : 0);
    y = (uint8_t)(b > 0 ? b : 0);
    if (WITH_P) {
        if (a > 0) d |= 0x08;
        if (b > 0) d |= 0x10;
    }
    return d;
}

// Exact maximum of the band (:207-250): ties follow the reference's scan - position en0 first (order 0), then the four
// interleaved lanes of its 4-wide loop over [st0, en1) (lane by lane, ascending), then the scalar remainder [en1, en0).
NUCL_HD int ksw_tie_en1(int st0, int en0) { return st0 + (en0 - st0) / 4 * 4; }
NUCL_HD unsigned ksw_tie_order(int t, int st0, int en1) {
    return t < en1 ? 1u + (unsigned)((t - st0) & 3) * 0x100000u + (unsigned)((t - st0) >> 2) : 1u + 4u * 0x100000u + (unsigned)(t - en1);
}
NUCL_HD int ksw_tie_position(unsigned o, int st0, int en0, int en1) {
    if (o == 0) return en0;
    if (o <= 4u * 0x100000u) return st0 + (int)((o - 1u) & 0xFFFFFu) * 4 + (int)((o - 1u) >> 20);
    return en1 + (int)(o - 1u - 4u * 0x100000u);
}

// ksw_apply_zdrop (ksw2.h:182-199) with the maximum of anti-diagonal r; true: the extension ends here, and the caller sets
// ez.zdropped (set in here, the compiler merges that store with the one of ez.max_q through a chosen pointer before it inlines
// this, and Ez then lives in scratch memory)
NUCL_HD bool ksw_zdrop_step(Ez &ez, int max_H, int max_t, int r, int zdrop, int e) {
    if (max_H > ez.max) {
        ez.max = max_H;
        ez.max_t = max_t;
        ez.max_q = r - max_t;
    } else if (max_t >= ez.max_t && r - max_t >= ez.max_q) {
        const int tl = max_t - ez.max_t, ql = (r - max_t) - ez.max_q;
        const int l = tl > ql ? tl - ql : ql - tl;
        return zdrop >= 0 && ez.max - max_H > zdrop + l * e;
    }
    return false;
}

// ---- the 16-lane form: lane = byte of the reference's 128-bit vector, one block per step, the state in LDS (nucl_kernel.hip)

// WITH_P: record the direction bytes (calls without KSW_EZ_SCORE_ONLY).  All lanes of the group run this in step.
template <bool WITH_P, int N = NG>
NUCL_HD void ksw_extz2(const SeqView &qv, int qlen, const SeqView &tv, int tlen, const int8_t *mat, int q, int e, int zdrop,
                          GroupLds &S, uint8_t *p, Ez &ez) {
    static_assert(N == 16, "the LDS form is one block of the reference's vectors wide");
    const int lane = group_lane();
    const int qe = q + e;
    if (!ksw_begin(ez, qlen, tlen, mat, qe)) return;
    const int8_t sc_mch = mat[0], sc_mis = mat[1];
    const uint8_t max_sc_u = (uint8_t)s8(mat[0] + qe * 2);
    const int tlen_ = (tlen + 15) / 16;
    const int n_col = ksw_n_col(qlen, tlen);

    int init_blocks = 0;           // blocks [0, init_blocks) of the window hold defined contents
    int last_st = -1, last_en = -1;
    for (int r = 0; r < qlen + tlen - 1; ++r) {
        int st, en;
        ksw_band(r, qlen, tlen, st, en);
        if (st > en) {
            ez.zdropped = 1;
            break;
        }
        const int st0 = st, en0 = en;
        st = st / 16 * 16;
        en = (en + 16) / 16 * 16 - 1;
        // blocks the window reaches for the first time: zeros / "never computed" (the reference's calloc and H fill)
        {
            const int need = ksw_blocks_needed(ksw_last_scored(st0, en0), en, tlen_);
            for (int b = init_blocks; b < need; ++b) {
                const int k = (b * 16 + lane) & (WIN - 1);
                S.u[k] = 0; S.v[k] = 0; S.x[k] = 0; S.y[k] = 0; S.s[k] = 0;
                S.H[k] = KSW_NEG_INF;
            }
            init_blocks = init_blocks > need ? init_blocks : need;
        }
        NUCL_SYNC();
        // what enters the lowest block from the left (:126-132)
        int8_t x1, v1;
        if (st > 0) {
            if (st - 1 >= last_st && st - 1 <= last_en) { x1 = (int8_t)S.x[(st - 1) & (WIN - 1)]; v1 = (int8_t)S.v[(st - 1) & (WIN - 1)]; }
            else x1 = v1 = 0;
        } else {
            x1 = 0;
            v1 = r ? (int8_t)q : (int8_t)0;
        }
        NUCL_SYNC();   // every lane has read the carry-in
        if (en >= r && lane == 0) {
            S.y[r & (WIN - 1)] = 0;
            S.u[r & (WIN - 1)] = r ? (uint8_t)q : (uint8_t)0;
        }
        // scores of this anti-diagonal, whole 16-byte groups starting at st0 (:135-145); letter m - 1 is a wildcard.
        // Positions past the target read the allocation's zeros, query positions before its start likewise.
        for (int t0 = st0; t0 <= en0; t0 += 16) {
            const int t = t0 + lane;
            if (t < tlen_ * 16) {
                const uint8_t a = t < tlen ? tv.get(t) : (uint8_t)0;
                const uint8_t b = (r - t >= 0 && r - t < qlen) ? qv.get(r - t) : (uint8_t)0;
                S.s[t & (WIN - 1)] = ksw_score(a, b, sc_mch, sc_mis);
            }
        }
        NUCL_SYNC();
        // core: blocks from the highest to the lowest - cell t reads x[t-1], v[t-1], which a lower block still holds
        const bool x1_neg = x1 < 0, v1_neg = v1 < 0;
        for (int blk = en / 16; blk >= st / 16; --blk) {
            const int t = blk * 16 + lane, k = t & (WIN - 1);
            int8_t xt1 = 0, vt1 = 0;
            if (t != st) { xt1 = (int8_t)S.x[(t - 1) & (WIN - 1)]; vt1 = (int8_t)S.v[(t - 1) & (WIN - 1)]; }
            ksw_carry_in(t - st, x1, v1, x1_neg, v1_neg, xt1, vt1);
            const int8_t sc = (int8_t)S.s[k];
            uint8_t ut = S.u[k], yt = S.y[k], vt, xt;
            NUCL_SYNC();   // all reads of the block before its writes (lane + 1 reads this lane's x, v)
            const uint8_t d = ksw_cell<WITH_P>(sc, xt1, vt1, ut, vt, xt, yt, q, qe, max_sc_u);
            S.u[k] = ut;
            S.v[k] = vt;
            S.x[k] = xt;
            S.y[k] = yt;
            if (WITH_P) p[(size_t)r * (size_t)n_col + (size_t)(t - st)] = d;
        }
        // exact maximum of the band (ksw_tie_order)
        int max_H, max_t;
        NUCL_SYNC();
        if (r > 0) {
            const int k0 = en0 & (WIN - 1);
            const int h_en0 = en0 > 0 ? S.H[(en0 - 1) & (WIN - 1)] + (int)S.u[k0] - qe : S.H[k0] + (int)S.v[k0] - qe;
            const int en1 = ksw_tie_en1(st0, en0);
            NUCL_SYNC();   // H[en0 - 1] is read above and updated below by another lane
            int best_h = h_en0;
            unsigned best_o = 0;
            for (int t = st0 + lane; t < en0; t += NG) {
                const int k = t & (WIN - 1);
                const int h = S.H[k] + (int)S.v[k] - qe;
                S.H[k] = h;
                const unsigned o = ksw_tie_order(t, st0, en1);
                if (h > best_h || (h == best_h && o < best_o)) { best_h = h; best_o = o; }
            }
            if (lane == 0) S.H[k0] = h_en0;
            group_best(best_h, best_o);
            max_H = best_h;
            max_t = ksw_tie_position(best_o, st0, en0, en1);
        } else {
            const int h0 = (int)S.v[0] - qe - qe;
            if (lane == 0) S.H[0] = h0;
            max_H = h0;
            max_t = 0;
        }
        NUCL_SYNC();
        {
            const int h_en0 = S.H[en0 & (WIN - 1)], h_st0 = S.H[st0 & (WIN - 1)];
            if (en0 == tlen - 1 && h_en0 > ez.mte) { ez.mte = h_en0; ez.mte_q = r - en; }
            if (r - st0 == qlen - 1 && h_st0 > ez.mqe) { ez.mqe = h_st0; ez.mqe_t = st0; }
        }
        if (ksw_zdrop_step(ez, max_H, max_t, r, zdrop, e)) {
            ez.zdropped = 1;
            break;
        }
        if (r == qlen + tlen - 2 && en0 == tlen - 1) ez.score = S.H[(tlen - 1) & (WIN - 1)];
        last_st = st;
        last_en = en;
        NUCL_SYNC();
    }
    NUCL_SYNC();
}

// The state of one step of ksw_backtrack (ksw2.h:134-173, is_rot, no introns) at cell (i = target, j = query) of anti-diagonal
// r = i + j, whose direction bytes are row[0 ..]: 0 = 'M' to (i - 1, j - 1), 1 or 3 = 'D' to (i - 1, j), else 'I' to (i, j - 1).
// The two walks spell the move out themselves: moved in here through references, the compiler merges the decrements of i and j
// into one store through a selected pointer before it inlines this and both then live in scratch memory; moved by the letter
// (i -= c != 'I') the step of the wave form's walk, one lane's dependent chain, is 18 instructions longer.
NUCL_HD int ksw_walk_state(const uint8_t *row, int qlen, int tlen, int i, int j, int state) {
    int st, en;
    band_of(i + j, qlen, tlen, st, en);
    int force_state = -1;
    if (i < st) force_state = 2;
    if (i > en) force_state = 1;
    const unsigned tmp = force_state < 0 ? row[i - st] : 0u;
    if (state == 0) state = tmp & 7;
    else if (!(tmp >> (state + 2) & 1)) state = 0;
    if (state == 0) state = tmp & 7;
    if (force_state >= 0) state = force_state;
    return state;
}

// The walk from cell (i0, j0): one letter per step, last column first, into w[]; returns the number of letters.  One lane.
NUCL_HD int ksw_walk(const uint8_t *p, int qlen, int tlen, int i0, int j0, char *w) {
    const size_t n_col = (size_t)ksw_n_col(qlen, tlen);
    int i = i0, j = j0, state = 0, n = 0;
    while (i >= 0 && j >= 0) {
        state = ksw_walk_state(p + (size_t)(i + j) * n_col, qlen, tlen, i, j, state);
        if (state == 0) { w[n++] = 'M'; --i; --j; }
        else if (state == 1 || state == 3) { w[n++] = 'D'; --i; }
        else { w[n++] = 'I'; --j; }
    }
    for (; i >= 0; --i) w[n++] = 'D';
    for (; j >= 0; --j) w[n++] = 'I';
    return n;
}

struct LdsForm {
    typedef GroupLds Lds;
    template <bool WITH_P>
    static NUCL_HD void extz2(const SeqView &qv, int qlen, const SeqView &tv, int tlen, const int8_t *mat, int q, int e, int zdrop,
                                 Lds &S, uint8_t *p, Ez &ez) {
        ksw_extz2<WITH_P>(qv, qlen, tv, tlen, mat, q, e, zdrop, S, p, ez);
    }
    static NUCL_HD int lane0(int v) { return NUCL_SHFL(v, 0); }
    static NUCL_HD int walk(const uint8_t *p, int qlen, int tlen, int i0, int j0, char *w, Lds &) {   // lane 0 walks in HBM
        int n = 0;
        if (group_lane() == 0) n = ksw_walk(p, qlen, tlen, i0, j0, w);
        return lane0(n);
    }
};

// DistanceCalculator::computeSubstitutionStartEndDistance along one diagonal (:178-200), the group working through
// 16 positions at a time: every lane fetches one score, the recurrence then runs over the 16 by shuffles (uniform).
NUCL_HD void seed_segment(const SeqView &qv, int qo, const SeqView &tv, int to, unsigned len, const int8_t *mat, int &start,
                             int &end, int &best) {
    const int lane = group_lane();
    int max_score = 0, max_end = 0, max_start = 0, min_pos = -1, score = 0;
    for (unsigned base = 0; base < len; base += NG) {
        const unsigned pos = base + (unsigned)lane;
        int sc = 0;
        if (pos < len) sc = mat[qv.strand(qo + (int)pos) * 5 + tv.strand(to + (int)pos)];
        const int cnt = (int)(len - base < (unsigned)NG ? len - base : (unsigned)NG);
        for (int k = 0; k < cnt; ++k) {
            score += NUCL_SHFL(sc, k);
            if (score <= 0) { score = 0; min_pos = (int)base + k; }
            if (score > max_score) { max_end = (int)base + k; max_start = min_pos + 1; max_score = score; }
        }
    }
    start = max_start;
    end = max_end;
    best = max_score;
}

struct Seed {
    int start, end, diagonal;
    unsigned score, dist;
};

NUCL_HD Seed seed_on_diagonal(const SeqView &qv, unsigned qlen, const SeqView &tv, unsigned tlen, int diagonal, const int8_t *mat) {
    Seed r;
    r.start = -1; r.end = -1; r.score = 0;
    r.dist = (unsigned)(diagonal < 0 ? -diagonal : diagonal);
    r.diagonal = diagonal;
    int s, e, sc;
    if (diagonal >= 0 && r.dist < qlen) {
        const unsigned len = tlen < qlen - r.dist ? tlen : qlen - r.dist;
        seed_segment(qv, (int)r.dist, tv, 0, len, mat, s, e, sc);
        r.start = s; r.end = e; r.score = (unsigned)sc;
    } else if (diagonal < 0 && r.dist < tlen) {
        const unsigned len = tlen - r.dist < qlen ? tlen - r.dist : qlen;
        seed_segment(qv, 0, tv, (int)r.dist, len, mat, s, e, sc);
        r.start = s; r.end = e; r.score = (unsigned)sc;
    }
    return r;
}

// The ungapped seed of BandedNucleotideAligner::align (:98-113).  Plain: every 65536-shift of the 16-bit prefilter diagonal that
// fits (computeUngappedAlignment, DistanceCalculator.h:93-112).  Wrapped scoring: the query is its sequence written twice - where
// it is at least twice the target, every window of half its length that starts at a shift of the diagonal is laid on the target
// from position 0 (computeUngappedWrappedAlignment, :56-90; the loop bounds are the reference's unsigned comparisons), otherwise
// the plain seed over the first half.
NUCL_HD Seed pick_seed(const SeqView &qv, int qlen, const SeqView &tv, int tlen, unsigned diag16, bool wrapped, const int8_t *mat) {
    Seed best;
    best.start = -1; best.end = -1; best.score = 0; best.dist = 0; best.diagonal = 0;
    if (wrapped && qlen >= tlen * 2) {
        const unsigned half = (unsigned)qlen / 2u;
        const unsigned len = (unsigned)tlen < half ? (unsigned)tlen : half;
        for (int pass = 0; pass < 2; pass++)
            for (unsigned d = pass == 0 ? 1u : 0u;
                 pass == 0 ? (0u - d * 65536u + diag16) > 0u - (unsigned)tlen : (d * 65536u + diag16) < half; d++) {
                const int real = pass == 0 ? (int)((0u - d * 65536u + diag16) + half) : (int)(d * 65536u + diag16);
                Seed t;
                t.dist = (unsigned)(real < 0 ? -real : real);
                t.diagonal = real;
                int s, e, sc;
                seed_segment(qv, real, tv, 0, len, mat, s, e, sc);
                t.start = s; t.end = e; t.score = (unsigned)sc;
                if (t.score > best.score) best = t;
            }
        return best;
    }
    const unsigned ql = wrapped ? (unsigned)qlen / 2u : (unsigned)qlen;
    for (unsigned d = 1; d <= 1u + (unsigned)tlen / 32768u; d++) {
        const Seed t = seed_on_diagonal(qv, ql, tv, (unsigned)tlen, (int)(0u - d * 65536u + diag16), mat);
        if (t.score > best.score) best = t;
    }
    for (unsigned d = 0; d <= ql / 65536u; d++) {
        const Seed t = seed_on_diagonal(qv, ql, tv, (unsigned)tlen, (int)(d * 65536u + diag16), mat);
        if (t.score > best.score) best = t;
    }
    return best;
}

// ---- BandedNucleotideAligner::align (:76-263) for the pairs of a call: align_pairs<F> and its steps.  A form F supplies
//   F::Lds                       the LDS of one alignment
//   F::extz2<WITH_P>(...)        ksw_extz2_sse, all lanes
//   F::walk(...)                 the backtrack, all lanes; the number of letters in every lane
//   F::lane0(v)                  lane 0's value in every lane

// the two sequences of a pair from their first letters, with the letters one past their ends (the pair's own or the call's)
NUCL_HD void pair_views(const NuclLaunch &L, const mmgpu_nucl_pair &P, SeqView &qv, SeqView &tv) {
    qv.base = L.q_res + L.q_off[P.query];
    qv.rl = P.reverse ? L.rev_lookup : nullptr;
    qv.L = (int)(L.q_off[P.query + 1] - L.q_off[P.query]);
    qv.off = 0; qv.past = (P.past_end & 0x80u) ? (int)(P.past_end & 7u) : L.past_end_q; qv.reversed = false;
    tv.base = L.t_res + (size_t)L.t_off4[P.target] * 4;
    tv.rl = nullptr;
    tv.L = (int)L.t_len[P.target];
    tv.off = 0; tv.past = (P.past_end & 0x80u) ? (int)((P.past_end >> 3) & 7u) : L.past_end_t; tv.reversed = false;
}

// first and last position of the seed on the query and on the target
struct SeedEnds {
    int qs, qe, ts, te;
};
NUCL_HD SeedEnds seed_ends(const Seed &s) {
    SeedEnds r;
    if (s.diagonal >= 0) { r.qs = s.start + (int)s.dist; r.qe = s.end + (int)s.dist; r.ts = s.start; r.te = s.end; }
    else { r.qs = s.start; r.qe = s.end; r.ts = s.start + (int)s.dist; r.te = s.end + (int)s.dist; }
    return r;
}

// the letters of an alignment in w[]: in alignment order, or (backwards) last column first as a walk leaves them
struct Letters {
    const char *w;
    int n;
    bool backwards;
    NUCL_HD char at(int i) const { return backwards ? w[n - 1 - i] : w[i]; }
};

// The extensions from a seed that ends at (qe_, te): score, rectangle -> res, the letters -> w[].
template <class F>
NUCL_HD Letters extend(const NuclLaunch &L, const SeqView &qv, const SeqView &tv, int qe_, int te, int orig, typename F::Lds &S,
                          uint8_t *p, char *w, mmgpu_nucl_hit &res) {
    const int qlen = qv.L, tlen = tv.L;
    const bool wrapped = L.wrapped != 0;
    // left extension, score only, on the (shifted) reversed sequences from the seed's end backwards (:165-181)
    const int q_start_rev = qlen - qe_ - 1, t_start_rev = tlen - te - 1;
    SeqView qr = qv, tr = tv;
    qr.reversed = true; qr.off = q_start_rev;
    tr.reversed = true; tr.off = t_start_rev;
    Ez ez, eza;
    // (wrapped scoring: neither extension runs over more than the original query, :171-174,189-191)
    const int q_rev_len = wrapped && qlen - q_start_rev > orig ? orig : qlen - q_start_rev;
    F::template extz2<false>(qr, q_rev_len, tr, tlen - t_start_rev, L.mat, L.gapo, L.gape, L.zdrop, S, nullptr, ez);
    const int q_start = qlen - (q_start_rev + ez.max_q) - 1, t_start = tlen - (t_start_rev + ez.max_t) - 1;
    // right extension with directions from that start (:183-196)
    SeqView qf = qv, tf = tv;
    qf.off = q_start;
    tf.off = t_start;
    int wq = wrapped && qlen - q_start > orig ? orig : qlen - q_start, wt = tlen - t_start;
    F::template extz2<true>(qf, wq, tf, wt, L.mat, L.gapo, L.gape, L.zdrop, S, p, eza);
    // the walk produces the letters last column first; the forward pass wants them reversed, the redone backward pass
    // (CIGAR reversed once more by the caller) as they are
    Letters s = {w, 0, true};
    if (ez.max_q > eza.max_q && ez.max_t > eza.max_t) {
        // the forward pass fell short of the backward pass: the backward pass is redone with directions and
        // its CIGAR reversed (:201-210)
        wq = q_rev_len;
        wt = tlen - t_start_rev;
        F::template extz2<true>(qr, wq, tr, wt, L.mat, L.gapo, L.gape, L.zdrop, S, p, eza);
        s.backwards = false;
    }
    NUCL_SYNC_MEM();   // the direction bytes were written by all lanes
    if (eza.max_t >= 0 && eza.max_q >= 0) s.n = F::walk(p, wq, wt, eza.max_t, eza.max_q, w, S);
    NUCL_SYNC_MEM();
    res.score = eza.max;
    res.q_start = q_start;
    res.q_end = q_start + eza.max_q;
    res.t_start = t_start;
    res.t_end = t_start + eza.max_t;
    return s;
}

// the string in alignment order, zero-terminated, at off of the call's string buffer
NUCL_HD void copy_string(const NuclLaunch &L, unsigned long long off, const Letters &s) {
    const int lane = group_lane();
    for (int i = lane; i < s.n; i += NG) L.bt[off + (unsigned long long)i] = s.at(i);
    if (lane == 0) L.bt[off + (unsigned long long)s.n] = 0;
}

// Identities of an alignment that starts at (q_start, t_start): every lane takes a contiguous chunk of the letters; the letters
// before it say where on the sequences it starts (a prefix over the lanes).  The sum, in every lane.
NUCL_HD unsigned count_identities(const SeqView &qv, const SeqView &tv, int q_start, int t_start, const Letters &s) {
    const int lane = group_lane();
    const int chunk = (s.n + NG - 1) / NG;
    const int c0 = lane * chunk < s.n ? lane * chunk : s.n, c1 = c0 + chunk < s.n ? c0 + chunk : s.n;
    int dq = 0, dt = 0;
    for (int i = c0; i < c1; ++i) {
        const char c = s.at(i);
        dq += c != 'D';
        dt += c != 'I';
    }
    int pq = dq, pt = dt;        // inclusive prefix over the lanes
    for (int d = 1; d < NG; d <<= 1) {
        const int oq = NUCL_SHFL(pq, lane - d), ot = NUCL_SHFL(pt, lane - d);
        if (lane >= d) { pq += oq; pt += ot; }
    }
    int qp = q_start + pq - dq, tp = t_start + pt - dt;
    unsigned ids = 0;
    for (int i = c0; i < c1; ++i) {
        const char c = s.at(i);
        if (c == 'M') { ids += tv.strand(tp) == qv.strand(qp) ? 1u : 0u; ++qp; ++tp; }
        else if (c == 'I') ++qp;
        else ++tp;
    }
    for (int d = 1; d < NG; d <<= 1) ids += (unsigned)NUCL_SHFL_XOR((int)ids, d);
    return ids;
}

// One group of NG lanes: pulls pairs from the queue until it is empty.
template <class F>
NUCL_HD void align_pairs(const NuclLaunch &L, typename F::Lds &S, uint8_t *p, char *w) {
    const int lane = group_lane();
    for (;;) {
        // Every lane takes part in the ticket draw (only lane 0 adds something): with the draw under `if (lane == 0)`
        // the compiler threads the loop-invariant branch through the back edge, the other lanes then come round to the
        // broadcast below without lane 0 and read a stale ticket - the group falls apart and never ends.  The phase
        // boundaries at both ends of the body keep the lanes together across the back edge.
        NUCL_SYNC();
        unsigned pi = NUCL_ATOMIC_ADD_U32(L.next_pair, lane == 0 ? 1u : 0u);
        pi = (unsigned)F::lane0((int)pi);
        if (pi >= L.n_pairs) break;
        const mmgpu_nucl_pair P = L.pairs[L.order[pi]];
        SeqView qv, tv;
        pair_views(L, P, qv, tv);
        // ungapped seed (pick_seed); origQueryLen of the reference: half of a wrapped query
        const bool wrapped = L.wrapped != 0;
        const int orig = wrapped ? qv.L / 2 : qv.L;
        const Seed best = pick_seed(qv, qv.L, tv, tv.L, (unsigned)P.diagonal, wrapped, L.mat);
        const SeedEnds se = seed_ends(best);

        mmgpu_nucl_hit res;
        res.bt_off = 0;
        res.status = MMGPU_NUCL_OK;
        Letters s = {w, 0, false};
        if (se.qe - se.qs == orig - 1 && se.ts == 0 && se.te == tv.L - 1) {
            // the seed spans both sequences (:130-160)
            res.score = (int32_t)best.score;
            res.q_start = se.qs; res.q_end = se.qe; res.t_start = se.ts; res.t_end = se.te;
            for (int i = lane; i < orig; i += NG) w[i] = 'M';
            s.n = orig;
        } else {
            s = extend<F>(L, qv, tv, se.qe, se.te, orig, S, p, w, res);
        }
        NUCL_SYNC_MEM();   // w[] was written by lane 0 (or all lanes), every lane reads it below
        // output: reserve space, copy the string, count identities (:231-258)
        unsigned long long off = NUCL_ATOMIC_ADD_U64(L.bt_cursor, lane == 0 ? (unsigned long long)s.n + 1ull : 0ull);
        off = NUCL_SHFL_U64(off, 0);
        const bool fits = off + (unsigned long long)s.n + 1ull <= L.bt_cap;
        if (fits) copy_string(L, off, s);
        const unsigned ids = count_identities(qv, tv, res.q_start, res.t_start, s);
        if (lane == 0) {
            res.ident = ids;
            res.bt_off = fits ? off : 0ull;
            res.bt_len = (uint32_t)s.n;
            if (!fits) res.status = MMGPU_NUCL_BT_OVERFLOW;
            L.out[L.order[pi]] = res;
        }
        NUCL_SYNC();
    }
}

// One 16-lane group (nucl_kernel.hip, tests/nucl_emu.cpp).  A template only so that an includer with NG = 64, which never calls
// it, does not instantiate the LDS form.
template <class F = LdsForm>
NUCL_HD void align_group(const NuclLaunch &L, typename F::Lds &S, uint8_t *p, char *w) { align_pairs<F>(L, S, p, w); }

}  // namespace NUCL_NS

#endif  // NUCL_HD

}  // namespace mmgpu

#endif
