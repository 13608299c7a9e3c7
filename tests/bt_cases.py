"""Shared by tests/test_bt_formulation.py (CPU), tests/test_bt_gpu.py and tests/bt_gpu_check.py: seeded (query, target) pairs for
the banded traceback (mmgpu_sw_traceback; oracle/sw_oracle.c banded_backtrace_impl), made so that a test can PROVE from the
restatement's final band (`r["band"]` of Oracle.sw_align(..., need_bt=True)) which band class, how many doublings and which
code path of the kernels a pair reached.

 * offsetting indels: q = A + ins(g) + B + C, t = A' + B' + ins'(g) + C' - equal lengths (initial band 1), the path leaves the
   diagonal by g, the band doubles until it is >= g;  with ins' shorter than ins the initial band is not a power of two;
 * one-sided long gaps: q = A + B, t = A' + junk(g) + B' (initial band g + 1, no doubling), and the mirror image (the query is
   the longer one: bands clipped by the target end);
 * homologs with up to 6 indels of up to 25 residues, periodic queries / targets (exact E / F / diagonal ties on the path),
   sequences with X;
 * engineered ties at chosen offsets from the row's first band column (chunk boundaries of the wave kernel), tie_cases().
Primed parts are copies with substitutions only."""
import numpy as np

from mmseqs2_amd import workloads as wl
from oracle.bt_rows import banded_rows
from tests import sw_param_cases as pc

# mmseqs2_amd/csrc: the wave kernel's LDS ring holds 2 * band + 2 <= 1024 columns (bt_wave_kernel.hip BTW_RING); the last tier
# of the lane kernel takes rows of 2 * band + 3 <= 8195 words and 1048576 direction words of 8 cells (mmgpu_api.hip tier_band /
# tier_dir)
WAVE_MAX_BAND = 511
LANE_MAX_BAND = 4096
LANE_MAX_DIR_WORDS = 1048576
BT_OK, BT_TOO_LARGE, BT_FAILED, BT_NO_START = 0, 1, 2, 3       # include/mmgpu.h

BAND_CLASSES = ("1..32", "33..256", "257..511", "512..4096")
DOUBLING_CLASSES = ("0", "1", "2", ">=3")


def _bg(rng, n):
    return rng.choice(20, size=int(n), p=wl.BACKGROUND).astype(np.uint8)


def _subs(rng, s, identity):
    return wl.mutate(rng, s, identity, max_indels=0)


def comp_bias(oracle, v, q):
    """composition bias of q as ssw_init rounds it, from the set's own matrix and background"""
    return oracle.round_comp_bias(oracle.comp_bias(v["mat"].astype(np.int16), v["pback"], q, 1.0))


def offsetting_pair(rng, flank, g, g_t=None, identity=0.9):
    a, b, c = _bg(rng, flank), _bg(rng, flank), _bg(rng, flank)
    q = np.concatenate([a, _bg(rng, g), b, c])
    t = np.concatenate([_subs(rng, a, identity), _subs(rng, b, identity), _bg(rng, g if g_t is None else g_t), _subs(rng, c, identity)])
    return q, t


def one_sided_pair(rng, flank, g, identity=0.9, query_longer=False):
    a, b = _bg(rng, flank), _bg(rng, flank)
    short = np.concatenate([a, b])
    long_ = np.concatenate([_subs(rng, a, identity), _bg(rng, g), _subs(rng, b, identity)])
    return (long_, short) if query_longer else (short, long_)


def homolog_pair(rng, lo, hi):
    q = _bg(rng, rng.integers(lo, hi))
    t = wl.mutate(rng, q, float(rng.uniform(0.4, 0.95)), max_indels=6, max_indel_len=25)
    if rng.random() < 0.5:
        pre = _bg(rng, rng.integers(0, 60))
        t = np.concatenate([pre, t, pre[::-1]])
    return q, t


def path_deviation(bt):
    """the farthest the path of a backtrace string gets from the diagonal of its first cell"""
    b = np.frombuffer(bt.encode(), np.uint8)
    d = np.cumsum((b == ord("D")).astype(np.int64) - (b == ord("I")).astype(np.int64))
    return int(np.abs(d).max()) if len(d) else 0


def classify(r):
    """a finished restatement result (need_bt=True, non-empty string) -> dict(band, band_class, doublings, doubling_class,
    multi_chunk: a band row is wider than the wave's 64 lanes, wide128: wider than two chunks, clipped: the band holds rows
    i <= band + 1 that the target end cuts (i + band >= tlen, i.e. 2 * band + 2 > tlen) - the rows in which the reference's
    zeroed frame slot destroys a valid cell of the last column, the kernels' `zero_last`)"""
    ql, tl, band = r["q_end"] - r["q_start"] + 1, r["t_end"] - r["t_start"] + 1, r["band"]
    b0 = abs(tl - ql) + 1
    n = 0
    while b0 << n < band:
        n += 1
    assert b0 << n == band, (b0, band)
    cls = BAND_CLASSES[0 if band <= 32 else 1 if band <= 256 else 2 if band <= 511 else 3] if band <= LANE_MAX_BAND else ">4096"
    return dict(band=band, rows=ql, band_class=cls, doublings=n, doubling_class=DOUBLING_CLASSES[min(n, 3)],
                multi_chunk=2 * band + 1 > 64, wide128=2 * band + 1 > 128, clipped=2 * band + 2 > tl)


def required_status(rows, band):
    """the status mmgpu_sw_traceback has to give a pair with a start position: OK whenever the last tier of the lane kernel
    holds it (whatever the wave kernel decides), TOO_LARGE when neither kernel can; None where only the wave kernel can and the
    room left in its direction pool decides."""
    if band <= LANE_MAX_BAND and (2 * band + 1 + 7) // 8 * rows <= LANE_MAX_DIR_WORDS:
        return BT_OK
    return BT_TOO_LARGE if band > WAVE_MAX_BAND else None


class Tally:
    """counts of the classes a list of finished cases populated"""

    def __init__(self):
        self.band = dict.fromkeys(BAND_CLASSES, 0)
        self.doublings = dict.fromkeys(DOUBLING_CLASSES, 0)
        self.multi_chunk = self.wide128 = self.clipped = self.with_gap = self.with_bias = self.n = 0

    def add(self, r, cb=None):
        c = classify(r)
        self.band[c["band_class"]] = self.band.get(c["band_class"], 0) + 1
        self.doublings[c["doubling_class"]] += 1
        self.multi_chunk += c["multi_chunk"]
        self.wide128 += c["wide128"]
        self.clipped += c["clipped"]
        self.with_gap += ("I" in r["bt"]) or ("D" in r["bt"])
        self.with_bias += cb is not None and bool(np.any(np.asarray(cb) != 0))
        self.n += 1
        return c

    def __str__(self):
        return "%d strings (%d with gaps, %d with composition bias): band %s, doublings %s, rows of > 64 cells %d, > 128 cells %d, clipped %d" % (
            self.n, self.with_gap, self.with_bias, self.band, self.doublings, self.multi_chunk, self.wide128, self.clipped)


OFFSETTING = [(60, 3), (150, 20), (300, 70), (600, 200), (1200, 400)]       # (flank, g): final bands 4, 32, 128, 256, 512


def raw_pairs(seed, small=False, wide=False, n_other=36):
    """[(label, min path deviation or 0, query, target)].  small: at most ~260 query rows (the serial Python model walks them);
    wide: plus the pairs whose final band lies beyond the wave kernel (512 and 601; lane kernel, last tier)."""
    rng = np.random.default_rng(seed)
    out = []
    if small:
        for rep in range(12):
            for flank, g in [(60, 3), (60, 8), (70, 20), (50, 40)]:
                out.append(("offsetting_%d_%d" % (flank, g), g) + offsetting_pair(rng, flank, g, identity=0.95 if g >= 20 else 0.9))
            out.append(("offsetting_unequal_60_30_12", 30) + offsetting_pair(rng, 60, 30, g_t=12, identity=0.95))
            out.append(("one_sided_90_%d" % (20 + 9 * rep), 0) + one_sided_pair(rng, 90, 20 + 9 * rep))
            out.append(("query_longer_100_%d" % (10 + 5 * rep), 0) + one_sided_pair(rng, 100, 10 + 5 * rep, query_longer=True))
            out.append(("one_sided_25_%d" % (50 + 4 * rep), 0) + one_sided_pair(rng, 25, 50 + 4 * rep, identity=1.0))     # band > tlen / 2
            tiny = _bg(rng, 3)                                           # a 3 x 3 rectangle: 2 * band + 2 = 4 > tlen
            out.append(("tiny_3", 0, tiny, np.concatenate([_bg(rng, 4), tiny, _bg(rng, 4)])))
        lo, hi, cut = 8, 260, 260
    else:
        for flank, g in OFFSETTING[:5 if wide else 4]:
            out.append(("offsetting_%d_%d" % (flank, g), g) + offsetting_pair(rng, flank, g))
        for flank, g in OFFSETTING[:3]:
            out.append(("offsetting_%d_%d_id80" % (flank, g), g) + offsetting_pair(rng, flank, g, identity=0.8))
        out.append(("offsetting_60_1", 1) + offsetting_pair(rng, 60, 1))                       # band 1, no doubling
        out.append(("offsetting_60_2", 2) + offsetting_pair(rng, 60, 2))                       # one doubling
        out.append(("offsetting_unequal_900_300_200", 300) + offsetting_pair(rng, 900, 300, g_t=200, identity=0.95))   # 101 -> 404
        out.append(("offsetting_unequal_150_50_30", 50) + offsetting_pair(rng, 150, 50, g_t=30))                       # 21 -> 84
        out.append(("one_sided_900_300", 0) + one_sided_pair(rng, 900, 300, identity=0.95))                             # 301
        out.append(("one_sided_200_40", 0) + one_sided_pair(rng, 200, 40))
        out.append(("query_longer_300_120", 0) + one_sided_pair(rng, 300, 120, query_longer=True))
        if wide:
            out.append(("one_sided_700_600", 0) + one_sided_pair(rng, 700, 600))                                        # 601
        lo, hi, cut = 13, 900, 1 << 20
    for k in range(n_other):
        kind = ("homolog", "periodic_query", "periodic_target", "with_x", "homolog", "long_insertion")[k % 6]
        if kind == "homolog":
            q, t = homolog_pair(rng, lo, hi)
        elif kind == "long_insertion":
            q = _bg(rng, rng.integers(max(lo, 30), min(hi, 400)))
            p = int(rng.integers(1, len(q)))
            t = np.concatenate([q[:p], _bg(rng, rng.integers(20, 120)), q[p:]])
        else:
            q, t = pc.make_pair(rng, kind)
            q, t = q[:cut], t[:cut + 60]
        out.append((kind, 0, q, t))
    return out


def band_cases(oracle, v, seed, small=False, wide=False, n_other=36, bias_every=1, log=print):
    """-> ([dict(label, q, cb, t, r = the restatement's result with bt / ident / band)], pairs outside the acceptance rule).
    Every pair (every bias_every-th) carries the composition bias of its query from the set's own matrix; an offsetting pair is kept
    only if the restatement's path deviates from the diagonal by the gap it was built with (the alignment spans it)."""
    out, n_refused = [], 0
    for k, (label, dev, q, t) in enumerate(raw_pairs(seed, small, wide, n_other)):
        cb = comp_bias(oracle, v, q) if k % bias_every == 0 else None
        if not pc.rule_accepts(oracle, v["mat"], cb, len(q), v["go"], v["ge"]):
            n_refused += 1
            continue
        r = oracle.sw_align(q, cb, t, v["mat"], v["go"], v["ge"], need_start=True, need_bt=True)
        assert r["score"] < 32767, (label, r["score"])
        if dev and path_deviation(r["bt"]) < dev:
            log("  %s: the alignment does not span the gap at these costs (deviation %d), left out" % (label, path_deviation(r["bt"])))
            continue
        out.append(dict(label=label, q=q, cb=cb, t=t, r=r))
    return out, n_refused


# ---- engineered ties on the path, at chosen offsets from the row's first band column -------------------------------------------
TIE_OFFSETS = (62, 63, 64, 65, 127, 128)      # the last lanes of a 64-lane chunk of the wave kernel and the first ones of the next
TIE_KINDS = ("hd", "ee", "ff", "ef")


def _dissimilar_block(mat, go, ge):
    """(u, v, k): k residues u against k residues v cost more as mismatches than as a gap in each sequence, so the path takes the
    two gaps - in either order at the same score; None where no such k exists (|min score| <= 2 gap_extend)"""
    m = mat[:20, :20].astype(int)
    lo = int(m.min())
    if -lo <= 2 * ge:
        return None
    u, v = (int(x) for x in np.argwhere(m == lo)[0])
    k = 2 * (go - ge) // (-lo - 2 * ge) + 1
    return (u, v, k) if k <= 40 and u != v else None


def tie_recipe(mat, go, ge, kind):
    """what a tie of this kind needs of the matrix and the gap costs, or None (the construction is then skipped for the set):
    'hd'  H between the diagonal and a gap (rule: the diagonal) - a gap whose last residue equals the residue before it can sit
          in two places at one score; any matrix;
    'ee'  a gap between being opened and being extended (rule: extended) - letters (p, s, c) with mat[p, c] - (gap_open -
          gap_extend) == mat[s, c] > 0: "s|c, then a gap over p and the next residue" scores what "a gap over s, p|c, a gap over the
          next residue" scores (sw_param_cases._gap_tie_letters with the difference of the two costs as the price of the trade);
    'ff'  the same with the gap in the target (F instead of E): the mirror image, letters from the transposed matrix;
    'ef'  H between E and F (rule: F unless E is strictly greater) - _dissimilar_block."""
    if kind == "hd":
        return ()
    if kind == "ee":
        return pc._gap_tie_letters(mat, go - ge)
    if kind == "ff":
        return pc._gap_tie_letters(mat.T, go - ge)
    return _dissimilar_block(mat, go, ge)


def _tie_pair(rng, mat, kind, recipe, x, flank=200, g=130, tail=150):
    """one offsetting-indel pair (final band 256: rows of 513 cells, nine chunks) whose first flank holds the construction with
    its tie cell in target column x - rows up to the band start at column 0, so x is also the offset from the row's first band
    column -> (q, t, row of the tie cell)"""
    a = _bg(rng, flank)
    if kind == "hd":
        r = a[x]
        y = next(int(c) for c in rng.permutation(20) if c != a[x - 1] and c != r)
        qa, ta, extra, row = np.concatenate([a[:x + 1], [y, r], a[x + 1:]]), a, 2, x + 2
    elif kind == "ee":
        p_, s_, c_ = recipe
        u2 = int(np.argmin(mat[:20, c_]))
        qa, ta, extra, row = np.concatenate([a[:x], [s_, p_, u2], a[x + 1:]]), np.concatenate([a[:x], [c_], a[x + 1:]]), 2, x + 2
    elif kind == "ff":
        p_, s_, c_ = recipe
        u2, x0 = int(np.argmin(mat[c_, :20])), x - 2
        qa, ta, extra, row = np.concatenate([a[:x0], [c_], a[x0 + 1:]]), np.concatenate([a[:x0], [s_, p_, u2], a[x0 + 1:]]), -2, x0
    else:
        u, v, k = recipe
        s0 = x + 1 - k
        qa, ta, extra, row = np.concatenate([a[:s0], np.full(k, u), a[s0:]]), np.concatenate([a[:s0], np.full(k, v), a[s0:]]), 0, x
    b, c = _bg(rng, tail), _bg(rng, tail)
    q = np.concatenate([qa, _bg(rng, g + max(-extra, 0)), b, c]).astype(np.uint8)           # equal lengths: the initial band is 1
    t = np.concatenate([ta, _subs(rng, b, 0.95), _bg(rng, g + max(extra, 0)), _subs(rng, c, 0.95)]).astype(np.uint8)
    return q, t, row


def tie_cases(oracle, v, seed=5, log=print):
    """-> ([dict(label, kind, x, q, cb=None, t, r)], {kind: reason} for the kinds this set admits no construction for).  One pair
    per kind and offset of TIE_OFFSETS; a pair is kept only when the model's walk (oracle/bt_rows.py, whose string has to be the
    restatement's) consults a tie of that kind in the constructed cell, at that offset, in a row of more than 128 cells -
    random flanks that spoil a construction are redrawn."""
    mat, go, ge = v["mat"], v["go"], v["ge"]
    rng = np.random.default_rng(seed)
    out, skipped = [], {}
    for kind in TIE_KINDS:
        recipe = tie_recipe(mat, go, ge, kind)
        if recipe is None:
            skipped[kind] = "matrix and gap costs %d/%d admit no exact trade" % (go, ge)
            log("  tie construction '%s' skipped: %s" % (kind, skipped[kind]))
            continue
        for x in TIE_OFFSETS:
            for attempt in range(40):
                q, t, row = _tie_pair(rng, mat, kind, recipe, x)
                r = oracle.sw_align(q, None, t, mat, go, ge, need_start=True, need_bt=True)
                if r["q_start"] != 0 or r["t_start"] != 0 or 2 * r["band"] + 1 <= 128:
                    continue
                qs, qe, ts, te = r["q_start"], r["q_end"], r["t_start"], r["t_end"]
                s, on_path = banded_rows(q[qs:qe + 1], None, t[ts:te + 1], mat, go, ge, r["score"], band=r["band"], ties=True)
                assert s == r["bt"], (kind, x)
                if (row, x, x, kind) in on_path:
                    out.append(dict(label="tie_%s_%d" % (kind, x), kind=kind, x=x, q=q, cb=None, t=t, r=r))
                    break
            else:
                raise AssertionError("no pair holds the tie construction '%s' at offset %d" % (kind, x))
    return out, skipped


def profile_query(rng, mat, n):
    """a profile query of n positions: (int8 [20][n] score rows - the substitution row of a random consensus letter, jittered -,
    consensus uint8 [n]) as mmgpu_sw_query.profile / Oracle.sw_align_profile take them"""
    cons = rng.integers(0, 20, n).astype(np.uint8)
    rows = mat[cons][:, :20].astype(np.int32) + rng.integers(-1, 2, (n, 20))
    return np.clip(rows, -30, 30).astype(np.int8).T.copy(), cons


# ---- the device side, shared by tests/test_bt_gpu.py and tests/bt_gpu_check.py -------------------------------------------------
def run_cases(gpu, v, cases, mode=1, min_start_score=0):
    """one query per case against its own target -> the run batch (the caller frees it)"""
    tres, toff = wl.seqs_from_list([c["t"] for c in cases])
    gpu.load_targets(tres, toff, 21)
    queries = [dict(q=c["q"], comp_bias=c["cb"], targets=np.array([i], np.uint32), min_start_score=min_start_score) for i, c in enumerate(cases)]
    b = gpu.sw_prepare(v["mat"], v["go"], v["ge"], queries, mode=mode)
    b.run()
    return b


def check_traceback(b, cases, tag, pick=None):
    """mmgpu_sw_traceback of the picked result slots (all by default) against each case's restatement result r, bit-exact: status
    (required_status from the final band), string, ident, bt_len; the records of the forward / reverse scans are checked on the
    way.  -> (Tally of the compared strings, [mismatch descriptions])"""
    pick = np.arange(len(cases), dtype=np.uint32) if pick is None else np.asarray(pick, np.uint32)
    res = b.fetch()
    info, strs = b.traceback(pick)
    tally, bad = Tally(), []
    for k, p in enumerate(pick.tolist()):
        c, r, h = cases[p], cases[p]["r"], res[p]
        got = tuple(int(h[f]) for f in ("score", "q_end", "t_end", "q_start", "t_start"))
        exp = (r["score"], r["q_end"], r["t_end"], r["q_start"], r["t_start"]) if r["score"] > 0 else (0, r["q_end"], r["t_end"], -1, -1)
        status = int(info[k]["status"])
        if got[:1] + got[3:] != exp[:1] + exp[3:] or (r["score"] > 0 and got != exp):
            bad.append((tag, c["label"], "record", got, exp))
            continue
        if r["score"] <= 0:
            if status != BT_NO_START or strs[k] != "":
                bad.append((tag, c["label"], "status of a pair without a start", status))
            continue
        cl = classify(r)
        want = required_status(cl["rows"], cl["band"])
        if want is None or status != want:
            bad.append((tag, c["label"], "status", status, want, cl))
        elif status == BT_OK:
            if strs[k] != r["bt"] or int(info[k]["ident"]) != r["ident"] or int(info[k]["bt_len"]) != len(r["bt"]):
                first = next((i for i, (x, y) in enumerate(zip(strs[k], r["bt"])) if x != y), min(len(strs[k]), len(r["bt"])))
                bad.append((tag, c["label"], "string", cl, "first difference at op %d" % first, strs[k][max(0, first - 20):first + 20],
                            r["bt"][max(0, first - 20):first + 20], int(info[k]["ident"]), r["ident"]))
            else:
                tally.add(r, c["cb"])
        elif int(info[k]["bt_len"]) != 0 or strs[k] != "":
            bad.append((tag, c["label"], "a string with status", status))
    return tally, bad
