"""Shared by tests/test_nucl_params.py, tests/test_nucl_params_gpu.py, tests/nucl_gpu_check.py and
tests/golden/make_nucl_param_golden.py: the table of (gap open, gap extend, z-drop, matrix) settings the nucleotide alignment
step (mmgpu_nucl_align) is pinned at, the matrices as text, and the seeded generators of the pairs that go through it.

The extension kernel computes in wrapping int8 with a ceiling (mat[0] + 2 (open + extend)), an early return (-min > 2 (open +
extend)) and a carry-in (open) that depend on the setting, it scores with mat[0] / mat[1] only and a wildcard letter at 0, while
the seed uses the whole matrix: the settings vary each of these, the matrices tell the seed and the extension apart (unequal
off-diagonal entries, an N row that is not the mismatch score)."""
import os

import numpy as np

from tests import nucl_common as nc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "nucl_param_vectors.npz")
SEED = 1

LETTERS = "ACTGX"          # column order of the matrix text = numeric codes 0..4 (N reads as X)


def _uniform(match, mismatch, x=None):
    x = mismatch if x is None else x
    return [[x if 4 in (i, j) else (match if i == j else mismatch) for j in range(5)] for i in range(5)]


def _transitions(match, transversion, transition):
    m = _uniform(match, transversion)
    for a, b in ((0, 3), (1, 2)):          # A <-> G, C <-> T
        m[a][b] = m[b][a] = transition
    return m


# the scores as the matrix text states them; what the reference derives from a text (it re-estimates lambda and the
# background and rounds again) is recorded next to it and is what the device gets
MATRICES = {
    "stock": _uniform(2, -3),
    "m1_1": _uniform(1, -1),
    "m2_7": _uniform(2, -7),
    "transitions": _transitions(2, -3, -1),
    "x0": _uniform(2, -3, 0),
}

# (key, gap open, gap extend, z-drop, matrix).  All of them construct in the reference (its e-value set-up aborts the process
# for some others, e.g. 1/1, 0/1 and 4/0 with the stock matrix).
NUCL_PARAM_SETS = [
    ("stock_5_2_zm1", 5, 2, -1, "stock"),
    ("stock_5_2_z0", 5, 2, 0, "stock"),
    ("stock_5_2_z400", 5, 2, 400, "stock"),
    ("stock_10_1_z40", 10, 1, 40, "stock"),
    ("stock_30_30_z40", 30, 30, 40, "stock"),
    ("stock_58_2_z100", 58, 2, 100, "stock"),
    ("m1_1_2_1_z20", 2, 1, 20, "m1_1"),
    ("m2_7_5_2_z40", 5, 2, 40, "m2_7"),
    ("transitions_5_2_z40", 5, 2, 40, "transitions"),
    ("x0_5_2_z40", 5, 2, 40, "x0"),
]
WRAPPED_SETS = ("stock_10_1_z40", "m1_1_2_1_z20")
WRAPPED_CIRCLES = (40, 130, 900)
LENGTHS = (1, 2, 15, 17, 40, 65, 130, 300, 700, 1500)


def set_by_key(key):
    for s in NUCL_PARAM_SETS:
        if s[0] == key:
            return s
    raise KeyError(key)


def matrix_text(rows):
    """the scores as a matrix file of the reference's layout: two comment lines with a background and a lambda, a header line of
    letters, one line per letter.  The background and lambda are the values the reference's own nucleotide matrix file states for
    2/-3 (data of the reference; they also stand in tests/golden/matrices.npz as part of its serialized matrix).  They are
    written for EVERY matrix here, 1/-1 and 2/-7 included, for which they are not the true values: with both lines present the
    reference skips its own estimate (which fails for 1/-1) and derives its int8 matrix as round(lambda * score / ln 2) after
    re-normalising - hence 2/-7 -> 2/-6.  Only that derived matrix, recorded next to the text, reaches the alignments."""
    out = ["# nucleotide scores, written by tests/nucl_param_cases.py",
           "# Background (precomputed optional): 0.2499975 0.2499975 0.2499975 0.2499975 0.00001",
           "# Lambda     (precomputed optional): 0.6337314",
           "   " + "       ".join(LETTERS)]
    for a, row in zip(LETTERS, rows):
        out.append(a + " " + " ".join("%7.4f" % v for v in row))
    return "\n".join(out) + "\n"


def serialized(matrix_key):
    """the "name:data" form RefNucl(serialized=...) takes"""
    return b"nucleotide.out:" + matrix_text(MATRICES[matrix_key]).encode()


def revcomp(s, rl):
    return np.asarray(rl, np.uint8)[np.asarray(s)[::-1]]


def _flanked(rng, t):
    return np.concatenate([rng.integers(0, 4, size=int(rng.integers(0, 100))).astype(np.uint8), t,
                           rng.integers(0, 4, size=int(rng.integers(0, 100))).astype(np.uint8)])


def generate_cases(index, rl):
    """the 120 (q, t, diagonal, reverse, past_q, past_t) of setting number `index`: per length an identical pair, a close one and
    a distant one with N letters (targets with random flanks), both strands, diagonal 0 and a random one"""
    rng = np.random.default_rng([SEED, index])
    out = []
    for L in LENGTHS:
        for variant in range(3):
            base = rng.integers(0, 4, size=L).astype(np.uint8)
            if variant == 0:
                q, t = base, base.copy()
            elif variant == 1:
                q, t = nc.mutate(rng, base, 0.10, 0.03), _flanked(rng, nc.mutate(rng, base, 0.05, 0.02))
            else:
                base[rng.random(L) < 0.05] = 4
                q, t = nc.mutate(rng, base, 0.25, 0.08), _flanked(rng, nc.mutate(rng, base, 0.10, 0.05))
            for reverse in (0, 1):
                tt = revcomp(t, rl) if reverse else t
                for diag in (0, int(rng.integers(-len(tt), len(q) + 1))):
                    out.append((q, tt, diag & 0xFFFF, reverse, int(rng.integers(0, 5)), int(rng.integers(0, 5))))
    return out


def generate_wrapped_cases(index, rl):
    """--wrapped-scoring, the construction of tests/test_nucl_gpu.py test_wrapped_scoring_vs_oracle: one circle per length, the
    doubled query read from another origin against the circle, a piece of it and the circle with a repeated part"""
    rng = np.random.default_rng([SEED, index, 7])
    out = []
    for n in WRAPPED_CIRCLES:
        circle = rng.integers(0, 4, size=n).astype(np.uint8)
        rot = int(rng.integers(0, n))
        q1 = nc.mutate(rng, np.roll(circle, -rot), rng.choice([0.0, 0.04]), rng.choice([0.0, 0.02]))
        q = np.concatenate([q1, q1])
        for t in (nc.mutate(rng, circle, 0.03, 0.01), circle[: max(8, n // 3)].copy(), np.concatenate([circle, circle[: n // 2]])):
            for reverse in (0, 1):
                tt = revcomp(t, rl) if reverse else t
                for diag in (0, rot & 0xFFFF, (-rot) & 0xFFFF, int(rng.integers(0, 65536))):
                    out.append((q, tt, diag, reverse, int(rng.integers(0, 5)), int(rng.integers(0, 5))))
    return out


def pack_cases(d, prefix, cases, expected, bts):
    """cases + results -> arrays under "<prefix>name" (the layout of nucl_vectors.npz)"""
    qs, ts = [c[0] for c in cases], [c[1] for c in cases]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint32)
    d[prefix + "qres"], d[prefix + "qoff"] = np.concatenate(qs).astype(np.uint8), off(qs)
    d[prefix + "tres"], d[prefix + "toff"] = np.concatenate(ts).astype(np.uint8), off(ts)
    d[prefix + "meta"] = np.array([c[2:6] for c in cases], np.int32)
    d[prefix + "expected"] = np.array(expected, np.int32)
    d[prefix + "bt"], d[prefix + "boff"] = np.frombuffer("".join(bts).encode(), np.uint8), off(bts)


def _unpack_cases(d, prefix):
    g = {k: d[prefix + k] for k in ("qres", "qoff", "tres", "toff", "meta", "expected", "bt", "boff")}
    return nc.golden_cases(g)


def load_param_vectors(path=FIXTURE):
    """-> {key: dict(go, ge, zdrop, mat [5, 5] int8, reverse, serialized, cases, wrapped)}; cases / wrapped: lists of
    (q, t, diagonal, reverse, past_q, past_t, expected tuple, backtrace) as nucl_common.golden_cases gives them"""
    d = np.load(path)
    out = {}
    for key, go, ge, zdrop, _ in NUCL_PARAM_SETS:
        if key + "/mat" not in d.files:
            continue
        assert tuple(int(x) for x in d[key + "/costs"]) == (go, ge, zdrop)
        out[key] = dict(go=go, ge=ge, zdrop=zdrop, mat=d[key + "/mat"], reverse=d[key + "/reverse"], serialized=d[key + "/serialized"],
                        cases=_unpack_cases(d, key + "/"), wrapped=_unpack_cases(d, key + "/w_") if key + "/w_meta" in d.files else [])
    return out


def hit_tuple(h):
    return (int(h["score"]), int(h["q_start"]), int(h["q_end"]), int(h["t_start"]), int(h["t_end"]), int(h["ident"]))


def past_end_byte(pq, pt):
    """mmgpu_nucl_pair::past_end (MMGPU_NUCL_PAST_END): the pair carries its own letters past the ends"""
    return 0x80 | (pq & 7) | ((pt & 7) << 3)


def run_cases(gpu, v, cases, wrapped=False):
    """one device call for the cases of one setting, every pair with its own past-end letters -> (hits, strings)"""
    tres = np.concatenate([c[1] for c in cases])
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).astype(np.uint64)
    gpu.load_targets(tres, toff, 5)
    pairs = [(i, i, c[2], c[3], past_end_byte(c[4], c[5])) for i, c in enumerate(cases)]
    # the call's own past-end letters are never the recorded ones' default
    return gpu.nucl_align(v["mat"], v["reverse"], [c[0] for c in cases], pairs, v["go"], v["ge"], v["zdrop"], 2, 1, wrapped=wrapped)


def fixture_mismatches(gpu, v, cases, wrapped=False):
    """-> list of (case number, got, expected) where status, fields or string differ from the fixture"""
    hits, strs = run_cases(gpu, v, cases, wrapped)
    return [(k, int(h["status"]), hit_tuple(h), c[6][:6]) for k, (c, h, s) in enumerate(zip(cases, hits, strs))
            if int(h["status"]) != 0 or hit_tuple(h) != c[6][:6] or s != c[7]]


# ---- queue / slot reuse --------------------------------------------------------------------------------------------------
def queue_pairs(rl, seed=23, n_short=588, n_long=12, long_len=1500):
    """-> (queries, targets, pairs [(query, target, diagonal, reverse, past_end byte)]): distinct pairs of 20 - 200 letters and a
    few of long_len (a short pair then follows a long one into the same wavefront's registers, LDS rings and scratch slice), both
    strands, N letters, right and wrong diagonals"""
    rng = np.random.default_rng(seed)
    queries, targets, pairs = [], [], []
    for k in range(n_short + n_long):
        L = long_len if k % ((n_short + n_long) // n_long) == 0 else int(rng.integers(20, 201))
        base = rng.integers(0, 4, size=L).astype(np.uint8)
        base[rng.random(L) < 0.03] = 4
        start, end = int(rng.integers(0, 60)), int(rng.integers(0, 60))
        t = np.concatenate([rng.integers(0, 4, size=start).astype(np.uint8), nc.mutate(rng, base, 0.04, 0.02),
                            rng.integers(0, 4, size=end).astype(np.uint8)])
        q = nc.mutate(rng, base, 0.08, 0.03)
        reverse = k & 1
        tt = revcomp(t, rl) if reverse else t          # the kernel reverse-complements the query: the flanks swap sides
        diag = (-(end if reverse else start)) & 0xFFFF if rng.random() < 0.7 else int(rng.integers(-len(tt), len(q) + 1)) & 0xFFFF
        queries.append(q)
        targets.append(tt)
        pairs.append((k, k, diag, reverse, past_end_byte(int(rng.integers(0, 5)), int(rng.integers(0, 5)))))
    return queries, targets, pairs


def oracle_results(orc, queries, targets, pairs, mat, rl, go, ge, zdrop, wrapped=False):
    """NuclOracle once per pair -> [(fields, string)]"""
    out = []
    for qi, ti, diag, reverse, pe in pairs:
        pq, pt = (pe & 7, (pe >> 3) & 7) if pe & 0x80 else (4, 4)
        e, bt = orc.align(queries[qi], targets[ti], np.asarray(mat).reshape(-1), rl, go, ge, zdrop, diag, reverse, pq, pt, wrapped=wrapped)
        out.append((e[:6], bt))
    return out


def load_targets(gpu, targets):
    tres = np.concatenate(targets)
    toff = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.uint64)
    gpu.load_targets(tres, toff, 5)


def pair_array(pairs):
    from mmseqs2_amd import capi
    pa = np.zeros(len(pairs), capi.NUCL_PAIR_DTYPE)
    for i, p in enumerate(pairs):
        pa[i] = (p[0], p[1], p[2] & 0xFFFF, p[3], p[4])
    return pa


def tiling_errors(hits, bt_used, cap=None):
    """the strings of the status-0 hits lie in [0, cap) without overlap, each followed by its terminator; without a cap (every
    string fitted) they tile [0, bt_used) exactly"""
    ok = hits[hits["status"] == 0]
    order = np.argsort(ok["bt_off"], kind="stable")
    off, ln = ok["bt_off"][order].astype(np.int64), ok["bt_len"][order].astype(np.int64)
    errs = []
    if len(off) and not np.all(off[1:] >= off[:-1] + ln[:-1] + 1):
        errs.append("strings overlap")
    if len(off) and cap is not None and int((off + ln + 1).max()) > cap:
        errs.append("a string ends beyond the cap")
    if cap is None:
        if len(ok) != len(hits):
            errs.append("a pair overflowed")
        elif len(off) and not (off[0] == 0 and np.all(off[1:] == off[:-1] + ln[:-1] + 1) and off[-1] + ln[-1] + 1 == bt_used):
            errs.append("strings do not tile [0, bt_used)")
    if int((hits["bt_len"].astype(np.int64) + 1).sum()) != int(bt_used):
        errs.append("bt_used %d is not the sum of bt_len + 1 = %d" % (bt_used, int((hits["bt_len"].astype(np.int64) + 1).sum())))
    return errs
