"""Shared by tests/test_sw_params.py, tests/test_sw_params_gpu.py and tests/golden/make_sw_param_golden.py: the table of
(matrix, gap open, gap extend) settings the Smith-Waterman path is pinned at, and one seeded generator of the pairs that
go through it.

The generator aims at what random background sequences reach only by luck: equal maxima in one column (a periodic query
against a few units), equal maxima along one row (a few units against a periodic target), low-complexity sequences with a
strongly negative composition bias, the letter X, homologs, and queries of more than 512 rows (two or more tiles)."""
import os

import numpy as np

from mmseqs2_amd import workloads as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (key, matrix file of the reference's data directory, gap open, gap extend).  All of them construct in the reference (its
# e-value set-up throws for some pairs, e.g. 7/1 and 4/1) and lie inside the acceptance rule for ordinary queries.
SW_PARAM_SETS = [
    ("blosum62_11_1", "blosum62.out", 11, 1),
    ("blosum62_9_2", "blosum62.out", 9, 2),
    ("blosum62_8_2", "blosum62.out", 8, 2),
    ("blosum62_5_2", "blosum62.out", 5, 2),
    ("blosum62_6_5", "blosum62.out", 6, 5),
    ("blosum62_10_9", "blosum62.out", 10, 9),
    ("blosum62_20_3", "blosum62.out", 20, 3),
    ("blosum45_11_1", "blosum45.out", 11, 1),
    ("blosum80_11_1", "blosum80.out", 11, 1),
    ("pam30_25_2", "PAM30.out", 25, 2),
]

# Settings the reference accepts but whose striped result is not the plain recurrence (gap_open == gap_extend), and
# matrices whose minimum leaves the rule at the chosen costs: the acceptance rule must refuse them.
SW_REFUSED_EQUAL_GAPS = [("blosum62.out", 6, 6), ("blosum62.out", 12, 12), ("blosum62.out", 3, 3)]

# at most this share of a set's queries may be left out as "outside the acceptance rule"
MAX_REFUSED_SHARE = 0.20


def set_by_key(key):
    for s in SW_PARAM_SETS:
        if s[0] == key:
            return s
    raise KeyError(key)


def _bg(rng, n, x_share=0.0):
    p = np.append(wl.BACKGROUND * (1.0 - x_share), x_share)
    return rng.choice(21, size=int(n), p=p).astype(np.uint8)


def _length(rng, long_ok=True):
    r = rng.random()
    if r < 0.45:
        return int(rng.integers(1, 120))
    if r < 0.85 or not long_ok:
        return int(rng.integers(120, 512))
    return int(rng.integers(513, 1100))


def _periodic(rng, unit_len, n):
    unit = _bg(rng, unit_len)
    return np.tile(unit, n // unit_len + 2)[:n], unit


def make_pair(rng, kind, low_complexity=True):
    """one (query, target) of the named kind"""
    if kind == "random":
        return _bg(rng, _length(rng), 0.01), _bg(rng, _length(rng), 0.01)
    if kind == "homolog":
        q = _bg(rng, max(_length(rng), 13))
        t = wl.mutate(rng, q, float(rng.uniform(0.3, 1.0)))
        if rng.random() < 0.5:
            pre = _bg(rng, rng.integers(0, 60))
            t = np.concatenate([pre, t, pre[::-1]])
        return q, t
    if kind == "periodic_query":       # the maximum recurs down one column
        u = int(rng.integers(3, 40))
        q, unit = _periodic(rng, u, _length(rng))
        k = int(rng.integers(1, 4))
        t = np.tile(unit, k)
        if rng.random() < 0.5:
            t = np.concatenate([_bg(rng, rng.integers(0, 30)), t, _bg(rng, rng.integers(0, 30))])
        return q, t
    if kind == "periodic_target":      # the maximum recurs along one row
        u = int(rng.integers(3, 40))
        t, unit = _periodic(rng, u, _length(rng))
        k = int(rng.integers(1, 4))
        q = np.tile(unit, k)
        if rng.random() < 0.5:
            q = np.concatenate([_bg(rng, rng.integers(0, 30)), q, _bg(rng, rng.integers(0, 30))])
        return q, t
    if kind == "two_letter":
        a = rng.choice(20, size=2, replace=False)
        if not low_complexity:
            return make_pair(rng, "random")
        q = a[rng.integers(0, 2, _length(rng, long_ok=False))].astype(np.uint8)
        t = a[rng.integers(0, 2, _length(rng, long_ok=False))].astype(np.uint8)
        return q, t
    if kind == "homopolymer":
        if not low_complexity:
            return make_pair(rng, "homolog")
        a = int(rng.integers(0, 20))
        q = np.full(_length(rng, long_ok=False), a, np.uint8)
        t = _bg(rng, _length(rng))
        p = int(rng.integers(0, len(t)))
        t[p:p + int(rng.integers(1, 80))] = a
        return q, t
    if kind == "with_x":
        q = _bg(rng, _length(rng), 0.08)
        t = wl.mutate(rng, q, float(rng.uniform(0.4, 1.0))) if len(q) > 12 else _bg(rng, _length(rng), 0.08)
        t = t.copy()
        t[rng.random(len(t)) < 0.05] = 20
        return q, t
    raise ValueError(kind)


KINDS = ["random", "homolog", "periodic_query", "periodic_target", "two_letter", "homopolymer", "with_x", "homolog",
         "random", "periodic_query", "periodic_target", "homolog"]


def generate_pairs(seed, n, low_complexity_every=1):
    """n seeded pairs, the kinds in a fixed rotation.  low_complexity_every = k keeps only every k-th two-letter / homopolymer
    pair (the others become random / homolog pairs): for settings at which their composition bias leaves the acceptance rule."""
    rng = np.random.default_rng(seed)
    out, n_low = [], 0
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        low = True
        if kind in ("two_letter", "homopolymer"):
            low = n_low % low_complexity_every == 0
            n_low += 1
        q, t = make_pair(rng, kind, low)
        out.append((kind, q, t))
    return out


def rule_accepts(oracle, mat, cb, qlen, go, ge):
    """the acceptance rule as the restatement states it (oracle/sw_oracle.c mmo_sw_check_params)"""
    from oracle.pyoracle import _ptr
    mat = np.ascontiguousarray(mat, np.int8)
    cbp = None if cb is None else np.ascontiguousarray(cb, np.int8)
    return oracle.L.mmo_sw_check_params(_ptr(mat), mat.shape[0], _ptr(cbp), int(qlen), int(go), int(ge)) == 0


def load_param_vectors():
    """tests/golden/sw_param_vectors.npz -> {key: dict(mat, pback, serialized, go, ge, pairs=[(q, cb, t, expect row)], bt=[str])}"""
    d = np.load(os.path.join(GOLDEN, "sw_param_vectors.npz"))
    out = {}
    for key, _, go, ge in SW_PARAM_SETS:
        qoff, toff = d[key + "/qoff"].astype(np.int64), d[key + "/toff"].astype(np.int64)
        qres, tres, cb, exp = d[key + "/qres"], d[key + "/tres"], d[key + "/cb"], d[key + "/expect"]
        pairs = [(qres[qoff[i]:qoff[i + 1]], cb[qoff[i]:qoff[i + 1]], tres[toff[i]:toff[i + 1]], exp[i]) for i in range(len(exp))]
        assert (int(d[key + "/gap_open"]), int(d[key + "/gap_extend"])) == (go, ge)
        out[key] = dict(mat=d[key + "/mat"], pback=d[key + "/pback"], serialized=d[key + "/serialized"], go=go, ge=ge, pairs=pairs,
                        bt=bytes(d[key + "/bt"]).decode().split("\n"))
    return out


def saturating_pair():
    """the pair of tests/test_sw_gpu.py test_int16_saturation_matches_word_pass plus a target that ends with the query's end"""
    rng = np.random.default_rng(3)
    q = rng.choice(20, size=7000, p=wl.BACKGROUND).astype(np.uint8)
    return q, [q.copy(), q[:3000].copy(), q[-5000:].copy()]


def maximal_length_cases(seed=65):
    """[(name, query, target, expected (q_end, t_end))]: a 300-residue motif planted in a 65535-residue sequence so that it ends
    in the last column / row, alone and with an equal copy earlier (the earlier one wins)."""
    rng = np.random.default_rng(seed)
    motif = rng.choice(20, size=300, p=wl.BACKGROUND).astype(np.uint8)
    big = rng.choice(20, size=65535, p=wl.BACKGROUND).astype(np.uint8)
    last = big.copy()
    last[-300:] = motif
    both = last.copy()
    both[1000:1300] = motif
    return [("target_last", motif, last, (299, 65534)), ("target_tie", motif, both, (299, 1299)),
            ("query_last", last, motif, (65534, 299)), ("query_tie", both, motif, (1299, 299))]


# ---- engineered ties ----------------------------------------------------------------------------------------------
SW_MAX_R = 28      # mmseqs2_amd/csrc/mmgpu_internal.h: rows per lane of the largest tile (16 lanes x SW_MAX_R rows)


def strip_geometry(qlen):
    """pick_class of mmseqs2_amd/csrc/mmgpu_api.hip: -> (R rows per lane, rows per tile = 16 R, tiles)"""
    max_rows = 16 * SW_MAX_R
    n_tiles = (qlen + max_rows - 1) // max_rows
    rows = (qlen + n_tiles - 1) // n_tiles
    R = max(1, (rows + 15) // 16)
    return R, 16 * R, n_tiles


def full_dp(q, cb, t, mat, go, ge):
    """H of the plain recurrence (oracle/sw_oracle.c forward_pass) for every cell, int32 [qlen, tlen]; numpy, column by column.
    Needs go >= ge: a vertical gap is then never better opened from a cell that a vertical gap produced, so the F of a column is
    a running maximum over the cells above."""
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    n = len(q)
    P = mat.astype(np.int32)[t[None, :], q[:, None]] + (0 if cb is None else np.asarray(cb, np.int32)[:, None])
    H = np.zeros((n, len(t)), np.int32)
    hprev = np.zeros(n, np.int32)
    E = np.zeros(n, np.int32)
    k = np.arange(n, dtype=np.int32)
    for j in range(len(t)):
        hd = np.concatenate([[0], hprev[:-1]]) + P[:, j]
        hnf = np.maximum(np.maximum(hd, E), 0)
        run = np.maximum.accumulate(hnf + k * ge)           # max over k' <= k of hnf[k'] + k' ge
        F = np.concatenate([[0], run[:-1] - go - (k[1:] - 1) * ge])
        h = np.maximum(hnf, F)
        E = np.maximum(np.maximum(E - ge, h - go), 0)
        H[:, j] = h
        hprev = h
    return H


def _row_categories(rows, qlen):
    """which kinds of row ties the rows (indices in the order the kernel walks the query) form: (a) two rows of one lane's
    strip, (b) different lanes of one tile, (c) different tiles"""
    R, tile_rows, _ = strip_geometry(qlen)
    lanes = {}
    for r in rows:
        lanes.setdefault(int(r) // tile_rows, []).append((int(r) % tile_rows) // R)
    out = set()
    if len(lanes) > 1:
        out.add("c")
    for ls in lanes.values():
        if len(set(ls)) < len(ls):
            out.add("a")
        if len(set(ls)) > 1:
            out.add("b")
    return out


def classify_ties(q, cb, t, mat, go, ge):
    """-> (forward categories, reverse categories, (score, q_end, t_end, q_start, t_start) by the tie rules) from the full DP.
    (a) - (c) as _row_categories for the rows holding the final maximum in the deciding column, (d) the final maximum recurs
    in a column more than 4 (one four-letter block) after it."""
    H = full_dp(q, cb, t, mat, go, ge)
    s = int(H.max())
    if s == 0:
        return set(), set(), (0, 0, -1, -1, -1)
    cols = np.nonzero(H.max(axis=0) == s)[0]
    t_end = int(cols[0])
    rows = np.nonzero(H[:, t_end] == s)[0]
    q_end = int(rows[0])
    fwd = _row_categories(rows, len(q))
    if cols[-1] - t_end > 4:
        fwd.add("d")
    # reverse scan: q[0..q_end] x t[0..t_end] walked backwards; the kernel's rows are those of the reversed WHOLE query
    qr, tr = np.asarray(q)[:q_end + 1][::-1], np.asarray(t)[:t_end + 1][::-1]
    cbr = None if cb is None else np.asarray(cb)[:q_end + 1][::-1]
    Hr = full_dp(qr, cbr, tr, mat, go, ge)
    assert int(Hr.max()) == s
    rcols = np.nonzero(Hr.max(axis=0) == s)[0]
    c0 = int(rcols[0])
    rrows = np.nonzero(Hr[:, c0] == s)[0]
    rev = _row_categories(rrows + (len(q) - 1 - q_end), len(q))
    if rcols[-1] - c0 > 4:
        rev.add("d")
    return fwd, rev, (s, q_end, t_end, q_end - int(rrows[0]), t_end - c0)


def _zero_net_letters(mat):
    """letters (z, x, y, [w ...]) with mat[x, y] == -mat[z, z] < 0 and mat[z, w] == 0: a stretch (x|y), (z|w) ..., (z|z) scores
    -v, 0, ..., +v - the alignment can be prolonged by it without changing its score"""
    m = mat[:20, :20].astype(int)
    for z in range(20):
        ws = [w for w in range(20) if m[z, w] == 0]
        xy = [(x, y) for x in range(20) for y in range(20) if m[x, y] == -m[z, z] and x != z and y != z]
        if len(ws) >= 2 and xy:
            return z, xy[0][0], xy[0][1], ws
    raise ValueError("no zero-net stretch in this matrix")


def _gap_tie_letters(mat, go):
    """letters (p, s, c) with mat[p, c] - go == mat[s, c] > 0, or None: a path that begins (p|c), skips the query residue s with a
    one-residue gap and goes on scores what the path that begins (s|c) scores - the same first column, two adjacent rows"""
    m = mat[:20, :20].astype(int)
    for c in range(20):
        for p_ in range(20):
            for s_ in range(20):
                if p_ != s_ and m[s_, c] > 0 and m[p_, c] - go == m[s_, c]:
                    return p_, s_, c
    return None


def engineered_tie_pairs(mat, go, seed=8):
    """[(name, query, target)]: equal maxima on purpose.  Periodic queries against a few units (the maximum recurs down the
    deciding column every `unit` rows: unit < R -> inside one lane's strip, unit >= R -> across lanes, queries above 448 rows ->
    across tiles), a few units against periodic targets (recurs along a row every `unit` columns), and cores decorated with
    zero-net stretches on both sides (the same score again 6 columns later / earlier, forward and reverse scan); where the
    matrix and gap_open allow it, two adjacent rows of the reverse scan's deciding column."""
    rng = np.random.default_rng(seed)
    out = []
    for qlen, unit, k in [(400, 7, 3), (400, 30, 2), (448, 11, 2), (300, 5, 6), (200, 40, 1), (1000, 13, 3), (1300, 31, 2), (900, 6, 5),
                          (97, 3, 4), (513, 17, 2)]:
        for rep in range(2):
            q, u = _periodic(rng, unit, qlen)
            t = np.tile(u, k)
            if rep:
                t = np.concatenate([_bg(rng, 25), t, _bg(rng, 25)])
            out.append(("periodic_query_%d_%d_%d" % (qlen, unit, rep), q, t))
    for tlen, unit, k, flank in [(300, 9, 3, 0), (500, 21, 2, 40), (200, 5, 5, 300), (700, 33, 4, 500), (150, 7, 2, 10)]:
        t, u = _periodic(rng, unit, tlen)
        q = np.concatenate([_bg(rng, flank), np.tile(u, k), _bg(rng, flank)])
        out.append(("periodic_target_%d_%d" % (tlen, unit), q, t))
    z, x, y, ws = _zero_net_letters(mat)
    for n_core, n_zero, q_pad in [(40, 4, 0), (60, 5, 30), (35, 7, 200), (80, 4, 500), (50, 9, 1000)]:
        core = _bg(rng, n_core)
        w = rng.choice(ws, size=n_zero)
        left_q = np.concatenate([[z], np.full(n_zero, z), [x]]).astype(np.uint8)       # outwards from the core: (x|y), (z|w) ..., (z|z)
        left_t = np.concatenate([[z], w, [y]]).astype(np.uint8)
        q = np.concatenate([_bg(rng, q_pad), left_q, core, left_q[::-1], _bg(rng, q_pad // 2)])
        t = np.concatenate([_bg(rng, 20), left_t, core, left_t[::-1], _bg(rng, 20)])
        out.append(("zero_net_%d_%d_%d" % (n_core, n_zero, q_pad), q, t))
    # reverse scan, two rows of its deciding column: only where the matrix and gap_open allow the exact trade (BLOSUM62 at 5/2: F|F,
    # a gap over W = W|F).  The pair of rows is moved over every lane boundary of a 600-row query and over its tile boundary.
    letters = _gap_tie_letters(mat, go)
    if letters is not None:
        p_, s_, c_ = letters
        n, n_core = 600, 45
        R, tile_rows, _ = strip_geometry(n)
        at_tile = n - 2 - (tile_rows - 1)          # row of p whose successor is the last reversed row of the first reversed tile
        for row in list(range(at_tile - R - 2, at_tile + R + 3)) + [3, 150]:
            core = _bg(rng, n_core)
            q = np.concatenate([_bg(rng, row), [p_, s_], core, _bg(rng, n - row - 2 - n_core)]).astype(np.uint8)
            t = np.concatenate([_bg(rng, 15), [c_], core, _bg(rng, 15)]).astype(np.uint8)
            out.append(("gap_tie_%d" % row, q, t))
    return out
