"""The exhaustive ungapped scan (`mmseqs ungappedprefilter`, include/mmgpu.h "exhaustive ungapped scan") restated in plain numpy:
the per-pair score by the cell recurrence, the list rule, the fixture's accessors and the edge cases of the device tests.

    p(i, x) = mat[x][q[i]] + cb[i]          B = |min(0, min mat)| + |min(0, min cb)|          cap = 255 - B
    S(i, j) = max(0, min(cap, S(i-1, j-1) + p(i, t[j])))                                        score = max S (0: empty target)
    list    = targets inside the length window with score > min_score, plus the query's own target inside the window,
              by (score descending, id ascending), cut at max_hits
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ungapped_scan.npz")
FULL_WINDOW = (0, 0xFFFFFFFF)


def split(res, off):
    return [res[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def bias_of(mat, cb):
    """profile->bias of ssw_init for a sequence query"""
    b = abs(min(0, int(np.min(mat))))
    if cb is not None and len(cb):
        b += abs(min(0, int(np.min(cb))))
    return b


def scores_one_query(mat, q, cb, targets):
    """scores of one query against a list of targets: uint8 [len(targets)].  All targets advance together, one column per step."""
    mat = np.asarray(mat, np.int32)
    alphabet = mat.shape[0]
    q = np.asarray(q, np.int64)
    cbv = np.zeros(len(q), np.int32) if cb is None else np.asarray(cb, np.int32)
    cap = 255 - bias_of(mat, cb)
    assert cap > 0
    P = np.vstack([mat[:, q] + cbv[None, :], np.zeros((1, len(q)), np.int32)])      # row `alphabet`: past a target's end
    nt = len(targets)
    lens = np.array([len(t) for t in targets], np.int64)
    order = np.argsort(-lens, kind="stable")      # longest first: the targets still running are a prefix
    L = int(lens.max()) if nt else 0
    T = np.full((nt, L), alphabet, np.int64)
    for k, o in enumerate(order):
        T[k, :lens[o]] = targets[o]
    S = np.zeros((nt, len(q)), np.int32)
    best_sorted = np.zeros(nt, np.int32)
    for j in range(L):
        n = int(np.sum(lens > j))
        add = P[T[:n, j]]
        new = np.empty((n, len(q)), np.int32)
        new[:, 0] = add[:, 0]
        new[:, 1:] = S[:n, :-1] + add[:, 1:]
        S[:n] = np.clip(new, 0, cap)
        best_sorted[:n] = np.maximum(best_sorted[:n], S[:n].max(axis=1))
    best = np.zeros(nt, np.int32)
    best[order] = best_sorted
    return best.astype(np.uint8)


def pair_score_cells(mat, q, cb, t):
    """the same number cell by cell (slow; the cross-check of the vector form)"""
    mat = np.asarray(mat, np.int32)
    cap = 255 - bias_of(mat, cb)
    S = [[0] * (len(t) + 1) for _ in range(len(q) + 1)]
    best = 0
    for i in range(1, len(q) + 1):
        for j in range(1, len(t) + 1):
            p = int(mat[t[j - 1], q[i - 1]]) + (0 if cb is None else int(cb[i - 1]))
            S[i][j] = max(0, min(cap, S[i - 1][j - 1] + p))
            best = max(best, S[i][j])
    return best


def select_list(scores, tlens, window, min_score, max_hits, identity=None):
    """-> (ids, scores) of one query's list"""
    scores = np.asarray(scores, np.int64)
    tlens = np.asarray(tlens, np.int64)
    ids = np.arange(len(scores), dtype=np.int64)
    lo, hi = window
    adm = (tlens >= lo) & (tlens <= hi) & ((scores > min_score) | (ids == (-1 if identity is None else identity)))
    ids = ids[adm]
    order = np.lexsort((ids, -scores[ids]))[:max_hits]
    return ids[order], scores[ids[order]]


class Golden:
    """tests/golden/ungapped_scan.npz (tests/golden/make_ungapped_scan_golden.py recorded it from the stock binary)"""

    def __init__(self, path=GOLDEN):
        g = self.g = np.load(path)
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.queries = split(g["qres"], g["qoff"])
        self.targets = split(g["tres"], g["toff"])
        self.tlens = np.diff(g["toff"].astype(np.int64))
        self.qoff, self.toff = g["qoff"].astype(np.int64), g["toff"].astype(np.int64)

    def mat(self, s):
        return self.g["mat_" + s["matrix"]]

    def setting_targets(self, s):
        """the target set of a setting: the targets, or - in the same-database run - the query set itself"""
        return self.queries if s["same_db"] else self.targets

    def setting_tlens(self, s):
        return np.array([len(t) for t in self.setting_targets(s)], np.int64)

    def setting_queries(self, s):
        """-> list of dicts (q, comp_bias, identity_id) of a setting; in the same-database run a query's own entry is its identity"""
        seqs, off, cbs = self.queries, self.qoff, self.g["qcb_" + s["matrix"]]
        out = []
        for k, q in enumerate(seqs):
            cb = cbs[int(off[k]):int(off[k + 1])] if s["comp_bias"] else None
            out.append(dict(q=q, comp_bias=cb, identity_id=k if s["same_db"] else None))
        return out

    def expected(self, k):
        """-> per query (ids, scores) of setting k"""
        off = self.g["exp_off_%d" % k].astype(np.int64)
        ids, sc = self.g["exp_ids_%d" % k].astype(np.int64), self.g["exp_scores_%d" % k].astype(np.int64)
        return [(ids[off[i]:off[i + 1]], sc[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def float32_window(cov_thr, cov_mode, qlen, tlens):
    """the window over the lengths present, by the predicate per target (Util::canBeCovered in float32); cov_thr 0 = full window"""
    from mmseqs2_amd import capi
    return capi.coverage_window(cov_thr, cov_mode, qlen, tlens)


def can_be_covered(cov_thr, cov_mode, qlen, tlen):
    """Util::canBeCovered (Util.cpp:542-559) for one pair, restated here so that the tests of capi.coverage_window do not compare
    the binding with itself: float32 operands, float32 division, the quotient compared with the float32 threshold; the second
    halves of modes 3 and 4 compare the float quotient with the double 1.0"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        q, t, thr = f(qlen), f(tlen), f(cov_thr)
        if cov_mode == 0:
            return bool(f(q / t) >= thr and f(t / q) >= thr)
        if cov_mode == 1:
            return bool(f(q / t) >= thr)
        if cov_mode == 2:
            return bool(f(t / q) >= thr)
        if cov_mode == 3:
            return bool(f(t / q) >= thr and float(f(t / q)) <= 1.0)
        if cov_mode == 4:
            return bool(f(q / t) >= thr and float(f(q / t)) <= 1.0)
        if cov_mode == 5:
            return bool(f(min(t, q) / max(t, q)) >= thr)
    return True


def check_recording(G):
    """what the recording must show to be worth committing (asserted by the generator on the reference's output and again by the CPU
    test on the file)"""
    by_name = {s["name"]: k for k, s in enumerate(G.settings)}
    n_sat = n_cut = n_ident_low = n_empty = n_cov = 0
    for k, s in enumerate(G.settings):
        qs = G.setting_queries(s)
        exp = G.expected(k)
        for qi, (ids, sc) in enumerate(exp):
            cap = 255 - bias_of(G.mat(s), qs[qi]["comp_bias"])
            n_sat += int(np.sum(sc == cap))
            n_empty += int(len(ids) == 0)
            if s["same_db"]:
                own = sc[ids == qi]
                n_ident_low += int(len(own) == 1 and own[0] <= s["min_score"])
    base, small = G.expected(by_name["base"]), G.expected(by_name["max_seqs_10"])
    for (bi, bs), (si, ss) in zip(base, small):      # cut inside a class: the element behind the cut scores what the last kept one does
        if len(si) == 10 and len(bi) > 10 and bs[10] == ss[9]:
            n_cut += 1
    for name in ("cov_mode_0", "cov_mode_1", "cov_mode_2"):
        for (bi, _), (ci, _) in zip(base, G.expected(by_name[name])):
            n_cov += len(set(bi.tolist()) - set(ci.tolist()))
    assert n_sat >= 8, n_sat
    assert n_cut >= 3, n_cut
    assert n_ident_low >= 1, n_ident_low
    assert n_empty >= 1, n_empty
    assert n_cov >= 1, n_cov
    return dict(saturated=n_sat, cut_in_class=n_cut, identity_at_or_below=n_ident_low, empty=n_empty, dropped_by_coverage=n_cov)


# ---- shapes of the device tests: the kernel's boundaries, not the workload's ----
TILE_ROWS = (128, 256, 384, 512)      # query rows of the one-tile kernels (16 lanes x 8, 16, 24, 32)
QUERY_LENGTHS = sorted(set([1, 2, 15, 16, 17] + [r + d for r in TILE_ROWS for d in (-1, 0, 1)] + [2 * 512 + 1, 3 * 512]))
TARGET_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65]
ROUND_TARGETS = 32       # targets a workgroup scores at once
JOB_TARGETS = 512        # targets of a one-tile job


def random_seq(rng, n, alphabet=20):
    return rng.integers(0, alphabet, n).astype(np.uint8)


def mutate(rng, seq, keep):
    out = seq.copy()
    flip = rng.random(len(seq)) > keep
    out[flip] = rng.integers(0, 20, int(flip.sum()))
    return out


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if seqs and off[-1] else np.zeros(0, np.uint8)
    return res, off


# ---- lists of the device tests (both scans and the profile queries compare them the same way) ----
def lists_of(hits, counts):
    return [(hits[k]["id"][:int(counts[k])].astype(np.int64), hits[k]["score"][:int(counts[k])].astype(np.int64)) for k in range(len(counts))]


def assert_lists(got, want, tag=""):
    assert len(got) == len(want)
    for k, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (tag, k, gi[:12], wi[:12], gs[:12], ws[:12])


# ---- the selection over more ids than one round of the compaction holds, and over a full key array ----
SELECT_ROUND = 1024      # ids the selection kernels compact per round
SELECT_KEYS = 4096       # keys they sort: the largest max_hits
ROUNDS_TIE_IDS = np.concatenate([np.arange(1000, 1061), np.arange(2030, 2071)])      # on both sides of ids 1024 and 2048
ROUNDS_BETTER_IDS = np.array([3, 500, 999, 1061, 1500, 2029, 2071, 2099])             # in every round, around the tie class
ROUNDS_MIN_SCORE = 15


def rounds_sequences():
    """-> (queries, targets): 2100 targets of length 5 .. 40; a class of identical targets at ROUNDS_TIE_IDS that query 0 contains, a
    few targets that hold more of query 0 and so score above the class, and an unrelated query 1"""
    rng = np.random.default_rng(31)
    ts = [random_seq(rng, int(n)) for n in rng.integers(5, 41, 2100)]
    q0 = random_seq(rng, 64)
    tied = q0[20:46].copy()
    for i in ROUNDS_TIE_IDS:
        ts[i] = tied.copy()
    for k, i in enumerate(ROUNDS_BETTER_IDS):
        ts[i] = q0[17 - k:47 + k // 2].copy()      # (distinct lengths of 30 .. 40: distinct scores above the class's)
    return [dict(q=q0), dict(q=random_seq(rng, 50))], ts


def rounds_max_hits(ids, scores):
    """the values of max_hits of the rounds case, from query 0's whole list (ids, scores as select_list gives them for a max_hits
    above the admitted count): the cut falls inside the tie class so that the last member kept is (a) before id 1023, (b) id 1023,
    the last of the first round, (c) id 1024, the first of the second, (d) in 2048 .. 2069, in the third; (all) above the count"""
    member = np.isin(ids, ROUNDS_TIE_IDS)
    first = int(np.flatnonzero(member)[0])      # the class is contiguous in the list and in id order
    assert member[first:first + len(ROUNDS_TIE_IDS)].all() and np.array_equal(ids[first:first + len(ROUNDS_TIE_IDS)], ROUNDS_TIE_IDS)

    def upto(last_id):
        return first + int(np.flatnonzero(ROUNDS_TIE_IDS == last_id)[0]) + 1
    return dict(a=upto(1009), b=upto(1023), c=upto(1024), d=upto(2052), all=len(ids) + 7)


def last_tie_member(ids):
    """the highest id of the tie class in a list, and how many of the class the list holds"""
    kept = ids[np.isin(ids, ROUNDS_TIE_IDS)]
    return int(kept.max()), len(kept)


def full_sequences():
    """-> (queries, targets): 4200 short targets, all of which a scan with min_score = -1 admits: a list of SELECT_KEYS entries.  300 of
    them are made of X (letter 20: -1 against everything) and score 0, so the lowest class is the one the cut falls into"""
    rng = np.random.default_rng(32)
    ts = [random_seq(rng, int(n)) for n in rng.integers(5, 21, 4200)]
    for i in rng.choice(4200, 300, replace=False):
        ts[i] = np.full(len(ts[i]), 20, np.uint8)
    return [dict(q=random_seq(rng, 24)), dict(q=random_seq(rng, 9))], ts


_select_cases = {}


def select_case(name, scan, score_fn, **rule):
    """the rounds / the full case of one scan ("ungapped", "gapped"): score_fn(qd, targets) -> raw scores of one query; rule: what the
    scan's select_list takes besides scores, lengths, window and max_hits.  -> dict(queries, targets, tlens, raw [query][target], rule);
    computed once and left unchanged"""
    key = (name, scan)
    if key not in _select_cases:
        qs, ts = rounds_sequences() if name == "rounds" else full_sequences()
        tl = np.array([len(t) for t in ts], np.int64)
        raw = np.stack([np.asarray(score_fn(qd, ts), np.int64) for qd in qs])
        raw.setflags(write=False)
        _select_cases[key] = dict(queries=qs, targets=ts, tlens=tl, raw=raw, rule=rule)
    return _select_cases[key]


def rounds_case():
    mat = Golden().g["mat_blosum62"]
    C = select_case("rounds", "ungapped", lambda qd, ts: scores_one_query(mat, qd["q"], None, ts), min_score=ROUNDS_MIN_SCORE)
    C.setdefault("mat", mat)
    C.setdefault("max_hits", rounds_max_hits(*select_list(C["raw"][0], C["tlens"], FULL_WINDOW, ROUNDS_MIN_SCORE, len(C["tlens"]))))
    return C


def full_case():
    mat = Golden().g["mat_blosum62"]
    C = select_case("full", "ungapped", lambda qd, ts: scores_one_query(mat, qd["q"], None, ts), min_score=-1)
    C.setdefault("mat", mat)
    C.setdefault("max_hits", dict(full=SELECT_KEYS))
    return C


def case_lists(C, select, max_hits):
    """the expected lists of a case for one max_hits, by the scan's select_list"""
    return [select(C["raw"][k], C["tlens"], FULL_WINDOW, max_hits=max_hits, **C["rule"]) for k in range(len(C["queries"]))]
