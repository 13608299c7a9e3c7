"""The exhaustive gapped scan (`mmseqs gappedprefilter`, include/mmgpu.h "exhaustive gapped scan") restated over the plain-C oracle:

    window    = targets with min_tlen <= length <= max_tlen                     (Util::canBeCovered as a window of lengths)
    score     = Oracle.sw_batch_score (ssw_align's score1, saturating at 32767) for every target of the window,
                Oracle.sw_score_identical (the int16-wrapping diagonal sum) for the query's own target
    list      = the query's own target, and the targets with score > min_score and score >= min_evalue_score,
                by (score descending, id ascending), cut at max_hits

and the fixture's accessors.  min_evalue_score is the host's translation of computeEvalue(score, qlen) <= -e: the smallest score
that passes (the E-value falls monotonically in the score)."""
import json
import os

import numpy as np

from tests import ungapped_scan_cases as uc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gapped_scan.npz")
FULL_WINDOW = uc.FULL_WINDOW
NEVER = 32768      # min_evalue_score of a query no score of which passes the E-value threshold


def min_evalue_score(evalue_of, qlen, e):
    """the smallest score s in [0, 32767] with evalue_of(s, qlen) <= e, NEVER if there is none; 0 = every score passes"""
    if not evalue_of(32767, qlen) <= e:
        return NEVER
    lo, hi = 0, 32767      # invariant: hi passes
    while lo < hi:
        mid = (lo + hi) // 2
        if evalue_of(mid, qlen) <= e:
            hi = mid
        else:
            lo = mid + 1
    return lo


def raw_scores(oracle, mat, go, ge, qd, targets, window=FULL_WINDOW):
    """int32 [len(targets)] of one query: the Gotoh score inside the window, 0 outside, the identity sum for its own target"""
    tl = np.array([len(t) for t in targets], np.int64)
    inside = np.flatnonzero((tl >= window[0]) & (tl <= window[1]))
    out = np.zeros(len(targets), np.int32)
    tres, toff = uc.pack(list(targets))
    if len(inside):
        if qd.get("profile") is not None:
            prof = np.asarray(qd["profile"], np.int8)
            for t in inside:
                out[t] = oracle.sw_align_profile(prof, qd["q"], targets[t], mat.shape[0], go, ge)["score"]
        else:
            out[inside] = oracle.sw_batch_score(qd["q"], qd.get("comp_bias"), tres, toff, inside.astype(np.uint32), mat, go, ge)[0]
    ident = qd.get("identity_id")
    if ident is not None and window[0] <= tl[ident] <= window[1]:
        out[ident] = score_identical(oracle, mat, qd, targets[ident])
    return out


def score_identical(oracle, mat, qd, t):
    """SmithWaterman::scoreIdentical: the diagonal sum accumulated in a short"""
    if qd.get("profile") is None:
        return int(oracle.sw_score_identical(qd["q"], qd.get("comp_bias"), t, np.ascontiguousarray(mat, np.int8)))
    prof = np.asarray(qd["profile"], np.int64)
    rows = min(prof.shape[0], mat.shape[0] - 1)      # ssw_init zeroes the X row; letters without a row score 0
    s = 0
    for pos, x in enumerate(np.asarray(t, np.int64)):
        s += int(prof[x, pos]) if x < rows else 0
    return ((s + 32768) % 65536) - 32768


def select_list(scores, tlens, window, min_score, min_ev, max_hits, identity=None):
    """-> (ids, scores) of one query's list"""
    scores = np.asarray(scores, np.int64)
    tlens = np.asarray(tlens, np.int64)
    ids = np.arange(len(scores), dtype=np.int64)
    own = ids == (-1 if identity is None else identity)
    adm = (tlens >= window[0]) & (tlens <= window[1]) & (own | ((scores > min_score) & (scores >= min_ev)))
    ids = ids[adm]
    order = np.lexsort((ids, -scores[ids]))[:max_hits]
    return ids[order], scores[ids[order]]


class Golden:
    """tests/golden/gapped_scan.npz (tests/golden/make_gapped_scan_golden.py recorded it from the stock binary)"""

    def __init__(self, path=GOLDEN):
        g = self.g = np.load(path)
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.queries = uc.split(g["qres"], g["qoff"])
        self.targets = uc.split(g["tres"], g["toff"])
        self.qoff = g["qoff"].astype(np.int64)

    def mat(self, s):
        return self.g["mat_" + s["matrix"]]

    def setting_targets(self, s):
        return self.queries if s["same_db"] else self.targets

    def setting_tlens(self, s):
        return np.array([len(t) for t in self.setting_targets(s)], np.int64)

    def setting_queries(self, k):
        """-> list of dicts (q, comp_bias, identity_id, min_evalue_score) of setting k"""
        s = self.settings[k]
        cbs, mev = self.g["qcb_" + s["matrix"]], self.g["minev_%d" % k]
        out = []
        for i, q in enumerate(self.queries):
            cb = cbs[int(self.qoff[i]):int(self.qoff[i + 1])] if s["comp_bias"] else None
            out.append(dict(q=q, comp_bias=cb, identity_id=i if s["same_db"] else None, min_evalue_score=int(mev[i])))
        return out

    def expected(self, k):
        off = self.g["exp_off_%d" % k].astype(np.int64)
        ids, sc = self.g["exp_ids_%d" % k].astype(np.int64), self.g["exp_scores_%d" % k].astype(np.int64)
        return [(ids[off[i]:off[i + 1]], sc[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def scoring_key(s):
    return (s["matrix"], s["comp_bias"], s["gap_open"], s["gap_extend"], s["same_db"])


_raw_cache = {}


def setting_raw_scores(oracle, G, k):
    """full-window raw scores [query][target] of setting k; settings that score alike share one computation"""
    s = G.settings[k]
    key = (id(G), scoring_key(s))
    if key not in _raw_cache:
        ts = G.setting_targets(s)
        _raw_cache[key] = np.stack([raw_scores(oracle, G.mat(s), s["gap_open"], s["gap_extend"], qd, ts) for qd in G.setting_queries(k)])
    return _raw_cache[key]


def restated_lists(oracle, G, k):
    """the lists of setting k by the restatement (coverage only removes targets: the scores of the full window serve every window)"""
    from mmseqs2_amd import capi
    s = G.settings[k]
    raw, tl = setting_raw_scores(oracle, G, k), G.setting_tlens(s)
    out = []
    for i, qd in enumerate(G.setting_queries(k)):
        win = capi.coverage_window(s["cov"], s["cov_mode"], len(qd["q"]), tl)
        out.append(select_list(raw[i], tl, win, s["min_score"], qd["min_evalue_score"], s["max_seqs"], qd["identity_id"]))
    return out


def check_recording(G, oracle):
    """what the recording must show to be worth committing (asserted by the recorder on the reference's output and again by the CPU
    test on the file)"""
    n_big = n_same = 0
    ev_binds, min_binds = [], []
    for k, s in enumerate(G.settings):
        raw, tl = setting_raw_scores(oracle, G, k), G.setting_tlens(s)
        qs, exp = G.setting_queries(k), G.expected(k)
        by_ev = by_min = 0
        for i, (ids, sc) in enumerate(exp):
            n_big += int(np.sum(sc > 255))
            if s["same_db"]:
                n_same += int(i in ids.tolist())
            if s["cov"] != 0:      # (the two counts below are over the full window)
                continue
            other = np.arange(len(tl)) != (i if s["same_db"] else -1)
            by_ev += int(np.sum(other & (raw[i] > s["min_score"]) & (raw[i] < qs[i]["min_evalue_score"])))
            by_min += int(np.sum(other & (raw[i] <= s["min_score"]) & (raw[i] >= qs[i]["min_evalue_score"])))
        if by_ev:
            ev_binds.append(s["name"])
        if by_min:
            min_binds.append(s["name"])
        if s["same_db"]:
            assert n_same == len(exp), (s["name"], n_same)
    assert n_big >= 8, n_big
    assert ev_binds and min_binds, (ev_binds, min_binds)
    return dict(above_255=n_big, evalue_binds_in=ev_binds, min_score_binds_in=min_binds, identity_entries=n_same)


# ---- shapes of the device tests: the kernels' boundaries, not the workload's ----
QUERY_LENGTHS = [8, 127, 128, 129, 255, 256, 257, 512, 513, 1025]      # the tile boundaries of the alignment kernels and a multi-tile query


def sw_job_constants():
    """JOB_HITS, JOB_ROUND and LONG_QUERY as the library's source states them (mmseqs2_amd/csrc/mmgpu_api.hip): the sizes at which the
    dense planner's jobs end, read here so that the tests follow the source"""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "mmseqs2_amd", "csrc", "mmgpu_api.hip")).read()
    out = {}
    for name in ("JOB_HITS", "JOB_ROUND", "LONG_QUERY"):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


# ---- the selection over more ids than one round of the compaction holds, and over a full key array: uc's sequences, this scan's
# scores and list rule ----
CASE_GO, CASE_GE = 11, 1


def _case(name, oracle, min_score, max_hits_of):
    mat = Golden().g["mat_blosum62"]
    C = uc.select_case(name, "gapped", lambda qd, ts: raw_scores(oracle, mat, CASE_GO, CASE_GE, qd, ts), min_score=min_score, min_ev=0)
    C.setdefault("mat", mat)
    if "max_hits" not in C:
        C["max_hits"] = max_hits_of(C)
    return C


def rounds_case(oracle):
    return _case("rounds", oracle, uc.ROUNDS_MIN_SCORE, lambda C: uc.rounds_max_hits(
        *select_list(C["raw"][0], C["tlens"], FULL_WINDOW, uc.ROUNDS_MIN_SCORE, 0, len(C["tlens"]))))


def full_case(oracle):
    return _case("full", oracle, -1, lambda C: dict(full=uc.SELECT_KEYS))
