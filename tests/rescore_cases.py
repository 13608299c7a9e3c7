"""Ungapped diagonal rescoring (`mmseqs rescorediagonal`, include/mmgpu.h "ungapped diagonal rescoring") restated in plain Python:

    serial      the three modes cell by cell and the loop over the candidate diagonals, statement for statement as
                DistanceCalculator::computeUngappedAlignment / ungappedAlignmentByDiagonal / computeSubstitutionStartEndDistance write them
    combine     the kernel's summary of a run of cells and the merge of two adjacent runs (mmseqs2_amd/csrc/rescore_kernel.hip), with its
                tie rules: the LATEST minimum of the prefix sums starts a segment, the EARLIEST maximum of the running score ends it
    accept      the acceptance rule of rescorediagonal.cpp:255-330 in numpy's float32 / float64, the cross-check of mmgpu_host_rescore_accept

and the accessors of tests/golden/rescore.npz (tests/golden/make_rescore_golden.py recorded it from the stock binary)."""
import json
import os
import re

import numpy as np

from tests import ungapped_scan_cases as uc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rescore.npz")
HAMMING, SUBSTITUTION, ALIGNMENT = 0, 1, 2
DEFAULT_RECORD = (0, 0, 0, -1, -1, 0)      # LocalAlignment(): score, diagonal, diag_len, start, end; ident


# ---- serial -----------------------------------------------------------------------------------------------------------------------
def walk(cells):
    """computeSubstitutionStartEndDistance -> (maxScore, maxStartPos, maxEndPos)"""
    max_score = max_end = max_start = 0
    min_pos = -1
    score = 0
    for pos, curr in enumerate(cells):
        score = curr + score
        is_min = score <= 0
        score = 0 if is_min else score
        min_pos = pos if is_min else min_pos
        is_new = score > max_score
        max_end = pos if is_new else max_end
        max_start = min_pos + 1 if is_new else max_start
        max_score = score if is_new else max_score
    return max_score, max_start, max_end


def by_diagonal(q, t, D, mat, mode):
    """ungappedAlignmentByDiagonal -> (score, diagonal, diag_len, start, end), the default record's fields where the diagonal is invalid"""
    dist = abs(D)
    if D >= 0 and dist < len(q):
        n = min(len(t), len(q) - dist)
        qs, ts = dist, 0
    elif D < 0 and dist < len(t):
        n = min(len(t) - dist, len(q))
        qs, ts = 0, dist
    else:
        return 0, D, 0, -1, -1
    qa, ta = q[qs:qs + n], t[ts:ts + n]
    if mode == HAMMING:
        return int(np.sum(qa == ta)), D, n, -1, -1
    score, start, end = walk([int(x) for x in mat[qa, ta]])
    return (score, D, n, start, end) if mode == ALIGNMENT else (score, D, n, -1, -1)


def rescore_hit(q, t, d, mat, mode):
    """computeUngappedAlignment for the stored diagonal d (uint16) -> (score, diagonal, diag_len, start, end, ident)"""
    q, t, mat = np.asarray(q, np.int64), np.asarray(t, np.int64), np.asarray(mat, np.int64)
    d = int(d) & 0xFFFF
    best = DEFAULT_RECORD[:5]
    for div in range(1, 1 + len(t) // 32768 + 1):
        tmp = by_diagonal(q, t, -div * 65536 + d, mat, mode)
        if tmp[0] > best[0]:
            best = tmp
    for div in range(0, len(q) // 65536 + 1):
        tmp = by_diagonal(q, t, div * 65536 + d, mat, mode)
        if tmp[0] > best[0]:
            best = tmp
    ident = 0
    if mode == HAMMING:
        ident = best[0]
    elif mode == ALIGNMENT and best[0] > 0:
        D, s, e = best[1], best[3], best[4]
        qs, ts = (D, 0) if D >= 0 else (0, -D)
        ident = int(np.sum(q[qs + s:qs + e + 1] == t[ts + s:ts + e + 1]))
    return tuple(int(x) for x in best) + (ident,)


def rescore_records(mat, queries, targets, hits, mode):
    """records (capi.RESCORE_HIT_DTYPE) of per-query (target, diagonal) lists, query-major"""
    from mmseqs2_amd import capi
    out = []
    for q, hs in zip(queries, hits):
        for target, d in np.asarray(hs, np.int64).reshape(-1, 2):
            out.append(rescore_hit(q, targets[int(target)], int(d), mat, mode))
    return np.array(out, capi.RESCORE_HIT_DTYPE) if out else np.zeros(0, capi.RESCORE_HIT_DTYPE)


# ---- combine ----------------------------------------------------------------------------------------------------------------------
NONE = -(1 << 30)


def kernel_constants():
    """RESCORE_GROUP (lanes per hit) and RESCORE_STEP (cells per load) as the library's source states them"""
    src = open(os.path.join(os.path.dirname(HERE), "mmseqs2_amd", "csrc", "mmgpu_internal.h")).read()
    out = {}
    for name in ("RESCORE_GROUP", "RESCORE_STEP"):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def lane_run(n):
    """cells per lane of a diagonal of n cells"""
    K = kernel_constants()
    per = -(-n // K["RESCORE_GROUP"])
    return -(-per // K["RESCORE_STEP"]) * K["RESCORE_STEP"]


def lane_cuts(n):
    """the positions at which the kernel cuts a diagonal of n cells into its lanes' runs"""
    run = lane_run(n)
    return [c for c in range(run, n, run)]


# a summary: (sum, mn, mn_pos, mx, mx_pos, best, best_end, best_start, matches) of a run [s, e), positions along the diagonal
def empty(pos):
    return (0, 0, pos - 1, NONE, pos, NONE, pos, pos, 0)


def cell(c, pos, equal=0):
    low = c <= 0
    mn, mn_pos = (c, pos) if low else (0, pos - 1)
    return (c, mn, mn_pos, c, pos, c - mn, pos, mn_pos + 1, int(equal))


def combine(A, B):
    a_sum, a_mn, a_mn_pos, a_mx, a_mx_pos, a_best, a_end, a_start, a_eq = A
    b_sum, b_mn, b_mn_pos, b_mx, b_mx_pos, b_best, b_end, b_start, b_eq = B
    mn, mn_pos = (a_sum + b_mn, b_mn_pos) if a_sum + b_mn <= a_mn else (a_mn, a_mn_pos)      # the latest minimum
    mx, mx_pos = (a_sum + b_mx, b_mx_pos) if a_sum + b_mx > a_mx else (a_mx, a_mx_pos)       # the earliest maximum
    cross = a_sum - a_mn + b_mx
    if cross > b_best or (cross == b_best and b_mx_pos < b_end):
        in_b = (cross, b_mx_pos, a_mn_pos + 1)
    else:
        in_b = (b_best, b_end, b_start)
    best, end, start = (a_best, a_end, a_start) if a_best >= in_b[0] else in_b
    return (a_sum + b_sum, mn, mn_pos, mx, mx_pos, best, end, start, a_eq + b_eq)


def fold(cells, lo, hi, equal=None):
    """the summary of cells [lo, hi), cell by cell, as a lane folds its run"""
    S = empty(lo)
    for pos in range(lo, hi):
        S = combine(S, cell(int(cells[pos]), pos, 0 if equal is None else equal[pos]))
    return S


def split_walk(cells, cuts, equal=None):
    """the runs between the cuts folded one by one, then merged pairwise in a tree as the lanes exchange them
    -> (score, start, end, matches) as walk() reports them (start = end = 0 when nothing scores above 0)"""
    edges = [0] + sorted(cuts) + [len(cells)]
    parts = [fold(cells, a, b, equal) for a, b in zip(edges[:-1], edges[1:])]
    while len(parts) > 1:
        parts = [combine(parts[k], parts[k + 1]) if k + 1 < len(parts) else parts[k] for k in range(0, len(parts), 2)]
    S = parts[0]
    return (S[5], S[7], S[6], S[8]) if S[5] > 0 else (0, 0, 0, S[8])


# ---- accept -----------------------------------------------------------------------------------------------------------------------
def _seq_id(seq_id_mode, ids, qlen, tlen, aln_len):
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        if seq_id_mode == 1:
            return f(ids) / f(min(qlen, tlen))
        if seq_id_mode == 2:
            return f(ids) / f(max(qlen, tlen))
        return f(ids) / f(aln_len)


def _cov(start, end, n):
    u = lambda x: int(x) & 0xFFFFFFFF
    return np.float32(((min(u(n), max(u(start), u(end))) - min(u(start), u(end)) + 1) & 0xFFFFFFFF)) / np.float32(n)


def accept(rec, qlen, tlen, is_identity, evalue, mode, seq_id_mode=0, min_seq_id=0.0, cov=0.0, cov_mode=0, e=0.001, min_aln_len=0,
           filter_hits=False, score_per_col_thr=0.0):
    """-> the fields of mmgpu_rescore_verdict"""
    f = np.float32
    score, D, dlen, start, end, ident = (int(rec[k]) for k in ("score", "diagonal", "diag_len", "start", "end", "ident"))
    dist = abs(D)
    seq_id, ev, aln_len = 0.0, 0.0, 0
    t_cov, q_cov = f(dlen) / f(tlen), f(dlen) / f(qlen)
    qs = qe = ts = te = 0
    if mode == HAMMING:
        seq_id = float(_seq_id(seq_id_mode, score, qlen, tlen, dlen))
        aln_len = dlen
    else:
        ev = float(evalue)
        if mode == ALIGNMENT:
            aln_len = end - start + 1
            qs, qe, ts, te = (start + dist, end + dist, start, end) if D >= 0 else (start, end, start + dist, end + dist)
            if ev <= e or is_identity:
                seq_id = float(_seq_id(seq_id_mode, ident, qlen, tlen, aln_len))
            q_cov, t_cov = _cov(qs, qe, qlen), _cov(ts, te, tlen)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_col = f(score) / f(dlen)
    thr = f(cov)
    has_cov = {0: q_cov >= thr and t_cov >= thr, 2: q_cov >= thr, 1: t_cov >= thr}.get(cov_mode, True)
    has_seq_id = seq_id >= float(f(min_seq_id) - np.finfo(np.float32).eps)
    has_to_filter = bool(filter_hits) and bool(per_col >= f(score_per_col_thr))
    ok = bool(is_identity) or has_to_filter or (aln_len >= min_aln_len and bool(has_cov) and has_seq_id and ev <= e)
    return dict(accepted=int(ok), aln_len=aln_len, seq_id=float(f(seq_id)), q_cov=float(q_cov), t_cov=float(t_cov), q_start=qs, q_end=qe,
                t_start=ts, t_end=te)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
OPTION_KEYS = ("e", "min_seq_id", "seq_id_mode", "cov", "cov_mode", "min_aln_len", "filter_hits", "score_per_col_thr", "sort_results", "backtrace")


class Golden:
    """tests/golden/rescore.npz"""

    def __init__(self, path=GOLDEN):
        g = self.g = np.load(path)
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.queries = uc.split(g["qres"], g["qoff"])
        self.targets = uc.split(g["tres"], g["toff"])
        self.mat = g["mat_blosum62"]

    def setting_targets(self, s):
        return self.queries if s["same_db"] else self.targets

    def hits(self, s):
        """the prefilter result the setting was run on: per query an int64 [n][2] of (target, diagonal as a short)"""
        tag = "same" if s["same_db"] else "other"
        off = self.g["hit_off_" + tag].astype(np.int64)
        pairs = np.stack([self.g["hit_target_" + tag].astype(np.int64), self.g["hit_diag_" + tag].astype(np.int64)], axis=1)
        return [pairs[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    def options(self, s):
        return {k: s[k] for k in OPTION_KEYS}

    def identity(self, s):
        return list(range(len(self.queries))) if s["same_db"] else None

    def expected(self, k):
        """per query the recorded lines: modes 0 and 1 (target, score, diagonal); mode 2 (target, bits, seqId, evalue, qStart, qEnd, qLen,
        tStart, tEnd, tLen, None - the line does not print alnLen -, the n of the backtrace `nM` or None), laid out as capi.rescore_lists"""
        s, g = self.settings[k], self.g
        off = g["exp_off_%d" % k].astype(np.int64)
        key, score = g["exp_key_%d" % k].astype(np.int64), g["exp_score_%d" % k].astype(np.int64)
        out = []
        if s["effective_mode"] != ALIGNMENT:
            diag = g["exp_diag_%d" % k].astype(np.int64)
            for i in range(len(off) - 1):
                out.append([(int(key[j]), int(score[j]), int(diag[j])) for j in range(off[i], off[i + 1])])
            return out
        sid, ev, pos = g["exp_seqid_%d" % k], g["exp_evalue_%d" % k], g["exp_pos_%d" % k].astype(np.int64)
        bt = g["exp_bt_%d" % k].astype(np.int64) if s["backtrace"] else None
        for i in range(len(off) - 1):
            out.append([(int(key[j]), int(score[j]), float(sid[j]), float(ev[j])) + tuple(int(x) for x in pos[j]) + (None, None if bt is None else int(bt[j]))
                        for j in range(off[i], off[i + 1])])
        return out


_record_cache = {}


def golden_records(G, s):
    """the serial restatement's records over the setting's coverable hits -> (kept hits per query, records); settings that score alike
    share one computation"""
    from mmseqs2_amd import capi
    ts = G.setting_targets(s)
    tl = np.array([len(t) for t in ts], np.int64)
    kept = [capi.rescore_coverable_hits(h, len(q), tl, s["cov"], s["cov_mode"]) for q, h in zip(G.queries, G.hits(s))]
    key = (id(G), s["same_db"], s["effective_mode"], s["cov"], s["cov_mode"])
    if key not in _record_cache:
        _record_cache[key] = rescore_records(G.mat, G.queries, ts, kept, s["effective_mode"])
    return kept, _record_cache[key]


def assert_lines(got, want, mode, tag=""):
    """membership and order exactly, integers exactly; seqId within one unit of the last of its three printed decimals
    (Util::fastSeqIdToBuffer truncates to 1/1000), the E-value within 1e-3 relative (Matcher::resultToBuffer prints %.3E)"""
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (gl, wl) in enumerate(zip(got, want)):
        assert [x[0] for x in gl] == [x[0] for x in wl], (tag, i, [x[0] for x in gl][:12], [x[0] for x in wl][:12])
        for a, b in zip(gl, wl):
            if mode != ALIGNMENT:
                assert tuple(a) == tuple(b), (tag, i, a, b)
                continue
            assert a[:2] == b[:2] and a[4:10] == b[4:10] and a[10] == a[5] - a[4] + 1, (tag, i, a, b)
            assert abs(a[2] - b[2]) <= 0.001, (tag, i, a, b)
            assert abs(a[3] - b[3]) <= 1e-3 * abs(b[3]) + 1e-300, (tag, i, a, b)
            assert (a[11] is None and b[11] is None) or a[11] == "%dM" % b[11], (tag, i, a, b)
