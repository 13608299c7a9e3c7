"""GPU parity (pytest -m gpu) of the wide Smith-Waterman bodies: a query of 449 .. 896 residues is one tile of a 32-lane group
(lane g of 32 owns R = ceil(qlen / 32) rows, four pairs per wavefront, sw_body.h) instead of two tiles of a 16-lane group.  Every
record - score, q_end, t_end, q_start, t_start, word - against the plain-C restatement, bit for bit.

What the cases are chosen for:
  * query lengths on either side of every change of path: 448 (last 16-lane tile), 449 and 480 (R = 15), 481 (R = 16), 768 / 769
    (R = 24 / 25: the kernel groups 1 / 2), 895 and 896 (R = 28, the last wide ones), 897 (the first that is still two tiles);
  * target lengths 1, 3, 4, 5, 31, 32, 33 and 300: the four-letter blocks, and the fill and drain of 32 skewed lanes;
  * lists of 1, 3, 4, 5, 16 and 17 hits (a wavefront takes chunks of 4, a workgroup rounds of 16), and a pair of very unequal targets
    sharing a group;
  * maxima placed in the strips of lanes 15, 16, 17 and 31, and equal maxima on both sides of the lane 15 | 16 boundary, where the
    hand-off crosses the DPP row boundary and the fold over the lanes takes its fifth step;
  * scores just below, at and above the f16 limit of 1792 (marked and unmarked pairs in one job), reverse scans for none, some
    and all pairs of a job, the reverse-only call, forward-only batches;
  * the fused prefilter -> alignment batch and the masked batch with a 600-residue query;
  * the switches MMGPU_SW_WIDE=0 and MMGPU_SW_HALF_WIDE=0 / 1, each in a child process, with records equal to the default's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from tests import sw_param_cases as pc

FIELDS = ("score", "q_end", "t_end", "q_start", "t_start", "word")
LIMIT = 2048 - 256
QUERY_LENS = (448, 449, 480, 481, 768, 769, 895, 896, 897)
TARGET_LENS = (1, 3, 4, 5, 31, 32, 33, 300)
RICH = {"W": 0.25, "C": 0.25, "H": 0.125, "Y": 0.125, "P": 0.125, "I": 0.125}     # BLOSUM62 diagonal 11, 9, 8, 7, 7, 4


def _bg(rng, n):
    return rng.choice(20, size=int(n), p=wl.BACKGROUND).astype(np.uint8)


def _expected(oracle, q, cb, t, mat, go, ge, min_start=0, mode=1):
    r = oracle.sw_align(q, cb, t, mat, go, ge, need_start=True)
    e = tuple(int(r[f]) for f in FIELDS)
    if mode == 0 or e[0] == 0 or e[0] < min_start:
        e = e[:3] + (-1, -1) + e[5:]
    return e


def _run_and_compare(gpu, oracle, mat, go, ge, targets, queries, mode=1, label=""):
    """queries: dicts with q, comp_bias, targets (ids), min_start_score; every record against the restatement"""
    gpu.load_targets(*wl.seqs_from_list(targets), 21)
    out = gpu.sw_batch(mat, go, ge, queries, mode=mode)
    off, scores = 0, []
    for qi, qd in enumerate(queries):
        for k, tid in enumerate(qd["targets"]):
            exp = _expected(oracle, qd["q"], qd["comp_bias"], targets[int(tid)], mat, go, ge, qd["min_start_score"], mode)
            got = tuple(int(out[off + k][f]) for f in FIELDS)
            assert got == exp, (label, mode, "query %d (%d residues)" % (qi, len(qd["q"])), "hit %d" % k, "target %d" % int(tid), got, exp)
            scores.append(exp[0])
        off += len(qd["targets"])
    assert off == len(out)
    return np.array(scores)


def _comp_bias(oracle, P, q):
    return oracle.round_comp_bias(oracle.comp_bias(P["mat"].astype(np.int16), P["pback"], q, 1.0))


# ---- query and target lengths, two parameter sets, both modes -----------------------------------------------------------------
def _length_case(oracle, key):
    P = pc.load_param_vectors()[key]
    rng = np.random.default_rng(449 + sum(map(ord, key)))
    targets = [_bg(rng, n) for n in TARGET_LENS]
    queries = []
    for n in QUERY_LENS:
        q = _bg(rng, n)
        mine = list(range(len(TARGET_LENS)))
        # homologs of the whole query, of its end (the last lane's rows) and of its middle (around the lane 15 | 16 boundary), and a
        # short exact piece
        for piece in (wl.mutate(rng, q, 0.8), wl.mutate(rng, q[n - 120:], 0.9), wl.mutate(rng, q[n // 2 - 60:n // 2 + 60], 0.7), q[n - 33:].copy(),
                      np.concatenate([_bg(rng, 40), wl.mutate(rng, q[100:400], 0.6), _bg(rng, 15)])):
            mine.append(len(targets))
            targets.append(piece)
        queries.append(dict(q=q, comp_bias=_comp_bias(oracle, P, q), targets=np.array(mine, np.uint32), min_start_score=0))
    return P, targets, queries


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("key", ["blosum62_11_1", "pam30_25_2"])
def test_query_and_target_lengths(gpu, oracle, key, mode):
    P, targets, queries = _length_case(oracle, key)
    scores = _run_and_compare(gpu, oracle, P["mat"], P["go"], P["ge"], targets, queries, mode, key)
    assert (scores > 100).sum() >= 3 * len(QUERY_LENS) and (scores < 30).sum() >= 3 * len(QUERY_LENS)


# ---- list lengths and unequal partners ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_list_lengths_and_unequal_partners(gpu, oracle, matrices):
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(1617)
    q = _bg(rng, 600)
    cb = np.zeros(600, np.int8)
    targets = [wl.mutate(rng, q[a:a + n], 0.8) for a, n in zip(rng.integers(0, 300, 17), rng.integers(20, 300, 17))]
    targets += [q[599:].copy(), wl.mutate(rng, q, 0.9)]              # one residue and the whole query: partners of one group
    lists = [np.arange(n, dtype=np.uint32) for n in (1, 3, 4, 5, 16, 17)] + [np.array([17, 18], np.uint32), np.array([18, 3, 17], np.uint32)]
    queries = [dict(q=q, comp_bias=cb, targets=l, min_start_score=0) for l in lists]
    _run_and_compare(gpu, oracle, mat, 11, 1, targets, queries, 1)


# ---- where the maximum lies -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("qlen", [640, 880])          # R = 20 (kernel group 1) and R = 28 (group 2)
def test_maximum_in_the_strips_around_the_row_boundary(gpu, oracle, matrices, qlen):
    """Composition bias zero, so a copy of q[a:b] ends its alignment in row b - 1.  Lane g of the 32 owns the rows [g R, (g + 1) R):
    one target per lane 14 .. 18, 0, 1, 30 and 31 ends in the strip's first, a middle and its last row.  Ties: a motif planted twice in
    an otherwise random query, the copies ending in lanes (15, 16), (16, 17), (14, 15), (0, 31) and twice in lane 16 - the target is the
    motif, alone and with flanks, so both rows hold the maximum in one column and the smaller row has to win; with the reverse scan's
    rows counted from the query's end the same pairs tie there in the mirrored lanes."""
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(qlen)
    R = (qlen + 31) // 32
    q = _bg(rng, qlen)
    cb = np.zeros(qlen, np.int8)
    targets, queries = [], []
    mine = []
    for lane in (0, 1, 14, 15, 16, 17, 18, 30, 31):
        for row in (lane * R, lane * R + R // 2, lane * R + R - 1):
            if row >= qlen or row < 12:
                continue
            a = max(0, row + 1 - int(rng.integers(12, 70)))
            mine.append(len(targets))
            targets.append(np.concatenate([_bg(rng, rng.integers(0, 8)), q[a:row + 1]]))
    queries.append(dict(q=q, comp_bias=cb, targets=np.array(mine, np.uint32), min_start_score=0))
    n_strip = len(mine)
    motif = _bg(rng, 12)
    for la, lb in ((15, 16), (16, 17), (14, 15), (0, 31), (16, 16)):
        # rows the two copies end in: early in the strip of lane la, late in the strip of lane lb (12 rows apart or more: no overlap)
        ea = max(la * R + (0 if la == lb else 2), 11)
        eb = min(lb * R + R - (1 if la == lb else 3), qlen - 1)
        ea, eb = min(ea, eb), max(ea, eb)
        assert eb - ea >= 12 and sorted((ea // R, eb // R)) == sorted((la, lb))
        qt = _bg(rng, qlen)
        for e in (ea, eb):
            qt[e - 11:e + 1] = motif
        mine = []
        for t in (motif.copy(), np.concatenate([_bg(rng, 5), motif, _bg(rng, 7)]), np.concatenate([motif, _bg(rng, 3), motif])):
            mine.append(len(targets))
            targets.append(t)
        queries.append(dict(q=qt, comp_bias=cb, targets=np.array(mine, np.uint32), min_start_score=0))
    scores = _run_and_compare(gpu, oracle, mat, 11, 1, targets, queries, 1, "qlen %d" % qlen)
    assert (scores[:n_strip] >= 40).all() and (scores[n_strip:] >= int(mat.astype(int)[motif, motif].sum())).all()


# ---- scores around the f16 limit -------------------------------------------------------------------------------------------------
def _engineered(q, mat, values):
    """a target per value: a prefix of q whose self-score reaches it, with substitutions that take off the excess"""
    m = mat.astype(int)
    S = np.concatenate([[0], np.cumsum(m[q, q])])
    out = []
    for v in values:
        n0 = int(np.searchsorted(S, v))
        assert n0 < len(S)
        for n in range(n0, min(n0 + 4, len(q)) + 1):
            t, excess = q[:n].copy(), int(S[n]) - v
            reach = {0: []}
            for pos in range(4, n - 4):
                if excess in reach:
                    break
                a = int(q[pos])
                for s0, path in list(reach.items()):
                    for b in range(20):
                        d = m[a, a] - m[a, b]
                        if d > 0 and s0 + d <= excess and s0 + d not in reach:
                            reach[s0 + d] = path + [(pos, b)]
            if excess in reach:
                break
        for pos, b in reach.get(excess, []):
            t[pos] = b
        out.append(t)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_scores_around_the_f16_limit(gpu, oracle, matrices, mode):
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(1792)
    aa = [chr(c) for c in matrices["num2aa"]]
    q = rng.choice([aa.index(k) for k in RICH], size=500, p=list(RICH.values())).astype(np.uint8)
    cb = np.zeros(500, np.int8)
    wanted = list(range(LIMIT - 2, LIMIT + 3)) + [2047, 2048, 2049]
    targets = _engineered(q, mat, wanted) + [q.copy()] + [q[:k].copy() for k in (30, 90, 150, 200, 260, 400)] + [_bg(rng, 200)]
    ids = np.arange(len(targets), dtype=np.uint32)
    exp = np.array([_expected(oracle, q, cb, t, mat, 11, 1)[0] for t in targets])
    assert set(wanted) <= set(exp.tolist()) and exp.max() > 4000          # the query against itself is well above
    under, over = ids[exp <= LIMIT], ids[exp > LIMIT]
    lists = [ids, under, over, np.append(under[::2], over[0]).astype(np.uint32)]      # mixed, none marked, all marked, exactly one
    queries = [dict(q=q, comp_bias=cb, targets=l, min_start_score=0) for l in lists]
    _run_and_compare(gpu, oracle, mat, 11, 1, targets, queries, mode)


# ---- reverse scans ---------------------------------------------------------------------------------------------------------------
def _reverse_case(oracle, matrices):
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(77)
    q = _bg(rng, 700)
    cb = oracle.round_comp_bias(oracle.comp_bias(mat.astype(np.int16), matrices["blosum62_pback"], q, 1.0))
    targets = [wl.mutate(rng, q[a:a + n], idn) for a, n, idn in zip(rng.integers(0, 400, 20), rng.integers(30, 300, 20), rng.uniform(0.4, 1.0, 20))]
    targets += [_bg(rng, n) for n in (50, 150, 250, 350)]
    return mat, q, cb, targets


@pytest.mark.gpu
def test_reverse_scan_for_none_some_and_all_pairs(gpu, oracle, matrices):
    mat, q, cb, targets = _reverse_case(oracle, matrices)
    ids = np.arange(len(targets), dtype=np.uint32)
    scores = np.array([_expected(oracle, q, cb, t, mat, 11, 1)[0] for t in targets])
    some = int(np.median(scores))
    queries = [dict(q=q, comp_bias=cb, targets=ids, min_start_score=m) for m in (0, some, int(scores.max()) + 1)]
    _run_and_compare(gpu, oracle, mat, 11, 1, targets, queries, 1)
    assert 0 < (scores >= some).sum() < len(scores)


@pytest.mark.gpu
def test_reverse_only_call(gpu, oracle, matrices):
    """mode 2 leaves the int16-range hits (word == 1) without a start; mmgpu_sw_reverse_pairs runs the reverse scan of the named ones"""
    mat, q, cb, targets = _reverse_case(oracle, matrices)
    gpu.load_targets(*wl.seqs_from_list(targets), 21)
    ids = np.arange(len(targets), dtype=np.uint32)
    b = gpu.sw_prepare(mat, 11, 1, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=2)
    b.run()
    got = b.fetch()
    exp = [_expected(oracle, q, cb, t, mat, 11, 1) for t in targets]
    word = np.array([e[5] == 1 for e in exp])
    assert word.sum() >= 6 and (~word).sum() >= 4
    for k, e in enumerate(exp):
        assert tuple(int(got[k][f]) for f in FIELDS) == (e[:3] + (-1, -1) + e[5:] if word[k] else e), k
    pick = np.nonzero(word)[0][::2].astype(np.uint32)
    back = b.reverse_pairs(pick)
    for k, p in enumerate(pick):
        assert tuple(int(back[k][f]) for f in FIELDS) == exp[int(p)], int(p)
    b.free()


# ---- other ways to a batch -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fused_prefilter_batch_with_a_600_residue_query(gpu, oracle, matrices):
    from mmseqs2_amd import capi
    from tests import pf_common as pfc
    from tests import pf_gpu_check as chk
    g = pfc.golden()
    thr = int(g["kmer_thr"])
    chk.load_case(gpu, g, g["tres"], g["toff"], thr)
    ts = wl.split(g["tres"], g["toff"])
    rng = np.random.default_rng(600)
    # 600 residues made of pieces of six targets: their k-mers bring those targets (and their relatives) into the list
    pieces, k = [], 0
    while sum(map(len, pieces)) < 600:
        pieces.append(ts[(37 * k + 5) % len(ts)][:100])
        k += 1
    q = np.concatenate(pieces)[:600].astype(np.uint8)
    mat = matrices["blosum62_sw"]
    cb = capi.host_comp_bias(mat.astype(np.int16), matrices["blosum62_pback"], q, lib=gpu.L)[1]
    short = pfc.golden_queries(g)[0]
    pfq = [dict(q=q, comp_bias=np.zeros(600, np.float32), identity_id=None), dict(q=short["q"], comp_bias=short["comp_bias"], identity_id=None)]
    pfb = gpu.pf_prepare(pfq, thr, max_hits=300, ref_bins=2)
    pfb.run()
    hits, counts, status, _ = pfb.fetch()
    assert int(counts[0]) >= 6
    cb1 = capi.host_comp_bias(mat.astype(np.int16), matrices["blosum62_pback"], short["q"], lib=gpu.L)[1]
    swq = [dict(q=q, comp_bias=cb, min_start_score=30), dict(q=short["q"], comp_bias=cb1, min_start_score=30)]
    fused = gpu.sw_prepare_from_pf(mat, 11, 1, swq, pfb, mode=1)
    fused.run()
    fr = fused.fetch().reshape(2, pfb.max_hits)
    for i, qd in enumerate(swq):
        for k in range(int(counts[i])):
            exp = _expected(oracle, qd["q"], qd["comp_bias"], ts[int(hits[i]["id"][k])], mat, 11, 1, 30)
            assert tuple(int(fr[i, k][f]) for f in FIELDS) == exp, (i, k)
    fused.free()
    pfb.free()


@pytest.mark.gpu
def test_masked_batch_with_a_600_residue_query(gpu, oracle, matrices):
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(601)
    q = _bg(rng, 600)
    cb = oracle.round_comp_bias(oracle.comp_bias(mat.astype(np.int16), matrices["blosum62_pback"], q, 1.0))
    targets, masks, expect = [], [], []
    for k in range(9):
        t = np.concatenate([wl.mutate(rng, q[50:250], 0.9), _bg(rng, 20), wl.mutate(rng, q[300:560], 0.8)])
        spans = [(0, 150 + 7 * k)] if k % 3 else []          # most of the first domain: the second one still aligns
        masked = t.copy()
        for a, b in spans:
            masked[a:b] = 20
        targets.append(t)
        masks.append(spans)
        expect.append(_expected(oracle, q, cb, masked, mat, 11, 1))
    gpu.load_targets(*wl.seqs_from_list(targets), 21)
    b = gpu.sw_prepare_masked(mat, 11, 1, [dict(q=q, comp_bias=cb, targets=np.arange(9, dtype=np.uint32), masks=masks, min_start_score=0)], mode=1)
    b.run()
    got = b.fetch()
    b.free()
    for k, e in enumerate(expect):
        assert tuple(int(got[k][f]) for f in FIELDS) == e, k
    assert min(e[0] for e in expect) > 100


# ---- the switches ------------------------------------------------------------------------------------------------------------------
def _switch_case():
    """queries of 500 and 800 residues (kernel groups 1 and 2) and one of 300, lists with pairs above the f16 limit; -> (mat, targets, queries)"""
    mats = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices.npz")))
    mat = mats["blosum62_sw"]
    rng = np.random.default_rng(20)
    targets, queries = [], []
    for n in (500, 800, 300):
        q = _bg(rng, n)
        mine = []
        for t in [q.copy(), wl.mutate(rng, q, 0.9), q[: n // 2].copy()] + [wl.mutate(rng, q[a:a + 150], 0.7) for a in (0, 100, n - 150)] + [_bg(rng, 120)]:
            mine.append(len(targets))
            targets.append(t)
        queries.append(dict(q=q, comp_bias=np.zeros(n, np.int8), targets=np.array(mine, np.uint32), min_start_score=0))
    return mat, targets, queries


def _switch_run(gpu):
    mat, targets, queries = _switch_case()
    gpu.load_targets(*wl.seqs_from_list(targets), 21)
    return [gpu.sw_batch(mat, 11, 1, queries, mode=mode) for mode in (1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"MMGPU_SW_WIDE": "0"}, {"MMGPU_SW_HALF_WIDE": "0"}, {"MMGPU_SW_HALF_WIDE": "1"}])
def test_switches_leave_the_records_unchanged(gpu, tmp_path, env):
    ref = _switch_run(gpu)
    assert ref[0]["score"].max() > LIMIT and (ref[0]["q_start"] >= 0).sum() > 10
    out = str(tmp_path / "records.npy")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=child_env, cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert np.array_equal(got, np.concatenate(ref)), env


if __name__ == "__main__":      # the child of test_switches_leave_the_records_unchanged: the same batches under the parent's environment
    import mmseqs2_amd
    g = mmseqs2_amd.MMGpu(0)
    np.save(sys.argv[1], np.concatenate(_switch_run(g)))
    g.close()
