"""GPU tests of the exhaustive ungapped scan (mmgpu_scan_*): the device's lists against the lists recorded from the stock binary
(tests/golden/ungapped_scan.npz), its raw scores against the numpy restatement (tests/ungapped_scan_cases.py) over shapes chosen for
the kernel's boundaries - rows per lane, tiles, chunks of columns, rounds and jobs of targets - the selection rules, the batch
lifecycle, the hand-over into the alignment batch and the refusals.  Small shapes only."""
import ctypes
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import ungapped_scan_cases as uc
from tests.ungapped_scan_cases import assert_lists, lists_of

pytestmark = pytest.mark.gpu

X = 20


@functools.lru_cache(maxsize=None)
def golden():
    return uc.Golden()


@functools.lru_cache(maxsize=None)
def blosum62():
    return golden().g["mat_blosum62"]


def device_scores(gpu, mat, queries, targets, **kw):
    """load, scan with the full window, -> uint8 [queries][targets] of debug_scores"""
    gpu.load_targets(*uc.pack(targets), 21)
    b = gpu.scan_prepare(mat, queries, **kw)
    b.run()
    out = np.stack([b.debug_scores(k) for k in range(len(queries))])
    b.free()
    return out


def expect_scores(mat, queries, targets):
    return np.stack([uc.scores_one_query(mat, qd["q"], qd.get("comp_bias"), targets) for qd in queries])


def assert_scores(gpu, mat, queries, targets):
    got, want = device_scores(gpu, mat, queries, targets), expect_scores(mat, queries, targets)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(q), int(t), int(got[q, t]), int(want[q, t]), len(queries[q]["q"]), len(targets[t])) for q, t in bad[:8]]
    return want


# ---- 1. the recorded lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_device_lists_equal_the_recorded_lists(gpu, k):
    G = golden()
    s = G.settings[k]
    gpu.load_targets(*uc.pack(G.setting_targets(s)), 21)
    tl = G.setting_tlens(s)
    qs = [dict(qd, window=capi.coverage_window(s["cov"], s["cov_mode"], len(qd["q"]), tl)) for qd in G.setting_queries(s)]
    hits, counts = gpu.scan_batch(G.mat(s), qs, min_score=s["min_score"], max_hits=min(s["max_seqs"], 4096))
    assert hits.shape[1] == min(s["max_seqs"], len(tl)) and not hits["diagonal"].any()
    assert_lists(lists_of(hits, counts), G.expected(k), s["name"])


# ---- 2. query-length boundaries ----------------------------------------------------------------------------------------------
def boundary_case(rng):
    """every query length of uc.QUERY_LENGTHS; per query, targets that hold 24 of its residues around the rows where a strip, a
    tile or the query ends, behind prefixes that move the match over the chunks of columns.  The matches score about 120: below
    the cap, so a diagonal broken at a boundary shows."""
    qs, ts = [], []
    for n in uc.QUERY_LENGTHS:
        q = uc.random_seq(rng, n)
        qs.append(dict(q=q, comp_bias=rng.integers(-2, 3, n).astype(np.int8)))
        rows = next((r for r in uc.TILE_ROWS if n <= r), 512) // 16      # rows per lane of the query's kernel
        for centre in sorted({rows, 2 * rows, 15 * rows, 512, 1024, n - 8, n // 2}):
            if 0 < centre < n + 8:
                seg = q[max(0, centre - 12):min(n, centre + 12)]
                ts.append(np.concatenate([uc.random_seq(rng, int(rng.integers(0, 70))), seg, uc.random_seq(rng, int(rng.integers(0, 40)))]))
    return qs, ts


def test_scores_at_the_query_length_boundaries(gpu):
    qs, ts = boundary_case(np.random.default_rng(11))
    want = assert_scores(gpu, blosum62(), qs, ts)
    assert (want > 60).sum() >= len(qs) and (want < 200).all()      # the planted matches are seen and none of them hides behind the cap


# ---- 3. target shapes --------------------------------------------------------------------------------------------------------
def two_queries(rng):
    """a one-tile query and one of two tiles plus a row"""
    return [dict(q=uc.random_seq(rng, 100), comp_bias=rng.integers(-1, 2, 100).astype(np.int8)),
            dict(q=uc.random_seq(rng, 2 * 512 + 1), comp_bias=None)]


def test_short_targets_and_a_long_one(gpu):
    rng = np.random.default_rng(12)
    qs = two_queries(rng)
    ts = [uc.random_seq(rng, n) for n in uc.TARGET_LENGTHS]
    # pad letters must never score: short targets made of the query's own residues, so that a pad read as a letter would add
    ts += [qs[0]["q"][:n].copy() for n in (1, 2, 3, 5, 63, 65)]
    long_t = uc.random_seq(rng, 40003)
    long_t[39970:39994] = qs[0]["q"][40:64]         # matches near the end, over the last chunks of columns
    long_t[20000:20024] = qs[1]["q"][500:524]       # ... and over the first tile boundary of the long query
    long_t[31:55] = qs[1]["q"][1001:1025]           # ... and over the second, into the one row of the third tile
    ts.append(long_t)
    want = assert_scores(gpu, blosum62(), qs, ts)
    assert want[0, 0] == 0 and want[1, 0] == 0 and want[0, -1] > 60 and want[1, -1] > 60


@pytest.mark.parametrize("n", [1, 7, uc.ROUND_TARGETS - 1, uc.ROUND_TARGETS + 1, uc.JOB_TARGETS - 1, uc.JOB_TARGETS + 1])
def test_target_counts_around_a_round_and_a_job(gpu, n):
    """one target; odd counts (a pair with one half empty); one below and above what a workgroup holds at once and per job"""
    rng = np.random.default_rng(100 + n)
    qs = two_queries(rng)
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(1, 90, n)]
    ts[n // 2] = np.concatenate([uc.random_seq(rng, 13), qs[1]["q"][505:530], qs[0]["q"][10:30]])
    assert_scores(gpu, blosum62(), qs, ts)


# ---- 4. special content ------------------------------------------------------------------------------------------------------
def test_x_targets_bias_and_the_cap(gpu):
    rng = np.random.default_rng(13)
    mat = blosum62()
    A = 0
    assert mat[A, A] == 4 and mat.min() == -4
    selfs = {int(mat[a, a]): a for a in range(20)}
    # no composition bias: cap = 251.  60 A + one letter of self score 9 / 11: 249 and 251; 61 A + that letter: 255, capped
    below, at = np.array([A] * 60 + [selfs[9]], np.uint8), np.array([A] * 60 + [selfs[11]], np.uint8)
    above = np.array([A] * 61 + [selfs[11]], np.uint8)
    # a query whose bias alone moves B: one position at -9 -> B = 13, cap = 242
    cb = np.zeros(80, np.int8)
    cb[5] = -9
    qs = [dict(q=below), dict(q=at), dict(q=above), dict(q=np.array([A] * 80, np.uint8), comp_bias=cb), dict(q=uc.random_seq(rng, 50))]
    ts = [below, at, above, np.array([A] * 80, np.uint8), np.full(37, X, np.uint8), np.full(1, X, np.uint8), uc.random_seq(rng, 64)]
    want = assert_scores(gpu, mat, qs, ts)
    assert (want[0, 0], want[1, 1], want[2, 2]) == (249, 251, 251)
    assert want[3, 3] == 242 and uc.bias_of(mat, cb) == 13
    assert not want[:, 4].any() and not want[:, 5].any()      # X scores -1 against everything


# ---- 5. selection ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def selection_case():
    rng = np.random.default_rng(14)
    qs = [dict(q=uc.random_seq(rng, n), comp_bias=None) for n in (40, 90, 200)]
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(5, 120, 150)]
    ts[7] = uc.mutate(rng, qs[1]["q"], 0.7)
    ts[9] = qs[0]["q"][:6].copy()      # the identity target of query 0 in the tests below: scores far below any threshold
    return qs, ts, expect_scores(blosum62(), qs, ts)


def run_lists(gpu, qs, ts, min_score, max_hits):
    gpu.load_targets(*uc.pack(ts), 21)
    return lists_of(*gpu.scan_batch(blosum62(), qs, min_score=min_score, max_hits=max_hits))


@pytest.mark.parametrize("min_score,max_hits", [(15, 1), (15, 150), (15, 400), (-1, 400), (-1, 20), (25, 10)])
def test_selection_against_the_list_rule(gpu, min_score, max_hits):
    qs, ts, sc = selection_case()
    tl = [len(t) for t in ts]
    got = run_lists(gpu, qs, ts, min_score, max_hits)
    assert_lists(got, [uc.select_list(sc[k], tl, uc.FULL_WINDOW, min_score, max_hits) for k in range(len(qs))], (min_score, max_hits))
    if min_score == -1 and max_hits == 400:
        assert all(len(ids) == len(ts) for ids, _ in got)      # every admitted target, score 0 included


def test_equal_scores_come_in_id_order(gpu):
    rng = np.random.default_rng(15)
    t = uc.random_seq(rng, 30)
    ts = [t.copy() for _ in range(77)]
    qs = [dict(q=np.concatenate([uc.random_seq(rng, 9), t[3:25]]))]
    for max_hits in (77, 20, 1):
        (ids, scores), = run_lists(gpu, qs, ts, 15, max_hits)
        assert np.array_equal(ids, np.arange(min(max_hits, 77))) and len(set(scores.tolist())) == 1 and scores[0] > 15


def test_identity_and_windows(gpu):
    qs, ts, sc = selection_case()
    tl = np.array([len(t) for t in ts])
    thr = 33
    # the identity target at the threshold (not above it) is listed, last by its score; outside the window it is not
    inside, outside = (0, 0xFFFFFFFF), (int(tl[9]) + 1, 0xFFFFFFFF)
    assert sc[0, 9] <= thr
    # ... and queries with different windows share a batch
    batch = [dict(qs[0], identity_id=9, window=inside), dict(qs[0], identity_id=9, window=outside), dict(qs[1], window=(30, 60)),
             dict(qs[2], window=(61, 119)), dict(qs[2], window=(0xFFFFFFFF, 0xFFFFFFFF))]
    got = run_lists(gpu, batch, ts, thr, 400)
    want = [uc.select_list(sc[0], tl, inside, thr, 400, 9), uc.select_list(sc[0], tl, outside, thr, 400, 9),
            uc.select_list(sc[1], tl, (30, 60), thr, 400), uc.select_list(sc[2], tl, (61, 119), thr, 400), (np.zeros(0, np.int64),) * 2]
    assert_lists(got, want)
    assert got[0][0][-1] == 9 and 9 not in got[1][0] and len(got[0][0]) == len(got[1][0]) + 1
    assert len(got[2][0]) and len(got[3][0]) and not len(got[4][0])


# ---- 6. lifecycle ------------------------------------------------------------------------------------------------------------
def test_run_twice_and_prepare_again(gpu):
    qs, ts, _ = selection_case()
    gpu.load_targets(*uc.pack(ts), 21)
    b = gpu.scan_prepare(blosum62(), qs, min_score=15, max_hits=50)
    b.run()
    h1, c1, s1 = *b.fetch(), b.debug_scores(1)
    b.run()
    h2, c2, s2 = *b.fetch(), b.debug_scores(1)
    assert h1.tobytes() == h2.tobytes() and c1.tobytes() == c2.tobytes() and s1.tobytes() == s2.tobytes()
    assert b.kernel_ms() > 0
    other = gpu.scan_prepare(blosum62(), qs[:1], min_score=15, max_hits=50)
    other.run()
    with pytest.raises(capi.MMGpuError):      # the context's scratch now holds the other batch's scores
        b.debug_scores(0)
    other.free()
    b.free()
    b = gpu.scan_prepare(blosum62(), qs, min_score=15, max_hits=50)
    b.run()
    h3, c3 = b.fetch()
    b.free()
    assert h1.tobytes() == h3.tobytes() and c1.tobytes() == c3.tobytes()


# ---- 7. hand-over ------------------------------------------------------------------------------------------------------------
def test_lists_go_into_the_alignment_batch_on_the_device(gpu, matrices):
    G = golden()
    s = G.settings[0]
    gpu.load_targets(*uc.pack(G.targets), 21)
    qs = [dict(qd, min_start_score=0) for qd in G.setting_queries(s)[2:10]]
    sw_mat = matrices["blosum62_sw"]
    hits, counts, rec = capi.exhaustive_search(gpu, G.mat(s), sw_mat, 11, 1, qs, min_score=s["min_score"], max_hits=40, mode=1)
    assert_lists(lists_of(hits, counts), [(i[:40], sc[:40]) for i, sc in G.expected(0)[2:10]])
    host = gpu.sw_batch(sw_mat, 11, 1, [dict(qd, targets=hits[k]["id"][:int(counts[k])]) for k, qd in enumerate(qs)], mode=1)
    at = 0
    for k in range(len(qs)):
        n = int(counts[k])
        assert n > 0 and rec[k, :n].tobytes() == host[at:at + n].tobytes(), k
        at += n


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def raw_prepare(g, mat, queries, min_score=15, max_hits=300):
    par, arr, keep = g._scan_marshal(mat, queries, min_score, max_hits)
    h = ctypes.c_void_p(1)
    rc = g.L.mmgpu_scan_prepare(g.ctx, ctypes.byref(par), ctypes.cast(arr, ctypes.c_void_p), len(queries), ctypes.byref(h))
    return rc, h.value


def test_refusals_leave_the_handle_null(gpu):
    import mmseqs2_amd
    rng = np.random.default_rng(16)
    q = dict(q=uc.random_seq(rng, 30))
    fresh = mmseqs2_amd.MMGpu(0)
    try:
        assert raw_prepare(fresh, blosum62(), [q]) == (-3, None)                          # MMGPU_ERR_STATE: no targets loaded
    finally:
        fresh.close()
    gpu.load_targets(*uc.pack([uc.random_seq(rng, 20) for _ in range(5)]), 21)
    assert raw_prepare(gpu, blosum62(), [q], max_hits=4097) == (-4, None)                 # MMGPU_ERR_UNSUPPORTED
    bad = dict(q=np.array([1, 2, 21, 3], np.uint8))
    assert raw_prepare(gpu, blosum62(), [q, bad]) == (-1, None)                           # MMGPU_ERR_ARG: a letter outside the alphabet
    cb = np.full(30, -128, np.int8)
    cb[1] = 127
    assert raw_prepare(gpu, blosum62(), [dict(q, comp_bias=cb)]) == (-1, None)            # max(p) + B > 255
    big = blosum62().astype(np.int16)
    big[big == big.min()] = -128
    assert raw_prepare(gpu, big.astype(np.int8), [dict(q, comp_bias=cb)]) == (-1, None)   # 255 - B <= 0
    rc, h = raw_prepare(gpu, blosum62(), [q])
    assert rc == 0 and h
    gpu.L.mmgpu_scan_free(gpu.ctx, ctypes.c_void_p(h))


# ---- the selection over several rounds of the compaction and over a full key array ----------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "all", "full"])
def test_selection_over_rounds_and_a_full_key_array(gpu, tag):
    """uc.rounds_case: 2100 targets, the cut inside a tie class whose last kept member is (a) before, (b) the last id of the first
    round of 1024 ids, (c) the first of the second, (d) in the third, (all) no cut; uc.full_case: 4200 admitted targets, 4096 keys"""
    C = uc.full_case() if tag == "full" else uc.rounds_case()
    m = C["max_hits"][tag]
    gpu.load_targets(*uc.pack(C["targets"]), 21)
    hits, counts = gpu.scan_batch(C["mat"], C["queries"], min_score=C["rule"]["min_score"], max_hits=m)
    assert_lists(lists_of(hits, counts), uc.case_lists(C, uc.select_list, m), tag)
