"""GPU tests of the exhaustive gapped scan (mmgpu_gscan_*): the device's lists against the lists recorded from the stock binary
(tests/golden/gapped_scan.npz), its raw scores against the restatement over the plain-C oracle (tests/gapped_scan_cases.py) at the
alignment kernels' tile and job boundaries, chunked runs against the unchunked one, the selection over 16-bit scores with both
thresholds, the identity rule, profile queries, the batch lifecycle, the hand-over into the alignment batch and the refusals.
Small shapes only."""
import ctypes
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import gapped_scan_cases as gc
from tests import ungapped_scan_cases as uc
from tests.ungapped_scan_cases import assert_lists, lists_of
from tests import ungapped_scan_profile_cases as upc

pytestmark = pytest.mark.gpu

X = 20
GO, GE = 11, 1


@functools.lru_cache(maxsize=None)
def golden():
    return gc.Golden()


@functools.lru_cache(maxsize=None)
def blosum62():
    return golden().g["mat_blosum62"]


@functools.lru_cache(maxsize=None)
def the_oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def expect_scores(queries, targets, go=GO, ge=GE):
    return np.stack([gc.raw_scores(the_oracle(), blosum62(), go, ge, qd, targets, qd.get("window") or gc.FULL_WINDOW) for qd in queries])


def device_scores(gpu, queries, targets, **kw):
    gpu.load_targets(*uc.pack(targets), 21)
    b = gpu.gscan_prepare(blosum62(), GO, GE, queries, **kw)
    b.run()
    out = np.stack([b.debug_scores(k) for k in range(len(queries))])
    b.free()
    return out


def assert_scores(gpu, queries, targets, **kw):
    got, want = device_scores(gpu, queries, targets, **kw), expect_scores(queries, targets)
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
    qs = [dict(qd, window=capi.coverage_window(s["cov"], s["cov_mode"], len(qd["q"]), tl)) for qd in G.setting_queries(k)]
    hits, counts = gpu.gscan_batch(G.mat(s), s["gap_open"], s["gap_extend"], qs, min_score=s["min_score"], max_hits=min(s["max_seqs"], 4096))
    assert hits.shape[1] == min(s["max_seqs"], len(tl)) and not hits["diagonal"].any()
    assert_lists(lists_of(hits, counts), G.expected(k), s["name"])


# ---- 2. tile boundaries, target shapes -----------------------------------------------------------------------------------------
def test_scores_at_the_tile_boundaries_and_target_shapes(gpu):
    rng = np.random.default_rng(21)
    qs = [dict(q=uc.random_seq(rng, n), comp_bias=rng.integers(-2, 3, n).astype(np.int8)) for n in gc.QUERY_LENGTHS]
    ts = [uc.random_seq(rng, n) for n in (1, 2, 3, 4, 5)] + [qs[3]["q"][:n].copy() for n in (1, 2, 3, 5)]
    ts.append(np.full(37, X, np.uint8))
    for qd in qs:      # homologs with a gap, moved over the columns by a random prefix
        q = qd["q"]
        h = uc.mutate(rng, q, 0.7)
        cut = len(q) // 2
        ts.append(np.concatenate([uc.random_seq(rng, int(rng.integers(0, 70))), h[:cut], uc.random_seq(rng, 3), h[cut:]]))
    long_t = uc.random_seq(rng, 40003)
    long_t[39900:39900 + 100] = qs[2]["q"][20:120]        # matches near the end ...
    long_t[20000:20000 + 300] = qs[8]["q"][200:500]       # ... over the strips of a one-tile query ...
    long_t[31:31 + 200] = qs[9]["q"][825:1025]            # ... and over the tile boundary of the multi-tile query
    ts.append(long_t)
    want = assert_scores(gpu, qs, ts)
    assert want[:, 9].max() < 30                                     # the target of X: -1 a cell before the composition bias
    assert want[2, -1] > 255 and want[8, -1] > 255 and want[9, -1] > 255 and (want[:, 10:] > 60).sum() >= len(qs)


def test_a_pair_that_saturates(gpu):
    rng = np.random.default_rng(22)
    q = uc.random_seq(rng, 6000)
    qs = [dict(q=q), dict(q=uc.random_seq(rng, 300))]
    ts = [q.copy(), uc.random_seq(rng, 50), q[:3000].copy()]
    want = assert_scores(gpu, qs, ts)
    assert want[0, 0] == 32767 and 255 < want[0, 2] < 32767
    gpu.load_targets(*uc.pack(ts), 21)
    (ids, sc), _ = lists_of(*gpu.gscan_batch(blosum62(), GO, GE, qs, min_score=100, max_hits=10))
    assert ids.tolist() == [0, 2] and sc[0] == 32767


# ---- 3. job boundaries -------------------------------------------------------------------------------------------------------
JOBS = gc.sw_job_constants()


@pytest.mark.parametrize("n", sorted({1, 7, JOBS["JOB_ROUND"] // 4 - 1, JOBS["JOB_ROUND"] // 4 + 1, JOBS["JOB_ROUND"] - 1, JOBS["JOB_ROUND"] + 1,
                                      JOBS["JOB_HITS"] - 1, JOBS["JOB_HITS"] + 1}))
def test_target_counts_around_a_round_and_a_job(gpu, n):
    """one target; odd counts; one below and above a workgroup round (and a wave's share of it, the round of a long query) and a job"""
    rng = np.random.default_rng(200 + n)
    qs = [dict(q=uc.random_seq(rng, 100), comp_bias=rng.integers(-1, 2, 100).astype(np.int8)), dict(q=uc.random_seq(rng, JOBS["LONG_QUERY"] + 1))]
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(1, 90, n)]
    ts[n // 2] = np.concatenate([uc.random_seq(rng, 13), qs[1]["q"][505:530], qs[0]["q"][10:30]])
    assert_scores(gpu, qs, ts)


# ---- 4. chunking -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_case():
    rng = np.random.default_rng(23)
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(5, 120, 60)]
    qs = [dict(q=uc.random_seq(rng, n)) for n in (40, 90, 200, 600, 33)]
    qs[1]["window"] = (30, 90)
    for k, qd in enumerate(qs):
        ts[7 * k + 3] = uc.mutate(rng, qd["q"], 0.75)[:110]
    return qs, ts


def run_everything(gpu, qs, budget):
    b = gpu.gscan_prepare(blosum62(), GO, GE, qs, min_score=15, max_hits=25, pair_budget=budget)
    b.run()
    hits, counts = b.fetch()
    scores = np.stack([b.debug_scores(k) for k in range(len(qs))])
    chunks = b.stage_ms()[1]
    b.free()
    return hits.tobytes(), counts.tobytes(), scores.tobytes(), chunks


def test_chunked_runs_equal_the_unchunked_run(gpu):
    qs, ts = chunk_case()
    gpu.load_targets(*uc.pack(ts), 21)
    tl = np.array([len(t) for t in ts])
    pairs = [int(np.sum((tl >= (qd.get("window") or gc.FULL_WINDOW)[0]) & (tl <= (qd.get("window") or gc.FULL_WINDOW)[1]))) for qd in qs]
    assert pairs[0] == 60 and 0 < pairs[1] < 60
    whole = run_everything(gpu, qs, 0)
    assert whole[3] == 1
    # the boundary between two queries; a query whose window alone is larger than the budget; the budget equal to the batch
    for budget, chunks in ((pairs[0] + pairs[1], 4), (59, 5), (sum(pairs), 1), (sum(pairs) - 1, 2)):
        got = run_everything(gpu, qs, budget)
        assert got[3] == chunks, (budget, got[3])
        assert got[:3] == whole[:3], budget


# ---- 5. selection ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def selection_case():
    """150 random targets and 77 copies of one: query 0 holds the copy whole (the copies tie above 255), query 1 a part of it (they
    tie below), query 2 is unrelated"""
    rng = np.random.default_rng(24)
    t = uc.random_seq(rng, 90)
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(5, 120, 150)] + [t.copy() for _ in range(77)]
    qs = [dict(q=np.concatenate([uc.random_seq(rng, 9), t, uc.random_seq(rng, 20)])), dict(q=np.concatenate([uc.random_seq(rng, 9), t[3:30]])),
          dict(q=uc.random_seq(rng, 200))]
    ts[7] = uc.mutate(rng, qs[2]["q"], 0.7)
    return qs, ts, expect_scores(qs, ts)


def run_lists(gpu, qs, ts, min_score, max_hits):
    gpu.load_targets(*uc.pack(ts), 21)
    return lists_of(*gpu.gscan_batch(blosum62(), GO, GE, qs, min_score=min_score, max_hits=max_hits))


def want_lists(qs, ts, sc, min_score, max_hits):
    tl = [len(t) for t in ts]
    return [gc.select_list(sc[k], tl, qd.get("window") or gc.FULL_WINDOW, min_score, qd.get("min_evalue_score") or 0, max_hits, qd.get("identity_id"))
            for k, qd in enumerate(qs)]


@pytest.mark.parametrize("max_hits", [1, 20, 77, 100, 400])
def test_ties_and_the_cut_inside_a_class(gpu, max_hits):
    qs, ts, sc = selection_case()
    assert sc[0, 150] > 255 and 15 < sc[1, 150] < 255 and len(set(sc[0, 150:].tolist())) == 1
    got = run_lists(gpu, qs, ts, 15, max_hits)
    assert_lists(got, want_lists(qs, ts, sc, 15, max_hits), max_hits)
    for ids, _ in got[:2]:      # the copies lead both lists, in id order
        assert np.array_equal(ids[:min(max_hits, 77)], 150 + np.arange(min(max_hits, 77)))
    if max_hits == 400:
        assert all(len(ids) < 227 for ids, _ in got)


def test_either_threshold_binds_and_an_empty_window(gpu):
    qs, ts, sc = selection_case()
    mid = int(np.median(sc[2][sc[2] > 15]))
    batch = [dict(qs[2], min_evalue_score=mid), dict(qs[2], min_evalue_score=3), dict(qs[2], min_evalue_score=gc.NEVER),
             dict(qs[0], window=(0xFFFFFFFF, 0xFFFFFFFF)), dict(qs[1], window=(90, 90), min_evalue_score=sc[1, 150] + 1)]
    got = run_lists(gpu, batch, ts, 15, 400)
    raw = np.stack([sc[2], sc[2], sc[2], np.zeros_like(sc[0]), np.where(np.array([len(t) for t in ts]) == 90, sc[1], 0)])
    assert_lists(got, want_lists(batch, ts, raw, 15, 400))
    assert 0 < len(got[0][0]) < len(got[1][0]) and got[0][1].min() >= mid and got[1][1].min() == 16
    assert not len(got[2][0]) and not len(got[3][0]) and not len(got[4][0])


# ---- 6. identity -------------------------------------------------------------------------------------------------------------
def test_identity_rule(gpu):
    rng = np.random.default_rng(25)
    mat = blosum62()
    A = 0
    assert mat[A, A] == 4
    short = uc.random_seq(rng, 12)
    sour = np.concatenate([np.full(40, A, np.uint8), uc.random_seq(rng, 10)])
    cb = np.concatenate([np.full(40, -7, np.int8), np.zeros(10, np.int8)])      # forty diagonal terms of 4 - 7: the sum is negative
    e, cons = upc.make_entry(rng, mat, 64)
    prof = upc.alignment_profile(e)
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(20, 100, 30)] + [short.copy(), sour.copy(), cons.copy(), uc.mutate(rng, cons, 0.8)]
    ts[3] = np.concatenate([uc.random_seq(rng, 8), sour[40:], uc.random_seq(rng, 8)])      # what the sour query does find
    n = len(ts)
    qs = [dict(q=short, identity_id=n - 4, min_evalue_score=5000), dict(q=sour, comp_bias=cb, identity_id=n - 3),
          dict(q=short, identity_id=n - 4, window=(13, 0xFFFFFFFF)), dict(q=cons, profile=prof, identity_id=n - 2)]
    gpu.load_targets(*uc.pack(ts), 21)
    b = gpu.gscan_prepare(mat, GO, GE, qs, min_score=5, max_hits=400)
    b.run()
    got = lists_of(*b.fetch())
    dev = np.stack([b.debug_scores(k) for k in range(len(qs))])
    b.free()
    sc = expect_scores(qs, ts)
    assert np.array_equal(dev, sc)
    assert_lists(got, want_lists(qs, ts, sc, 5, 400))
    own = int(sum(mat[x, x] for x in short))
    assert got[0][0].tolist() == [n - 4] and got[0][1].tolist() == [own] and own < 5000      # below min_evalue_score, listed all the same
    sour_sum = -120 + int(sum(mat[x, x] for x in sour[40:]))
    assert sour_sum < 0 and 3 in got[1][0].tolist() and got[1][0][-1] == n - 3 and got[1][1][-1] == sour_sum      # negative: last
    assert n - 4 not in got[2][0].tolist() and dev[2, n - 4] == 0                              # outside the window
    rows = np.array([int(prof[x, i]) for i, x in enumerate(cons)])
    assert got[3][0][0] == n - 2 and got[3][1][0] == rows.sum() and dev[3, n - 1] != dev[3, n - 2]


# ---- 7. profile queries ------------------------------------------------------------------------------------------------------
def test_profile_queries_score_as_the_oracle_aligns_them(gpu):
    rng = np.random.default_rng(26)
    mat = blosum62()
    qs = []
    for make, L in ((upc.make_entry, 100), (lambda r, m, n: upc.make_entry(r, m, n, sharp=1.5), 257), (upc.entry_with_lowest_minus_1, 40),
                    (upc.make_entry, 513)):
        e, cons = make(rng, mat, L)
        qs.append(dict(q=cons, profile=upc.alignment_profile(e)))
    assert len({int(qd["profile"].min()) for qd in qs}) >= 3      # profiles of different lowest scores, all inside the acceptance rule
    qs.append(dict(q=uc.random_seq(rng, 77), comp_bias=rng.integers(-1, 2, 77).astype(np.int8)))      # a sequence query in the same batch
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(1, 150, 24)] + [np.full(30, X, np.uint8)]
    ts += [np.concatenate([uc.random_seq(rng, 11), uc.mutate(rng, qd["q"], 0.8)]) for qd in qs]
    want = assert_scores(gpu, qs, ts)
    assert all(want[k, 25 + k] > 60 for k in range(len(qs)))
    # a profile whose lowest score is -32 is outside the acceptance rule at 11/1, like a matrix would be: refused, not mis-scored
    e, cons = upc.entry_with_one_minus_128(rng, mat, 60)
    assert raw_prepare(gpu, mat, [qs[0], dict(q=cons, profile=upc.alignment_profile(e))]) == (-4, None)


# ---- 8. lifecycle and hand-over ----------------------------------------------------------------------------------------------
def test_run_twice_and_prepare_again(gpu):
    qs, ts = chunk_case()
    gpu.load_targets(*uc.pack(ts), 21)
    b = gpu.gscan_prepare(blosum62(), GO, GE, qs, min_score=15, max_hits=50)
    b.run()
    h1, c1, s1 = *b.fetch(), b.debug_scores(1)
    b.run()
    h2, c2, s2 = *b.fetch(), b.debug_scores(1)
    assert h1.tobytes() == h2.tobytes() and c1.tobytes() == c2.tobytes() and s1.tobytes() == s2.tobytes()
    assert b.kernel_ms() > 0
    other = gpu.gscan_prepare(blosum62(), GO, GE, qs[:1], min_score=15, max_hits=50)
    other.run()
    with pytest.raises(capi.MMGpuError):      # the context's scratch now holds the other batch's scores
        b.debug_scores(0)
    other.free()
    b.free()
    b = gpu.gscan_prepare(blosum62(), GO, GE, qs, min_score=15, max_hits=50)
    b.run()
    h3, c3 = b.fetch()
    b.free()
    assert h1.tobytes() == h3.tobytes() and c1.tobytes() == c3.tobytes()


def test_lists_go_into_the_alignment_batch_on_the_device(gpu):
    G = golden()
    k = [s["name"] for s in G.settings].index("same_db")
    s = G.settings[k]
    gpu.load_targets(*uc.pack(G.setting_targets(s)), 21)
    qs = [dict(qd, min_evalue_score=0, min_start_score=0) for qd in G.setting_queries(k)[2:10]]
    hits, counts, rec = capi.exhaustive_gapped_search(gpu, G.mat(s), 11, 1, qs, min_score=20, max_hits=12, mode=1)
    host = gpu.sw_batch(G.mat(s), 11, 1, [dict(qd, targets=hits[i]["id"][:int(counts[i])]) for i, qd in enumerate(qs)], mode=1)
    at = 0
    for i, qd in enumerate(qs):
        n = int(counts[i])
        assert n > 1 and rec[i, :n].tobytes() == host[at:at + n].tobytes(), i
        other = hits[i]["id"][:n] != qd["identity_id"]
        assert other.sum() == n - 1 and np.array_equal(rec[i, :n]["score"][other], hits[i]["score"][:n][other])
        at += n


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def raw_prepare(g, mat, queries, go=GO, ge=GE, max_hits=300):
    par, arr, keep = g._gscan_marshal(mat, go, ge, queries, 15, max_hits, 0)
    h = ctypes.c_void_p(1)
    rc = g.L.mmgpu_gscan_prepare(g.ctx, ctypes.byref(par), ctypes.cast(arr, ctypes.c_void_p), len(queries), ctypes.byref(h))
    return rc, h.value


def test_refusals_leave_the_handle_null(gpu):
    import mmseqs2_amd
    rng = np.random.default_rng(27)
    q = dict(q=uc.random_seq(rng, 30))
    fresh = mmseqs2_amd.MMGpu(0)
    try:
        assert raw_prepare(fresh, blosum62(), [q]) == (-3, None)                          # MMGPU_ERR_STATE: no targets loaded
    finally:
        fresh.close()
    ts = [uc.random_seq(rng, 20) for _ in range(5)] + [uc.random_seq(rng, 30)]
    gpu.load_targets(*uc.pack(ts), 21)
    assert raw_prepare(gpu, blosum62(), [q], max_hits=4097) == (-4, None)                 # MMGPU_ERR_UNSUPPORTED
    assert raw_prepare(gpu, blosum62(), [q], go=5, ge=5) == (-4, None)                    # gap_open <= gap_extend
    vtml40 = uc.Golden().g["mat_vtml40"]
    assert int(vtml40.min()) + GE <= -GO
    assert raw_prepare(gpu, vtml40, [q]) == (-4, None)                                    # VTML40 at 11/1: outside the acceptance rule
    bad = dict(q=np.array([1, 2, 21, 3], np.uint8))
    assert raw_prepare(gpu, blosum62(), [q, bad]) == (-1, None)                           # MMGPU_ERR_ARG: a letter outside the alphabet
    assert raw_prepare(gpu, blosum62(), [dict(q, identity_id=0)]) == (-1, None)           # the identity target is not of the query's length
    assert raw_prepare(gpu, blosum62(), [dict(q, identity_id=6)]) == (-1, None)           # ... nor a target at all
    par, arr, keep = gpu._gscan_marshal(blosum62(), GO, GE, [q], 15, 300, 0)
    h = ctypes.c_void_p(1)
    assert gpu.L.mmgpu_gscan_prepare(gpu.ctx, None, ctypes.cast(arr, ctypes.c_void_p), 1, ctypes.byref(h)) == -1 and h.value is None
    h = ctypes.c_void_p(1)
    assert gpu.L.mmgpu_gscan_prepare(gpu.ctx, ctypes.byref(par), None, 1, ctypes.byref(h)) == -1 and h.value is None
    gpu.pf_set_shard(2, 0, 12, np.arange(6, dtype=np.uint32), np.zeros(12, np.uint32), np.arange(12, dtype=np.uint32) % 6)
    try:
        assert raw_prepare(gpu, blosum62(), [q]) == (-4, None)                            # a sharded context
    finally:
        gpu.pf_clear_shard()
    rc, h = raw_prepare(gpu, blosum62(), [dict(q, identity_id=5)])
    assert rc == 0 and h
    gpu.L.mmgpu_gscan_free(gpu.ctx, ctypes.c_void_p(h))


# ---- the selection over several rounds of the compaction and over a full key array ----------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "all", "full"])
def test_selection_over_rounds_and_a_full_key_array(gpu, tag):
    """gc.rounds_case: 2100 targets, the cut inside a tie class whose last kept member is (a) before, (b) the last id of the first
    round of 1024 ids, (c) the first of the second, (d) in the third, (all) no cut; gc.full_case: 4200 admitted targets, 4096 keys"""
    C = gc.full_case(the_oracle()) if tag == "full" else gc.rounds_case(the_oracle())
    m = C["max_hits"][tag]
    gpu.load_targets(*uc.pack(C["targets"]), 21)
    qs = [dict(qd, min_evalue_score=C["rule"]["min_ev"]) for qd in C["queries"]]
    hits, counts = gpu.gscan_batch(C["mat"], gc.CASE_GO, gc.CASE_GE, qs, min_score=C["rule"]["min_score"], max_hits=m)
    assert_lists(lists_of(hits, counts), uc.case_lists(C, gc.select_list, m), tag)
