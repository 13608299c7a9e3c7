"""GPU tests of profile queries in the exhaustive ungapped scan (`mmgpu_scan_query::profile`): the device's lists against the lists
recorded from the stock binary with profile query databases (tests/golden/ungapped_scan_profile.npz), its raw scores against the
numpy restatement (tests/ungapped_scan_profile_cases.py) at the kernel's boundaries, batches that mix the two kinds of query, the
letters a profile has no row for, the bias, the hand-over into the alignment batch and the refusals.  Small shapes only."""
import ctypes
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import ungapped_scan_cases as uc
from tests.ungapped_scan_cases import assert_lists, lists_of
from tests import ungapped_scan_profile_cases as upc

pytestmark = pytest.mark.gpu

X = 20


@functools.lru_cache(maxsize=None)
def golden():
    return upc.Golden()


@functools.lru_cache(maxsize=None)
def blosum62():
    return uc.Golden().g["mat_blosum62"]


def device_scores(gpu, mat, queries, targets, alphabet=21):
    """load, scan with the full window, -> uint8 [queries][targets] of debug_scores"""
    gpu.load_targets(*uc.pack(targets), alphabet)
    b = gpu.scan_prepare(mat, queries)
    b.run()
    out = np.stack([b.debug_scores(k) for k in range(len(queries))])
    b.free()
    return out


def expect_row(mat, qd, targets, alphabet=21):
    """a query's own restatement: the profile's where it has one, else the sequence queries'"""
    if qd.get("profile") is not None:
        return upc.scores_one_query(qd["profile"], targets, alphabet)
    return uc.scores_one_query(mat, qd["q"], qd.get("comp_bias"), targets)


def assert_scores(gpu, mat, queries, targets, alphabet=21):
    got = device_scores(gpu, mat, queries, targets, alphabet)
    want = np.stack([expect_row(mat, qd, targets, alphabet) for qd in queries])
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(q), int(t), int(got[q, t]), int(want[q, t]), len(targets[t])) for q, t in bad[:8]]
    return want


# ---- 1. the recorded lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(golden().settings)), ids=["%s_%s" % (s["group"], s["name"]) for s in golden().settings])
def test_device_lists_equal_the_recorded_lists(gpu, k):
    G = golden()
    s = G.settings[k]
    gpu.load_targets(*uc.pack(G.targets(s["group"])), 21)
    tl = G.tlens(s["group"])
    qs = [dict(profile=p, window=capi.coverage_window(s["cov"], s["cov_mode"], p.shape[1], tl)) for p in G.profiles(s["group"])]
    hits, counts = gpu.scan_batch(blosum62(), qs, min_score=s["min_score"], max_hits=s["max_seqs"])
    assert hits.shape[1] == min(s["max_seqs"], len(tl)) and not hits["diagonal"].any()
    assert_lists(lists_of(hits, counts), G.expected(k), (s["group"], s["name"]))


# ---- 2. query-length boundaries ----------------------------------------------------------------------------------------------
def boundary_case(rng):
    """a profile query of every length of uc.QUERY_LENGTHS; per query, targets that hold 24 letters of its consensus around the
    rows where a strip, a tile or the query ends, behind prefixes that move the match over the chunks of columns (about 120 per
    match: below the cap, so a diagonal broken at a boundary shows); one target of about 4 000 residues with matches across the first
    tile boundary of the two longest queries, so that the boundary line re-enters a tile built from a profile"""
    qs, ts, cons = [], [], {}
    for n in uc.QUERY_LENGTHS:
        e, c = upc.make_entry(rng, blosum62(), n, sharp=1.0)
        cons[n] = c
        qs.append(dict(profile=upc.alignment_profile(e)))
        rows = next((r for r in uc.TILE_ROWS if n <= r), 512) // 16      # rows per lane of the query's kernel
        for centre in sorted({rows, 2 * rows, 15 * rows, 512, 1024, n - 8, n // 2}):
            if 0 < centre < n + 8:
                seg = c[max(0, centre - 12):min(n, centre + 12)]
                ts.append(np.concatenate([uc.random_seq(rng, int(rng.integers(0, 70))), seg, uc.random_seq(rng, int(rng.integers(0, 40)))]))
    long_t = uc.random_seq(rng, 4003)
    long_t[2000:2024] = cons[2 * 512 + 1][500:524]
    long_t[3970:3994] = cons[3 * 512][502:526]
    ts.append(long_t)
    return qs, ts


def test_scores_at_the_query_length_boundaries(gpu):
    qs, ts = boundary_case(np.random.default_rng(41))
    assert len(ts) <= 125 and max(len(t) for t in ts[:-1]) <= 140
    want = assert_scores(gpu, blosum62(), qs, ts)
    assert (want > 60).sum() >= len(qs) and (want < 200).all()      # the planted matches are seen and none of them hides behind the cap
    by_len = {qd["profile"].shape[1]: k for k, qd in enumerate(qs)}
    assert want[by_len[2 * 512 + 1], -1] > 60 and want[by_len[3 * 512], -1] > 60


# ---- 3. sequence and profile queries in one batch ----------------------------------------------------------------------------
def test_sequence_and_profile_queries_share_a_batch(gpu):
    """alternating kinds with equal lengths inside each class: a workgroup that kept the previous job's source would show"""
    rng = np.random.default_rng(42)
    qs, ts = [], []
    for n in (100, 100, 300, 300, 2 * 512 + 1, 2 * 512 + 1):
        if len(qs) % 2 == 0:
            q = uc.random_seq(rng, n)
            qs.append(dict(q=q, comp_bias=rng.integers(-2, 3, n).astype(np.int8)))
            src = q
        else:
            e, src = upc.make_entry(rng, blosum62(), n, sharp=0.8)
            qs.append(dict(profile=upc.alignment_profile(e)))
        for lo in (0, n // 2 - 12, n - 24):
            ts.append(np.concatenate([uc.random_seq(rng, int(rng.integers(0, 50))), src[lo:lo + 24], uc.random_seq(rng, int(rng.integers(0, 20)))]))
    ts += [uc.random_seq(rng, int(x)) for x in rng.integers(1, 100, 70)]      # 88 targets: three rounds, the last one partial
    want = assert_scores(gpu, blosum62(), qs, ts)
    for k in range(len(qs)):      # every query sees its own three matches, and nobody else's as well
        own = want[k, 3 * k:3 * k + 3]
        assert (own > 60).all() and (np.delete(want[k], range(3 * k, 3 * k + 3)) < own.min()).all(), k
    # the same queries in the other order give the same rows
    swapped = [qs[k ^ 1] for k in range(len(qs))]
    got = device_scores(gpu, blosum62(), swapped, ts)
    assert np.array_equal(got, want[[k ^ 1 for k in range(len(qs))]])


# ---- 4. letters without a row ------------------------------------------------------------------------------------------------
def test_letters_a_profile_has_no_row_for(gpu):
    rng = np.random.default_rng(43)
    e, cons = upc.make_entry(rng, blosum62(), 90, sharp=1.0)
    p20 = upc.alignment_profile(e)
    p21 = np.vstack([p20, np.full((1, 90), 2, np.int8)])
    ts = [np.full(37, X, np.uint8), np.full(1, X, np.uint8), np.full(200, X, np.uint8), cons[10:30].copy(),
          np.concatenate([cons[:12], np.full(5, X, np.uint8), cons[17:30]])]
    want = assert_scores(gpu, blosum62(), [dict(profile=p20), dict(profile=p21)], ts)
    assert not want[0, :3].any()                                # a 20-letter profile against the 21-letter database: X scores 0
    assert want[1, :3].tolist() == [2 * 37, 2, 2 * 90]          # 21 rows: row 20 is scored
    assert want[1, 4] == want[0, 4] + 2 * 5 and 60 < want[0, 3] < 200 and want[0, 4] > want[0, 3]
    # a profile of fewer rows than letters occur: the letters from profile_letters on score 0
    p7 = np.ascontiguousarray(p20[:7])
    assert_scores(gpu, blosum62(), [dict(profile=p7)], ts + [uc.random_seq(rng, 80)])


# ---- 5. the bias comes from the profile alone --------------------------------------------------------------------------------
def test_bias_from_the_profile_only(gpu):
    rng = np.random.default_rng(44)
    mat = blosum62().copy()
    mat[3, 5] = mat[5, 3] = -10
    assert mat.min() == -10
    e1, c1 = upc.entry_with_lowest_minus_1(rng, mat, 120)
    e32, c32 = upc.entry_with_one_minus_128(rng, mat, 120)
    e0, c0 = upc.make_entry(rng, mat, 120, sharp=1.0)
    e0[:, :20] = np.abs(e0[:, :20])
    profs = [upc.alignment_profile(e) for e in (e1, e32, e0)]
    assert [upc.bias_of(p) for p in profs] == [1, 32, 0]
    ts = [np.concatenate([c, c]) for c in (c1, c32, c0)] + [uc.random_seq(rng, 60)]
    want = assert_scores(gpu, mat, [dict(profile=p) for p in profs], ts)
    assert (want[0, 0], want[1, 1], want[2, 2]) == (254, 223, 255)      # (a sequence query with this matrix would stop at 245)


# ---- 6. comp_bias is ignored -------------------------------------------------------------------------------------------------
def test_comp_bias_is_ignored_for_a_profile_query(gpu):
    G = golden()
    ts = G.targets("B")[:100]
    profs = G.profiles("B")[4:12]
    gpu.load_targets(*uc.pack(ts), 21)
    out = []
    for with_bias in (False, True):
        qs = [dict(profile=p, comp_bias=np.full(p.shape[1], -20, np.int8) if with_bias else None) for p in profs]
        b = gpu.scan_prepare(blosum62(), qs, min_score=15, max_hits=50)
        b.run()
        hits, counts = b.fetch()
        out.append((hits.tobytes(), counts.tobytes(), b"".join(b.debug_scores(k).tobytes() for k in range(len(qs)))))
        b.free()
    assert out[0] == out[1] and any(out[0][2])


# ---- 7. hand-over ------------------------------------------------------------------------------------------------------------
def test_profile_lists_go_into_the_alignment_batch_on_the_device(gpu, matrices):
    G = golden()
    k = next(i for i, s in enumerate(G.settings) if (s["group"], s["name"]) == ("A", "base"))
    gpu.load_targets(*uc.pack(G.targets("A")), 21)
    qs = [dict(q=np.ascontiguousarray(e[:, 20]).view(np.uint8), profile=upc.alignment_profile(e), min_start_score=0) for e in G.entries("A")[:6]]
    sw_mat = matrices["blosum62_sw"]
    hits, counts, rec = capi.exhaustive_search(gpu, blosum62(), sw_mat, 11, 1, qs, min_score=15, max_hits=40, mode=1)
    assert_lists(lists_of(hits, counts), [(i[:40], sc[:40]) for i, sc in G.expected(k)[:6]])
    host = gpu.sw_batch(sw_mat, 11, 1, [dict(qd, targets=hits[j]["id"][:int(counts[j])]) for j, qd in enumerate(qs)], mode=1)
    at = 0
    for j in range(len(qs)):
        n = int(counts[j])
        assert n > 0 and rec[j, :n].tobytes() == host[at:at + n].tobytes(), j
        at += n


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def raw_prepare(g, mat, queries, letters=None):
    par, arr, keep = g._scan_marshal(mat, queries, 15, 300)
    if letters is not None:
        arr[len(queries) - 1].profile_letters = letters
    h = ctypes.c_void_p(1)
    rc = g.L.mmgpu_scan_prepare(g.ctx, ctypes.byref(par), ctypes.cast(arr, ctypes.c_void_p), len(queries), ctypes.byref(h))
    return rc, h.value


def test_refusals_leave_the_handle_null(gpu):
    rng = np.random.default_rng(46)
    e, _ = upc.make_entry(rng, blosum62(), 30)
    good = dict(profile=upc.alignment_profile(e))
    gpu.load_targets(*uc.pack([uc.random_seq(rng, 20) for _ in range(5)]), 21)
    assert raw_prepare(gpu, blosum62(), [good, good], letters=0) == (-1, None)       # MMGPU_ERR_ARG: a profile of no rows
    assert raw_prepare(gpu, blosum62(), [good, good], letters=22) == (-1, None)      # ... of more rows than the alphabet has letters
    with21 = dict(profile=np.vstack([good["profile"], np.zeros((1, 30), np.int8)]))
    for qd in (good, with21):
        assert "q" not in qd
        rc, h = raw_prepare(gpu, blosum62(), [qd])                                   # q = NULL: prepares and frees
        assert rc == 0 and h
        gpu.L.mmgpu_scan_free(gpu.ctx, ctypes.c_void_p(h))
