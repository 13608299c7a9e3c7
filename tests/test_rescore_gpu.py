"""GPU tests of the ungapped diagonal rescoring (mmgpu_rescore_*): the device's lists against the lists recorded from the stock binary
(tests/golden/rescore.npz), its records against the serial restatement (tests/rescore_cases.py) at the boundaries of the kernel's split
of a diagonal over lanes, at the extreme and the invalid diagonals, on the tie cases, with two valid candidates, the batch shapes,
the lifecycle and the refusals.  Integers are compared exactly; seqId and E-value as tests/rescore_cases.assert_lines states.
Small shapes only, apart from the diagonals that must be long."""
import ctypes
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import gapped_scan_cases as gc
from tests import rescore_cases as rc
from tests import ungapped_scan_cases as uc

pytestmark = pytest.mark.gpu

X = 20
MODES = (rc.HAMMING, rc.SUBSTITUTION, rc.ALIGNMENT)


@functools.lru_cache(maxsize=None)
def golden():
    return rc.Golden()


@functools.lru_cache(maxsize=None)
def matrices():
    return dict(blosum62=golden().mat, blosum80=gc.Golden().g["mat_blosum80"], vtml40=uc.Golden().g["mat_vtml40"])


def assert_records(gpu, mat, queries, targets, hits, modes=MODES, loaded=False):
    """device records == restatement, field by field, for every mode -> the restatement's records per mode"""
    if not loaded:
        gpu.load_targets(*uc.pack(targets), 21)
    out = {}
    for mode in modes:
        got = gpu.rescore_batch(mat, queries, hits, mode)
        want = rc.rescore_records(mat, queries, targets, hits, mode)
        assert got.dtype == want.dtype and len(got) == len(want)
        bad = np.flatnonzero(got != want)
        flat = [(qi, int(t), int(d)) for qi, hs in enumerate(hits) for t, d in np.asarray(hs, np.int64).reshape(-1, 2)]
        assert len(bad) == 0, (mode, [(flat[k], got[k].tolist(), want[k].tolist()) for k in bad[:6]])
        out[mode] = want
    return out


# ---- 1. the recorded lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_device_lists_equal_the_recorded_lists(gpu, k):
    G = golden()
    s = G.settings[k]
    gpu.load_targets(*uc.pack(G.setting_targets(s)), 21)
    got = capi.rescore_diagonal(gpu, G.mat, G.queries, G.hits(s), s["mode"], identity=G.identity(s), **G.options(s))
    rc.assert_lines(got, G.expected(k), s["effective_mode"], s["name"])


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


@pytest.mark.parametrize("name", ["blosum62", "blosum80", "vtml40"])
def test_diagonal_lengths_and_both_alignments(gpu, name):
    """a diagonal of n cells three ways: from query position 5 (the query side unaligned), from target position 3 (the target side
    unaligned), from 0 (n + 3 cells); 40003 cells once"""
    rng = np.random.default_rng(41)
    mat = matrices()[name]
    qs, ts, hits = [], [], []
    for n in LENGTHS + [40003]:
        q = uc.random_seq(rng, n + 5, 21)
        t = np.concatenate([uc.random_seq(rng, 3), uc.mutate(rng, q[:n], 0.6)])      # homologous along D = -3
        t[3], t[3 + n - 1] = q[0], q[n - 1]                                          # (its first and last cell match)
        qs.append(q)
        ts.append(t)
        hits.append([(len(ts) - 1, d) for d in ((-3,) if n > 2000 else (5, -3, 0))])
    want = assert_records(gpu, mat, qs, ts, hits)
    lens = want[rc.HAMMING]["diag_len"][want[rc.HAMMING]["score"] > 0]
    assert set(LENGTHS + [40003]) <= set(lens.tolist())
    assert (want[rc.ALIGNMENT]["ident"] > 0).sum() >= len(LENGTHS) and want[rc.ALIGNMENT]["score"].max() > 40003


def test_extreme_and_invalid_diagonals_and_a_target_of_x(gpu):
    rng = np.random.default_rng(42)
    q = uc.random_seq(rng, 70)
    t = uc.mutate(rng, q, 0.8)[:50]
    t[49], t[0] = q[0], q[69]      # the one-cell diagonals match
    allx = np.full(37, X, np.uint8)
    ts = [t, allx, q[:1].copy()]
    ql, tl = 70, 50
    hits = [[(0, 0), (0, ql - 1), (0, ql), (0, 65536 - (tl - 1)), (0, 65536 - tl), (0, 30000), (0, 32768), (0, 65535), (0, 1),
             (1, 0), (1, 5), (1, 65536 - 36), (2, 0), (2, 69), (2, 1)]]
    for mat in matrices().values():
        want = assert_records(gpu, mat, [q], ts, hits)
        h = want[rc.HAMMING]
        assert h[1].tolist() == (1, ql - 1, 1, -1, -1, 1) and h[3].tolist() == (1, -(tl - 1), 1, -1, -1, 1)
        for k in (2, 4, 5, 6):      # one past each end, valid for neither sign: the default record
            assert all(want[m][k].tolist() == rc.DEFAULT_RECORD for m in MODES)
        for k in (9, 10, 11):       # X against letters: -1 a cell, nothing above 0
            assert all(want[m][k].tolist() == rc.DEFAULT_RECORD for m in MODES)
        assert want[rc.ALIGNMENT][0]["score"] > 100 and want[rc.ALIGNMENT][12].tolist()[1:] == (0, 1, 0, 0, 1)


def mismatching(rng, q, mat):
    """a target that scores below 0 against q in every cell"""
    t = np.zeros(len(q), np.uint8)
    for i, a in enumerate(q):
        t[i] = rng.choice(np.flatnonzero(np.asarray(mat)[int(a), :20] < 0))
    return t


@pytest.mark.parametrize("n", [64, 301, 1000])
def test_segments_planted_on_every_lane_boundary(gpu, n):
    """the best segment starts or ends one before, on and one after every cut between two lanes' runs"""
    rng = np.random.default_rng(43 + n)
    mat = golden().mat
    cuts = rc.lane_cuts(n)
    assert len(cuts) == rc.kernel_constants()["RESCORE_GROUP"] - 1 and cuts[0] % rc.kernel_constants()["RESCORE_STEP"] == 0
    q = uc.random_seq(rng, n)
    base = mismatching(rng, q, mat)
    ts, planted = [], []
    for c in cuts:
        for s, e in ((c, c + 6), (c - 1, c + 6), (c + 1, c + 6), (c - 7, c - 1), (c - 7, c), (c - 7, c + 1), (c - 1, c), (c, c)):
            s, e = max(s, 0), min(e, n - 1)
            if s > e:
                continue
            t = base.copy()
            t[s:e + 1] = q[s:e + 1]
            ts.append(t)
            planted.append((s, e))
    ts.append(q.copy())                     # the whole diagonal: over every cut
    planted.append((0, n - 1))
    hits = [[(k, 0) for k in range(len(ts))]]
    want = assert_records(gpu, mat, [q], ts, hits)
    a = want[rc.ALIGNMENT]
    assert [(int(r["start"]), int(r["end"])) for r in a] == planted      # (every other cell is negative)
    assert np.array_equal(a["ident"], [e - s + 1 for s, e in planted]) and np.array_equal(want[rc.HAMMING]["score"], a["ident"])


def letters_for(mat, cells):
    """(q, t) whose diagonal scores exactly `cells` under mat"""
    q, t = [], []
    for c in cells:
        a, b = np.argwhere(np.asarray(mat)[:20, :20] == c)[0]
        q.append(a)
        t.append(b)
    return np.array(q, np.uint8), np.array(t, np.uint8)


def test_tie_cases_at_every_offset_to_the_lane_cuts(gpu):
    mat = golden().mat
    have = set(np.unique(mat[:20, :20]).tolist())
    seg = [5, -2, 4, 6]
    drop = [-4, -4, -4, -4]
    cases = [[3], [-3], [0], [-1, -4, -2, -4], [0, 0, 0], [2, -2] + seg, [4, -1, -3] + seg, [-3, 1, -1, 2, -2] + seg + [-4, -4, 1],
             seg + drop + seg, seg + drop + seg + drop + seg, [7, -4, -3, 7, -4, -3, 7], [3, -1, 1, -1, 1], [1, 1, -2, 1, 1, -2, 1, 1]]
    assert all(c in have for cells in cases for c in cells)
    qs, ts, hits, cells_of = [], [], [], []
    for cells in cases:
        for shift in range(0, 9):           # the case moves over the cuts of its diagonal (a run is 4 cells up to 64 of them)
            full = [-2] * shift + cells + [-2] * (2 + shift % 3)
            q, t = letters_for(mat, full)
            qs.append(q)
            ts.append(t)
            hits.append([(len(ts) - 1, 0)])
            cells_of.append(full)
    want = assert_records(gpu, mat, qs, ts, hits)
    for k, full in enumerate(cells_of):      # the restatement is the reference's loop over these very cells
        score, start, end = rc.walk(full)
        r = want[rc.ALIGNMENT][k]
        assert (int(r["score"]), int(r["start"]), int(r["end"])) == ((score, start, end) if score > 0 else (0, -1, -1))
    k = 9 * 5      # [2, -2] + seg at shift 0: the start is behind the zero-sum stretch; two equal maxima: the first
    assert want[rc.ALIGNMENT][k].tolist()[:5] == (13, 0, 8, 2, 5) and want[rc.ALIGNMENT][9 * 8].tolist()[:5] == (13, 0, 14, 0, 3)


# ---- 3. two valid candidates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longer", ["positive", "negative", "equal"])
def test_both_signs_of_a_stored_diagonal_are_valid(gpu, longer):
    """qLen 40000, tLen 50000, d 30000: D = 30000 (10000 cells) and D = -35536 (14464 cells).  Letters of the two sequences come from
    sets that score below 0 against each other, so only the planted segments score; the same segment on both: the negative wins"""
    rng = np.random.default_rng(44)
    mat = golden().mat
    order = np.argsort(-np.diag(mat)[:20])
    qset = order[:3]
    tset = np.array([x for x in range(20) if (mat[qset, x] < 0).all()][:3])
    assert len(tset) == 3 and (mat[np.ix_(qset, tset)] < 0).all()
    q = qset[rng.integers(0, 3, 40000)].astype(np.uint8)
    t = tset[rng.integers(0, 3, 50000)].astype(np.uint8)
    n_pos, n_neg = dict(positive=(80, 60), negative=(60, 80), equal=(60, 60))[longer]
    P = qset[rng.integers(0, 3, 80)].astype(np.uint8)
    q[30000 + 100:30000 + 100 + n_pos] = P[:n_pos]
    t[100:100 + n_pos] = P[:n_pos]
    q[200:200 + n_neg] = P[:n_neg]
    t[35536 + 200:35536 + 200 + n_neg] = P[:n_neg]
    want = assert_records(gpu, mat, [q], [t], [[(0, 30000)]])
    a = want[rc.ALIGNMENT][0]
    if longer == "positive":
        assert a.tolist()[1:] == (30000, 10000, 100, 179, 80) and want[rc.HAMMING][0].tolist() == (80, 30000, 10000, -1, -1, 80)
    else:
        assert a.tolist()[1:] == (-35536, 14464, 200, 200 + n_neg - 1, n_neg) and want[rc.HAMMING][0]["diagonal"] == -35536
    assert want[rc.SUBSTITUTION][0]["score"] == a["score"] == sum(int(mat[x, x]) for x in P[:max(n_pos, n_neg)])


# ---- 4. batch shape ----------------------------------------------------------------------------------------------------------
def test_batch_shape_order_and_agreement_of_the_modes(gpu):
    rng = np.random.default_rng(45)
    mat = golden().mat
    ts = [uc.random_seq(rng, int(x)) for x in rng.integers(1, 60, 200)]
    qs = [uc.random_seq(rng, n) for n in (40, 33, 57, 9)]
    for k in range(0, 200, 7):
        ts[k] = uc.mutate(rng, qs[2], 0.7)[:int(rng.integers(20, 57))]
    many = np.stack([rng.integers(0, 200, 4097), rng.integers(-8, 9, 4097)], axis=1)
    many[:12] = [(14, d) for d in (0, 1, -1, 2, -2, 3, 0, 0, 56, -19, 57, 30000)]      # one target under several diagonals, twice the same
    hits = [np.zeros((0, 2), np.int64), [(5, 0)], many, np.zeros((0, 2), np.int64)]
    want = assert_records(gpu, mat, qs, ts, hits)
    h, s, a = want[rc.HAMMING], want[rc.SUBSTITUTION], want[rc.ALIGNMENT]
    assert len(a) == 4098 and np.array_equal(s["score"], a["score"])
    assert np.array_equal(s["diagonal"], a["diagonal"]) and np.array_equal(s["diag_len"], a["diag_len"])
    assert a[7].tolist() == a[8].tolist() == a[1].tolist() and a[1]["score"] > 30 and (a["score"] > 30).sum() > 10
    for k in range(1, 4098):      # mode 0 counts the matches of the whole diagonal
        t, d = many[k - 1]
        D = int(d)
        n = int(h[k]["diag_len"])
        qa, ta = (qs[2][D:D + n], ts[t][:n]) if D >= 0 else (qs[2][:n], ts[t][-D:-D + n])
        assert h[k]["score"] == int(np.sum(qa == ta)) == h[k]["ident"] or (h[k]["score"] == 0 and n == 0)
    # the same list as separate single-query batches: output order is input order
    again = gpu.rescore_batch(mat, [qs[2]], [many[::-1]], rc.ALIGNMENT)
    assert again[::-1].tobytes() == a[1:].tobytes()


# ---- 5. lifecycle ------------------------------------------------------------------------------------------------------------
def test_run_twice_and_prepare_again(gpu):
    G = golden()
    s = G.settings[0]
    gpu.load_targets(*uc.pack(G.targets), 21)
    b = gpu.rescore_prepare(G.mat, G.queries, G.hits(s), rc.ALIGNMENT)
    with pytest.raises(capi.MMGpuError):      # not run yet
        b.fetch()
    b.run()
    r1 = b.fetch()
    b.run()
    r2 = b.fetch()
    assert r1.tobytes() == r2.tobytes() and b.kernel_ms() > 0 and len(r1) == sum(len(h) for h in G.hits(s))
    import torch
    d = torch.zeros(len(r1) * capi.RESCORE_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.fetch_device(d.data_ptr())
    gpu.synchronize()
    assert d.cpu().numpy().tobytes() == r1.tobytes()
    b.free()
    b = gpu.rescore_prepare(G.mat, G.queries, G.hits(s), rc.ALIGNMENT)
    b.run()
    r3 = b.fetch()
    b.free()
    assert r1.tobytes() == r3.tobytes()
    b = gpu.rescore_prepare(G.mat, G.queries[:2], G.hits(s)[:2], rc.HAMMING)
    gpu.load_targets(*uc.pack(G.targets[:50]), 21)      # a reload invalidates a prepared batch
    with pytest.raises(capi.MMGpuError):
        b.run()
    b.free()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def raw_prepare(g, mat, queries, hits, mode, null=None):
    par, arr, off, pairs, keep = g._rescore_marshal(mat, queries, hits, mode)
    h = ctypes.c_void_p(1)
    args = dict(par=ctypes.byref(par), qs=ctypes.cast(arr, ctypes.c_void_p), off=capi._ptr(off), pairs=capi._ptr(pairs))
    if null:
        args[null] = None
    rc_ = g.L.mmgpu_rescore_prepare(g.ctx, args["par"], args["qs"], len(queries), args["off"], args["pairs"], ctypes.byref(h))
    return rc_, h.value


def test_refusals_leave_the_handle_null(gpu):
    import mmseqs2_amd
    rng = np.random.default_rng(46)
    mat = golden().mat
    q = uc.random_seq(rng, 30)
    hits = [[(0, 0), (4, 3)]]
    fresh = mmseqs2_amd.MMGpu(0)
    try:
        assert raw_prepare(fresh, mat, [q], hits, 0) == (-3, None)                       # MMGPU_ERR_STATE: no targets loaded
    finally:
        fresh.close()
    ts = [uc.random_seq(rng, 20) for _ in range(5)]
    gpu.load_targets(*uc.pack(ts), 21)
    assert raw_prepare(gpu, mat, [q], hits, 3) == (-4, None)                             # MMGPU_ERR_UNSUPPORTED: end-to-end
    assert raw_prepare(gpu, mat, [q], hits, 4) == (-4, None)                             # ... window quality
    assert raw_prepare(gpu, mat[:5, :5].copy(), [q % 5], hits, 0) == (-4, None)          # an alphabet other than 21
    assert raw_prepare(gpu, mat, [q], hits, 5) == (-1, None)                             # MMGPU_ERR_ARG: no such mode
    assert raw_prepare(gpu, mat, [q], [[(0, 0), (5, 3)]], 0) == (-1, None)               # a target id outside the database
    assert raw_prepare(gpu, mat, [np.array([1, 2, 21, 3], np.uint8)], hits, 0) == (-1, None)      # a query letter outside the alphabet
    for null in ("par", "qs", "off", "pairs"):
        assert raw_prepare(gpu, mat, [q], hits, 0, null=null) == (-1, None), null        # null pointers
    assert gpu.L.mmgpu_rescore_prepare(gpu.ctx, None, None, 0, None, None, None) == -1
    gpu.pf_set_shard(2, 0, 10, np.arange(5, dtype=np.uint32), np.zeros(10, np.uint32), np.arange(10, dtype=np.uint32) % 5)
    try:
        assert raw_prepare(gpu, mat, [q], hits, 0) == (-4, None)                         # a sharded context
    finally:
        gpu.pf_clear_shard()
    gpu.load_targets(np.zeros(40, np.uint8), np.array([0, 20, 40], np.uint64), 5)        # nucleotide targets
    assert raw_prepare(gpu, mat, [q], [[(0, 0)]], 0) == (-4, None)
    gpu.load_targets(*uc.pack(ts), 21)
    rc_, h = raw_prepare(gpu, mat, [q], hits, 0)
    assert rc_ == 0 and h
    gpu.L.mmgpu_rescore_free(gpu.ctx, ctypes.c_void_p(h))
