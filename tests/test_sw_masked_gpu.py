"""GPU tests of the masked alignment batch (mmgpu_sw_prepare_masked): the copies sw_mask_gather_kernel makes, and every call a batch
serves - forward and reverse scan, multi-tile, traceback, block aligner, block_starts, profile queries - on masked targets against
the restatement on host-masked targets; capi.alt_alignments against the chains recorded from the real reference."""
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from mmseqs2_amd import workloads as wl
from tests.test_sw_masked import load_alt_ali_vectors

pytestmark = pytest.mark.gpu

X = 20
REC = ("score", "q_end", "t_end", "q_start", "t_start", "word")


def host_masked(t, spans):
    m = np.array(t, np.uint8)
    for a, b in ([] if spans is None else spans):
        m[int(a):int(b)] = X
    return m


def rec_tuple(h):
    return tuple(int(h[f]) for f in REC)


def oracle_tuple(r):
    return tuple(r[f] for f in REC)


def comp_bias(oracle, matrices, q):
    return oracle.round_comp_bias(oracle.comp_bias(matrices["blosum62_sw"].astype(np.int16), matrices["blosum62_pback"], q, 1.0))


# ---- 1. bytes ------------------------------------------------------------------------------------------------------------
BYTE_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099, 65535]


def byte_masks(rng, n):
    """the span lists every target length gets, one pair each (bounds clipped to the length)"""
    c = lambda a, b: (min(a, n), min(b, n))      # noqa: E731
    mid = n // 2
    out = [None, [(mid, mid)], [(0, 1)], [(n - 1, n)], [(0, n)],
           [c(1, 3), c(3, 6)],                                    # adjacent
           [c(0, mid + 1), c(mid // 2, n)],                       # overlapping
           [c(n - 2, n), c(mid, mid + 1), c(0, 1)] if n >= 2 else [(0, 1), (0, 0)]]      # descending
    twelve = []
    for _ in range(12):
        a = int(rng.integers(0, n + 1))
        twelve.append((a, int(rng.integers(a, min(n, a + 40) + 1))))
    out.append(twelve)
    return out


def test_copies_are_the_masked_targets_byte_for_byte(gpu, matrices, oracle):
    rng = np.random.default_rng(101)
    mat = matrices["blosum62_sw"]
    ts = [rng.integers(0, 20, n).astype(np.uint8) for n in BYTE_LENS]
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    q = rng.integers(0, 20, 24).astype(np.uint8)
    cb = comp_bias(oracle, matrices, q)
    ids, masks = [], []
    for t_id, n in enumerate(BYTE_LENS):
        for m in byte_masks(rng, n):
            ids.append(t_id)
            masks.append(m)
    # ... and every (t_from % 4, t_to % 4) inside the 64-residue target, each span on a pair of its own
    for a in range(4):
        for b in range(4):
            ids.append(BYTE_LENS.index(64))
            masks.append([(8 + a, 20 + b)])
    assert len({(a % 4, b % 4) for m in masks[-16:] for a, b in m}) == 16
    # a list beyond one pass of the kernel (64 spans per pass)
    ids.append(BYTE_LENS.index(4099))
    masks.append([(int(a), int(a) + 5) for a in rng.integers(0, 4090, 150)])
    ids = np.array(ids, np.uint32)
    # the second query names the same targets with other masks: every pair carries its own
    ids2 = np.array([BYTE_LENS.index(257), BYTE_LENS.index(257), BYTE_LENS.index(5)], np.uint32)
    masks2 = [[(0, 100)], [(200, 257)], None]
    plain_q = [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0), dict(q=q[:7], comp_bias=cb[:7], targets=ids2, min_start_score=0)]
    before = gpu.sw_batch(mat, 11, 1, plain_q, mode=1)
    b = gpu.sw_prepare_masked(mat, 11, 1, [dict(plain_q[0], masks=masks), dict(plain_q[1], masks=masks2)], mode=1)
    all_ids, all_masks = np.concatenate([ids, ids2]), masks + masks2
    assert b.pairs == len(all_ids)
    for p, (t_id, m) in enumerate(zip(all_ids, all_masks)):
        got, n = b.debug_masked_target(p)
        want = host_masked(ts[int(t_id)], m)
        assert n == len(want) and len(got) == (n + 3) & ~3, p
        assert np.array_equal(got[:n], want), (p, int(t_id), m)
        assert (got[n:] == 21).all(), (p, "pad letters")
    b.run()
    got = b.fetch()
    b.free()
    # a sample of the pairs against the restatement (pair 108 is the 65 535-residue target, the last one the 150-span list), the rest of the alignment in tests 2 - 7
    for p in list(range(0, len(all_ids), 9)) + [len(ids) - 1]:
        qq, cc = (q, cb) if p < len(ids) else (q[:7], cb[:7])
        r = oracle.sw_align(qq, cc, host_masked(ts[int(all_ids[p])], all_masks[p]), mat, 11, 1, need_start=True)
        assert rec_tuple(got[p]) == oracle_tuple(r), p
    # the resident targets are as they were
    assert np.array_equal(gpu.sw_batch(mat, 11, 1, plain_q, mode=1), before)


# ---- 2 / 3. scores, ends, starts, tracebacks --------------------------------------------------------------------------------
QUERY_LENS = [1, 37, 130, 300, 530, 1100]


def repeats_target(rng, q, copies, lo=0.5, hi=0.9):
    parts = []
    for _ in range(copies):
        parts.append(rng.integers(0, 20, int(rng.integers(0, 30))).astype(np.uint8))
        parts.append(wl.mutate(rng, q, float(rng.uniform(lo, hi))) if len(q) > 12 else q.copy())
    parts.append(rng.integers(0, 20, int(rng.integers(0, 30))).astype(np.uint8))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def _masked_case():
    """queries of QUERY_LENS, 40 targets each (24 of mutated repeats of the query, 16 unrelated), spans = the restatement's first
    alignment + one random span; the restatement's alignment of every pair on the host-masked target, computed once"""
    from oracle.pyoracle import Oracle
    from tests.conftest import GOLDEN
    import os
    orc = Oracle()
    matrices = dict(np.load(os.path.join(GOLDEN, "matrices.npz")))
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(202)
    ts, queries, expect = [], [], []
    for qlen in QUERY_LENS:
        q = rng.integers(0, 20, qlen).astype(np.uint8)
        cb = comp_bias(orc, matrices, q)
        mine, masks = [], []
        for k in range(40):
            if k < 24:
                t = repeats_target(rng, q, 1 + k % (2 if qlen > 600 else 3))
            else:
                t = rng.integers(0, 20, int(rng.integers(30, 400))).astype(np.uint8)
            r = orc.sw_align(q, cb, t, mat, 11, 1, need_start=True)
            a = int(rng.integers(0, len(t) + 1))
            spans = [(a, int(rng.integers(a, min(len(t), a + 60) + 1)))]
            if r["score"] > 0:
                spans.insert(0, (r["t_start"], r["t_end"]))
            mine.append(len(ts))
            ts.append(t)
            masks.append(spans)
            expect.append(orc.sw_align(q, cb, host_masked(t, spans), mat, 11, 1, need_start=True, need_bt=True))
        queries.append(dict(q=q, comp_bias=cb, targets=np.array(mine, np.uint32), masks=masks, min_start_score=0))
    return mat, queries, ts, expect


def test_scores_ends_starts_equal_the_restatement_on_masked_targets(gpu):
    mat, queries, ts, expect = _masked_case()
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    b = gpu.sw_prepare_masked(mat, 11, 1, queries, mode=1)
    b.run()
    got = b.fetch()
    b.free()
    assert len(got) == len(expect) == 40 * len(QUERY_LENS)
    for p, r in enumerate(expect):
        assert rec_tuple(got[p]) == oracle_tuple(r), (p, QUERY_LENS[p // 40])
    scores = np.array([r["score"] for r in expect]).reshape(len(QUERY_LENS), 40)
    assert (scores[1:, :24] > 30).mean() > 0.4 and sum(r["word"] for r in expect) > 20      # masked second alignments that still score


def test_tracebacks_of_a_masked_batch_equal_the_restatement(gpu):
    mat, queries, ts, expect = _masked_case()
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    b = gpu.sw_prepare_masked(mat, 11, 1, queries, mode=1)
    b.run()
    info, strs = b.traceback(np.arange(len(expect), dtype=np.uint32))
    b.free()
    n = 0
    for p, r in enumerate(expect):
        if r["score"] > 0:
            assert int(info[p]["status"]) == 0 and strs[p] == r["bt"] and int(info[p]["ident"]) == r["ident"], p
            n += 1
        else:
            assert int(info[p]["status"]) == 3, p
    assert n > 150


# ---- 4. block aligner --------------------------------------------------------------------------------------------------------
def test_block_aligner_and_block_starts_on_a_masked_batch(gpu, matrices, oracle):
    """The second alignments of three-domain targets, still in the int16 range: mmgpu_sw_block_backtrace against the restated block
    aligner on the masked target, and mmgpu_sw_block_starts by the rule of test_block_starts_is_the_search_semantics_of_one_call."""
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(303)
    ts, queries = [], []
    for qlen in (61, 130, 530):
        for _ in range(3):
            q = rng.integers(0, 20, qlen).astype(np.uint8)
            cb = comp_bias(oracle, matrices, q)
            mine, masks = [], []
            for k in range(8):
                t = repeats_target(rng, q, 3, 0.8, 0.95) if k < 6 else rng.integers(0, 20, 200).astype(np.uint8)
                r = oracle.sw_align(q, cb, t, mat, 11, 1, need_start=True)
                mine.append(len(ts))
                ts.append(t)
                masks.append([(r["t_start"], r["t_end"])] if r["score"] > 0 else None)
            queries.append(dict(q=q, comp_bias=cb, targets=np.array(mine, np.uint32), masks=masks, min_start_score=40))
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    b1 = gpu.sw_prepare_masked(mat, 11, 1, queries, mode=1)
    b1.run()
    ref = b1.fetch()
    pair_q = np.repeat(np.arange(len(queries)), 8)
    masked_t = [host_masked(ts[p], queries[p // 8]["masks"][p % 8]) for p in range(len(ref))]
    word = np.nonzero((ref["word"] == 1) & (ref["score"] > 0))[0].astype(np.uint32)
    assert len(word) >= 30
    blk, strs = b1.block_backtrace(word)
    n_ok = 0
    for k, p in enumerate(word):
        qd = queries[int(pair_q[p])]
        w = oracle.block_backtrace(qd["q"], qd["comp_bias"], masked_t[p], mat, 11, 1, int(ref[p]["score"]), int(ref[p]["q_end"]), int(ref[p]["t_end"]))
        assert int(blk[k]["status"]) == (0 if w["ok"] else 1), p
        if w["ok"]:
            assert (int(blk[k]["q_start"]), int(blk[k]["t_start"]), int(blk[k]["ident"]), strs[k]) == (w["q_start"], w["t_start"], w["ident"], w["bt"]), p
            n_ok += 1
    assert n_ok >= len(word) - max(3, len(word) // 20)
    # block_starts: what mode 1 + an explicit block_backtrace call + the host's choice between the two give
    sel = np.nonzero((ref["word"] == 1) & (ref["score"] >= 40) & (ref["score"] > 0))[0].astype(np.uint32)
    starts, _ = b1.block_backtrace(sel, mode="starts")
    b1.free()
    expect = ref.copy()
    ok = starts["status"] == 0
    assert set(np.unique(starts["status"]).tolist()) <= {0, 1}
    expect["q_start"][sel[ok]] = starts["q_start"][ok]
    expect["t_start"][sel[ok]] = starts["t_start"][ok]
    b2 = gpu.sw_prepare_masked(mat, 11, 1, queries, mode=2)
    b2.run()
    n_sel, n_declined, n_large = b2.block_starts()
    got = b2.fetch()
    b2.free()
    assert n_sel == len(sel) and n_declined == int((~ok).sum()) and n_large == 0
    assert np.array_equal(got, expect)
    for p in sel[~ok]:      # declined: the reverse scan's start on the masked target
        qd = queries[int(pair_q[p])]
        r = oracle.sw_align(qd["q"], qd["comp_bias"], masked_t[p], mat, 11, 1, need_start=True)
        assert (int(got[p]["q_start"]), int(got[p]["t_start"])) == (r["q_start"], r["t_start"]), p


# ---- 5. profile queries ---------------------------------------------------------------------------------------------------
def test_profile_queries_against_masked_targets(gpu, matrices, oracle):
    from tests.test_profile_query import cases, mutate
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(404)
    ts, queries = [], []
    for e, mine in cases(rng, mat, n_queries=4):
        cons = e[:, 20].astype(np.uint8)
        prof = (e[:, :20].astype(np.int32) / 4).astype(np.int8).T.copy()
        # two-domain targets (the second alignment has something left to find) beside two of the single-domain ones
        mine = mine[:2] + [np.concatenate([mutate(rng, cons, 0.8), rng.integers(0, 20, 20).astype(np.uint8), mutate(rng, cons, ident)])
                           for ident in (0.9, 0.7, 0.6, 0.45)]
        masks = []
        for t in mine:
            r = oracle.sw_align_profile(prof, cons, t, 21, 11, 1, need_start=True)
            a = int(rng.integers(0, len(t) + 1))
            masks.append(([(r["t_start"], r["t_end"])] if r["score"] > 0 else []) + [(a, min(len(t), a + 9))])
        queries.append(dict(q=cons, comp_bias=None, profile=prof, targets=np.arange(len(ts), len(ts) + len(mine), dtype=np.uint32),
                            masks=masks, min_start_score=0))
        ts += mine
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    b = gpu.sw_prepare_masked(mat, 11, 1, queries, mode=1)
    b.run()
    got = b.fetch()
    info, strs = b.traceback(np.arange(len(got), dtype=np.uint32))
    b.free()
    p = n = 0
    for qd in queries:
        for t_id, m in zip(qd["targets"], qd["masks"]):
            o = oracle.sw_align_profile(qd["profile"], qd["q"], host_masked(ts[int(t_id)], m), 21, 11, 1, need_start=True, need_bt=True)
            assert rec_tuple(got[p])[:3] + (int(got[p]["word"]),) == (o["score"], o["q_end"], o["t_end"], o["word"]), p
            if o["t_end"] != -1:
                assert (int(got[p]["q_start"]), int(got[p]["t_start"])) == (o["q_start"], o["t_start"]), p
                assert int(info[p]["status"]) == 0 and strs[p] == o["bt"] and int(info[p]["ident"]) == o["ident"], p
                n += 1
            p += 1
    assert n >= 16


# ---- 6. chains -------------------------------------------------------------------------------------------------------------
def test_alt_alignments_walk_the_recorded_reference_chains(gpu, matrices):
    par, fams = load_alt_ali_vectors()
    mat = matrices["blosum62_sw"]
    gpu.load_targets(*wl.seqs_from_list([f["t"] for f in fams]), 21)
    queries = [dict(q=f["q"], comp_bias=f["cb"], targets=np.array([k], np.uint32), min_start_score=0) for k, f in enumerate(fams)]
    first = np.zeros(len(fams), capi.SW_HIT_DTYPE)
    for k, f in enumerate(fams):
        for name, v in zip(("score", "q_end", "t_end", "q_start", "t_start", "word"), f["chain"][0][0]):
            first[k][name] = v
    # the first alignments themselves, on the unmasked targets
    assert np.array_equal(gpu.sw_batch(mat, par["gap_open"], par["gap_extend"], queries, mode=1), first)
    seen = [[] for _ in fams]      # every record checkCriteria is shown, the rejected last one of a chain included

    def accept(qi, records):
        assert len(records) == 1
        seen[qi].append(rec_tuple(records[0]))
        return records["score"] >= par["threshold"]

    out = capi.alt_alignments(gpu, mat, par["gap_open"], par["gap_extend"], queries, first, par["max_rounds"], accept,
                              mask_letter=par["mask_letter"], want_bt=True)
    for k, f in enumerate(fams):
        rest = f["chain"][1:]
        assert seen[k] == [tuple(row[:6]) for row, _ in rest], (len(f["q"]), "round by round")
        good = [(row, bt) for row, bt in rest if row[0] >= par["threshold"]]
        assert len(out[k]) == len(good)
        for d, (row, bt) in zip(out[k], good):
            assert [d[x] for x in ("score", "q_end", "t_end", "q_start", "t_start", "word", "ident")] == row and d["bt"] == bt, len(f["q"])
    assert seen[0] == [tuple(fams[0]["chain"][0][0][:6])]      # the one-residue alignment masks nothing: the same alignment again
    # ... and again in every remaining round while it is accepted
    again = capi.alt_alignments(gpu, mat, par["gap_open"], par["gap_extend"], queries[:1], first[:1], 3, lambda qi, r: np.ones(len(r), bool))
    assert [tuple(d[x] for x in REC) for d in again[0]] == [tuple(fams[0]["chain"][0][0][:6])] * 3


# ---- 7. all spans empty ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_empty_spans_give_the_plain_batch(gpu, mode):
    mat, queries, ts, _ = _masked_case()
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    plain = gpu.sw_prepare(mat, 11, 1, queries, mode=mode)
    plain.run()
    want = plain.fetch()
    rng = np.random.default_rng(707)
    empty = []
    for qd in queries:      # no list, no spans, spans without a residue
        kinds = rng.integers(0, 3, len(qd["targets"]))
        empty.append(dict(qd, masks=None if len(empty) == 0 else [None if k == 0 else [] if k == 1 else [(int(k), int(k))] * 2 for k in kinds]))
    b = gpu.sw_prepare_masked(mat, 11, 1, empty, mode=mode)
    b.run()
    got = b.fetch()
    assert np.array_equal(got, want)
    assert (b.cells, b.pairs) == (plain.cells, plain.pairs)
    if mode == 2:
        assert b.block_starts() == plain.block_starts()
        assert np.array_equal(b.fetch(), plain.fetch())
    b.free()
    plain.free()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, matrices):
    import ctypes
    import mmseqs2_amd
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(808)
    ts = [rng.integers(0, 20, n).astype(np.uint8) for n in (50, 7)]
    q = rng.integers(0, 20, 30).astype(np.uint8)
    qd = dict(q=q, comp_bias=None, targets=np.array([0, 1], np.uint32), min_start_score=0)
    par, arr, keep = gpu._marshal(mat, 11, 1, [qd])

    def status(g, span_off, spans, letter=X, masks=True):
        span_off, spans = np.array(span_off, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)
        mk = capi.SwMasks(span_off.ctypes.data_as(capi.c_p), spans.ctypes.data_as(capi.c_p), letter)
        h = capi.c_p(1)
        rc = g.L.mmgpu_sw_prepare_masked(g.ctx, ctypes.byref(par), ctypes.cast(arr, capi.c_p), 1, 1, ctypes.byref(mk) if masks else None, ctypes.byref(h))
        if rc == 0:
            g.L.mmgpu_sw_free(g.ctx, h)
        else:
            assert h.value is None, "a refused call returns no batch"
        return rc

    fresh = mmseqs2_amd.MMGpu(0)
    try:
        assert status(fresh, [0, 1, 1], [(0, 5)]) == -3      # MMGPU_ERR_STATE: no targets loaded
    finally:
        fresh.close()
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    assert status(gpu, [0, 1, 2], [(0, 50), (0, 7)]) == 0
    assert status(gpu, [0, 1, 2], [(0, 50), (0, 8)]) == -1      # beyond the target's length
    assert status(gpu, [0, 1, 2], [(0, 51), (0, 7)]) == -1
    assert status(gpu, [0, 1, 2], [(6, 5), (0, 7)]) == -1       # t_from > t_to
    assert status(gpu, [0, 2, 1], [(0, 5), (0, 5)]) == -1       # span_off not monotone
    assert status(gpu, [0, 1, 2], [(0, 5), (0, 5)], letter=21) == -1
    assert status(gpu, [0, 1, 2], [(0, 5), (0, 5)], letter=-1) == -1
    assert status(gpu, [0, 1, 2], [(0, 5), (0, 5)], masks=False) == -1
    # the debug aid on a plain batch
    b = gpu.sw_prepare(mat, 11, 1, [qd], mode=1)
    with pytest.raises(capi.MMGpuError):
        b.debug_masked_target(0)
    b.free()
    del keep


def test_span_off_may_start_beyond_zero(gpu, matrices):
    """span_off numbers the caller's span array: a list that starts at span 3 reads spans[3 ..], not the three before it"""
    mat = matrices["blosum62_sw"]
    rng = np.random.default_rng(909)
    ts = [rng.integers(0, 20, n).astype(np.uint8) for n in (50, 7)]
    gpu.load_targets(*wl.seqs_from_list(ts), 21)
    qd = dict(q=rng.integers(0, 20, 30).astype(np.uint8), comp_bias=None, targets=np.array([0, 1], np.uint32), min_start_score=0)
    par, arr, keep = gpu._marshal(mat, 11, 1, [qd])
    span_off = np.array([3, 5, 6], np.uint32)
    spans = np.array([(0, 50), (0, 50), (0, 50), (10, 20), (30, 31), (2, 5)], np.uint32)      # the first three belong to nobody
    b = gpu._sw_prepare_masked_raw(par, arr, keep, 1, span_off, spans, 1, X)
    for p, want in enumerate([host_masked(ts[0], [(10, 20), (30, 31)]), host_masked(ts[1], [(2, 5)])]):
        got, n = b.debug_masked_target(p)
        assert n == len(want) and np.array_equal(got[:n], want) and (got[n:] == 21).all(), p
    b.free()
