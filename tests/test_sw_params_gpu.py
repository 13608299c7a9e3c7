"""GPU parity tests (pytest -m gpu) of the Smith-Waterman kernels away from BLOSUM62 11/1: the parameter table of
tests/sw_param_cases.py against the reference's recorded results (tests/golden/sw_param_vectors.npz) and against the plain-C
restatement (pinned to the reference at the same points by tests/test_sw_params.py), settings the acceptance rule refuses,
engineered ties, the uint8/int16 boundary, saturated hits with start positions and sequences of the maximal 65535 residues.
Bar: bit-exact integers (score, q_end, t_end, q_start, t_start, word)."""
import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from mmseqs2_amd.capi import MMGpuError
from tests import sw_param_cases as pc

pytestmark = pytest.mark.gpu

MMGPU_ERR_UNSUPPORTED = -4      # include/mmgpu.h
FIELDS = ("score", "q_end", "t_end", "q_start", "t_start", "word")


@pytest.fixture(scope="module")
def param_sets():
    return pc.load_param_vectors()


def _cb(oracle, v, q):
    """composition bias of q as ssw_init rounds it, from the set's own matrix and background"""
    return oracle.round_comp_bias(oracle.comp_bias(v["mat"].astype(np.int16), v["pback"], q, 1.0))


def _expect(oracle, v, q, cb, t, mode, min_start=0):
    """the record the device has to return for one pair in this mode, from the restatement"""
    r = oracle.sw_align(q, cb, t, v["mat"], v["go"], v["ge"], need_start=mode >= 1)
    start = mode >= 1 and r["score"] > 0 and r["score"] >= min_start and not (mode == 2 and r["word"] == 1)
    return (r["score"], r["q_end"], r["t_end"], r["q_start"] if start else -1, r["t_start"] if start else -1, r["word"])


def _check(hits, oracle, v, q, cb, targets, mode, tag):
    for k, t in enumerate(targets):
        got = tuple(int(hits[k][f]) for f in FIELDS)
        exp = _expect(oracle, v, q, cb, t, mode)
        assert got == exp, (tag, k, len(q), len(t), got, exp)


def test_param_goldens_on_device(gpu, param_sets):
    """Every recorded pair of every set, forward and reverse scan: the device against the reference's recorded numbers directly."""
    for key, v in param_sets.items():
        tres, toff = wl.seqs_from_list([p[2] for p in v["pairs"]])
        gpu.load_targets(tres, toff, 21)
        queries = [dict(q=q, comp_bias=cb, targets=np.array([i], np.uint32), min_start_score=0) for i, (q, cb, t, exp) in enumerate(v["pairs"])]
        out = gpu.sw_batch(v["mat"], v["go"], v["ge"], queries, mode=1)
        n_word = 0
        for i, (q, cb, t, exp) in enumerate(v["pairs"]):
            got = [int(out[i][f]) for f in FIELDS]
            assert got == [int(x) for x in exp[:6]], (key, i, got, exp[:6].tolist())
            n_word += got[5]
        assert n_word >= 5, key


@pytest.mark.parametrize("key", [s[0] for s in pc.SW_PARAM_SETS])
def test_parameter_sets_across_tile_classes(gpu, oracle, param_sets, key):
    """Per set: queries of the register groups S / M / L and of two and four tiles, each with its composition bias from the
    set's own matrix, against 200 targets of the shared generator (homologs of the query among them); queries the acceptance rule
    refuses are not sent (at most 20 % of them)."""
    v = param_sets[key]
    rng = np.random.default_rng(sum(map(ord, key)))
    lengths = [5, 97, 200, 330, 448, 512, 513, 700, 1400]
    n_out = 0
    for qlen in lengths:
        q = rng.choice(21, size=qlen, p=np.append(wl.BACKGROUND * 0.99, 0.01)).astype(np.uint8)
        cb = _cb(oracle, v, q)
        if not pc.rule_accepts(oracle, v["mat"], cb, qlen, v["go"], v["ge"]):
            n_out += 1
            continue
        targets = [t for _, _, t in pc.generate_pairs(1000 + qlen, 150)]
        for k in range(50):
            h = wl.mutate(rng, q, float(rng.uniform(0.3, 1.0))) if qlen > 12 else q.copy()
            if k % 2:
                pre = rng.choice(20, size=int(rng.integers(0, 60)), p=wl.BACKGROUND).astype(np.uint8)
                h = np.concatenate([pre, h, pre[::-1]])
            targets.append(h)
        tres, toff = wl.seqs_from_list(targets)
        gpu.load_targets(tres, toff, 21)
        ids = rng.permutation(len(targets)).astype(np.uint32)
        out = gpu.sw_batch(v["mat"], v["go"], v["ge"], [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=1)
        _check(out, oracle, v, q, cb, [targets[i] for i in ids], 1, (key, qlen))
    assert n_out <= pc.MAX_REFUSED_SHARE * len(lengths), (key, n_out)


def test_refused_settings_are_refused(gpu, oracle, param_sets):
    """gap_open == gap_extend, a matrix whose minimum leaves the rule (PAM30 at 11/1) and a homopolymer query whose composition
    bias leaves it at 8/2: MMGPU_ERR_UNSUPPORTED (the reference accepts these settings, the host falls back to its own aligner),
    and the context serves a valid batch right after."""
    v62, vpam, v82 = param_sets["blosum62_11_1"], param_sets["pam30_25_2"], param_sets["blosum62_8_2"]
    rng = np.random.default_rng(5)
    q = rng.choice(20, size=150, p=wl.BACKGROUND).astype(np.uint8)
    targets = [wl.mutate(rng, q, 0.7), rng.choice(20, size=200, p=wl.BACKGROUND).astype(np.uint8)]
    tres, toff = wl.seqs_from_list(targets)
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(2, dtype=np.uint32)
    # a homopolymer whose composition bias reaches -6: -4 + -6 + 2 > -8 fails (without the bias the same query is inside the rule)
    homo = next(h for h in (np.full(120, a, np.uint8) for a in range(20))
                if not pc.rule_accepts(oracle, v82["mat"], _cb(oracle, v82, h), len(h), 8, 2))
    cb_homo = _cb(oracle, v82, homo)
    assert pc.rule_accepts(oracle, v82["mat"], None, len(homo), 8, 2)
    cases = [("6/6", v62["mat"], 6, 6, [dict(q=q, comp_bias=None, targets=ids)]),
             ("12/12", v62["mat"], 12, 12, [dict(q=q, comp_bias=None, targets=ids)]),
             ("pam30 11/1", vpam["mat"], 11, 1, [dict(q=q, comp_bias=None, targets=ids)]),
             ("homopolymer 8/2", v82["mat"], 8, 2, [dict(q=q, comp_bias=None, targets=ids), dict(q=homo, comp_bias=cb_homo, targets=ids)])]
    for name, mat, go, ge, queries in cases:
        with pytest.raises(MMGpuError) as e:
            gpu.sw_prepare(mat, go, ge, queries, mode=1)
        assert "error %d:" % MMGPU_ERR_UNSUPPORTED in str(e.value), (name, str(e.value))
        out = gpu.sw_batch(v62["mat"], 11, 1, [dict(q=q, comp_bias=None, targets=ids, min_start_score=0)], mode=1)
        _check(out, oracle, v62, q, None, targets, 1, "after " + name)


@pytest.mark.parametrize("key", ["blosum62_11_1", "blosum62_5_2"])
def test_engineered_ties(gpu, oracle, param_sets, key):
    """Equal maxima on purpose (sw_param_cases.engineered_tie_pairs), forward and reverse scan.  The full DP (numpy, in
    sw_param_cases.classify_ties) says for every pair where the final maximum recurs: (a) in two rows of one lane's strip,
    (b) in different lanes of one 16-lane group, (c) in different tiles, (d) in columns more than one four-letter block apart -
    every category has to occur, for the forward scan in both sets and for the reverse scan where the matrix and the gap costs
    allow the construction (5/2), so that the constructions cannot rot into a test of nothing."""
    v = param_sets[key]
    pairs = pc.engineered_tie_pairs(v["mat"], v["go"])
    tres, toff = wl.seqs_from_list([t for _, _, t in pairs])
    gpu.load_targets(tres, toff, 21)
    queries = [dict(q=q, comp_bias=None, targets=np.array([i], np.uint32), min_start_score=0) for i, (_, q, _) in enumerate(pairs)]
    out = gpu.sw_batch(v["mat"], v["go"], v["ge"], queries, mode=1)
    n_fwd, n_rev = dict.fromkeys("abcd", 0), dict.fromkeys("abcd", 0)
    for i, (name, q, t) in enumerate(pairs):
        fwd, rev, by_dp = pc.classify_ties(q, None, t, v["mat"], v["go"], v["ge"])
        exp = _expect(oracle, v, q, None, t, 1)
        assert exp[:5] == by_dp, (name, exp, by_dp)         # the test's own DP is the restatement's
        got = tuple(int(out[i][f]) for f in FIELDS)
        assert got == exp, (name, sorted(fwd), sorted(rev), got, exp)
        for c in fwd:
            n_fwd[c] += 1
        for c in rev:
            n_rev[c] += 1
    print(key, "forward ties", n_fwd, "reverse ties", n_rev)
    assert all(n > 0 for n in n_fwd.values()), n_fwd
    assert n_rev["d"] > 0, n_rev
    if key == "blosum62_5_2":
        assert all(n > 0 for n in n_rev.values()), n_rev


def _boundary_targets(oracle, v, q, cb, rng):
    """prefixes and point-mutated prefixes of q, chosen with the restatement so that score + bias takes every value 250 .. 260:
    -> {score + bias: [targets]} (up to three per value)"""
    bias = oracle.sw_bias(np.ascontiguousarray(v["mat"], np.int8), cb, len(q))
    found = {}
    first = next(n for n in range(1, len(q) + 1) if oracle.sw_align(q, cb, q[:n], v["mat"], v["go"], v["ge"])["score"] + bias >= 250)
    for trial in range(6000):
        if len(found) == 11 and all(len(x) >= 2 for x in found.values()):
            break
        n = int(rng.integers(max(first - 8, 1), min(first + 9, len(q) + 1)))
        t = q[:n].copy()
        for p in rng.integers(0, n, size=int(rng.integers(0, 4))):
            t[p] = rng.integers(0, 20)
        s = oracle.sw_align(q, cb, t, v["mat"], v["go"], v["ge"])["score"] + bias
        if 250 <= s <= 260 and len(found.setdefault(s, [])) < 3:
            found[s].append(t)
    return bias, found


@pytest.mark.parametrize("key", ["blosum62_11_1", "blosum80_11_1", "pam30_25_2"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_uint8_int16_boundary_sweep(gpu, oracle, param_sets, key, with_bias):
    """word = (score + bias >= 255) at every value of score + bias from 250 to 260, modes 1 and 2 (mode 2 leaves the start of a
    word == 1 hit at -1)."""
    v = param_sets[key]
    rng = np.random.default_rng(31 + sum(map(ord, key)) + int(with_bias))
    q = rng.choice(20, size=220, p=wl.BACKGROUND).astype(np.uint8)
    cb = _cb(oracle, v, q) if with_bias else None
    assert pc.rule_accepts(oracle, v["mat"], cb, len(q), v["go"], v["ge"])
    bias, found = _boundary_targets(oracle, v, q, cb, rng)
    assert sorted(found) == list(range(250, 261)), (key, with_bias, bias, sorted(found))
    targets = [t for s in sorted(found) for t in found[s]]
    tres, toff = wl.seqs_from_list(targets)
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(len(targets), dtype=np.uint32)
    for mode in (1, 2):
        out = gpu.sw_batch(v["mat"], v["go"], v["ge"], [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=mode)
        _check(out, oracle, v, q, cb, targets, mode, (key, with_bias, mode))
        words = {s: {int(out[k]["word"]) for k, t in enumerate(targets) if int(out[k]["score"]) + bias == s} for s in found}
        assert all(words[s] == {int(s >= 255)} for s in found), words
        if mode == 2:
            assert all(int(out[k]["q_start"]) == -1 for k in range(len(targets)) if out[k]["word"] == 1)


def test_saturated_hits_with_start_positions(gpu, oracle, param_sets):
    """The saturating self hit of tests/test_sw_params.py (score 32767) and its two partial targets: the reverse scan of a
    saturated hit (mode 1) equals the reference's fall-back, mode 2 leaves the starts of these int16-range hits open, and
    block_starts() fills them in with the block aligner's answer or, where it declines, with the reverse scan's."""
    v = param_sets["blosum62_11_1"]
    q, targets = pc.saturating_pair()
    tres, toff = wl.seqs_from_list(targets)
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(len(targets), dtype=np.uint32)
    queries = [dict(q=q, comp_bias=None, targets=ids, min_start_score=0)]
    out = gpu.sw_batch(v["mat"], 11, 1, queries, mode=1)
    _check(out, oracle, v, q, None, targets, 1, "saturated mode 1")
    assert int(out[0]["score"]) == 32767 and (out["word"] == 1).all()
    b = gpu.sw_prepare(v["mat"], 11, 1, queries, mode=2)
    b.run()
    _check(b.fetch(), oracle, v, q, None, targets, 2, "saturated mode 2")
    n_sel, n_declined, n_large = b.block_starts()
    got = b.fetch()
    b.free()
    assert n_sel == len(targets)
    print("block_starts on the saturated pairs: selected %d, declined %d, too large %d" % (n_sel, n_declined, n_large))
    n_block = 0
    for k, t in enumerate(targets):
        w = oracle.block_backtrace(q, None, t, v["mat"], 11, 1, int(out[k]["score"]), int(out[k]["q_end"]), int(out[k]["t_end"]))
        exp = (w["q_start"], w["t_start"]) if w["ok"] else (int(out[k]["q_start"]), int(out[k]["t_start"]))
        n_block += w["ok"]
        assert (int(got[k]["q_start"]), int(got[k]["t_start"])) == exp, (k, w["ok"], got[k], exp)
        assert tuple(int(got[k][f]) for f in ("score", "q_end", "t_end", "word")) == tuple(int(out[k][f]) for f in ("score", "q_end", "t_end", "word"))
    assert n_declined == len(targets) - n_block


def test_maximal_lengths(gpu, oracle, param_sets):
    """65535 residues, the longest sequence the 16-bit column / row fields of the result key can describe: a hit that ends in the
    last column (t_end == 65534), one that ends in the last row (q_end == 65534), and each with an equal copy earlier (the earlier
    one wins)."""
    v = param_sets["blosum62_11_1"]
    for name, q, t, (q_end, t_end) in pc.maximal_length_cases():
        tres, toff = wl.seqs_from_list([t])
        gpu.load_targets(tres, toff, 21)
        out = gpu.sw_batch(v["mat"], 11, 1, [dict(q=q, comp_bias=None, targets=np.zeros(1, np.uint32), min_start_score=0)], mode=1)
        _check(out, oracle, v, q, None, [t], 1, name)
        assert (int(out[0]["q_end"]), int(out[0]["t_end"])) == (q_end, t_end), name


@pytest.mark.parametrize("stride", [512, 513, 8192, 8193, 16384])
def test_list_ordering_kernel_at_every_stride_class(gpu, param_sets, stride):
    """mmgpu_sw_prepare_from_lists with synthetic device-resident lists (ids with repeats from 3000 resident targets of ragged
    lengths) of 0, 1, stride - 1 and stride entries: the counting path (lists up to 512), the bitonic network, and the strides
    8193 - 16384 that take the whole 64 KB of dynamic LDS - slot by slot what mmgpu_sw_prepare gives for the same lists from the
    host."""
    import torch
    from mmseqs2_amd import capi
    v = param_sets["blosum62_11_1"]
    rng = np.random.default_rng(stride)
    tl = [rng.choice(20, size=int(rng.integers(1, 70)), p=wl.BACKGROUND).astype(np.uint8) for _ in range(3000)]
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    counts = np.array([0, 1, stride - 1, stride, stride // 2 + 1], np.uint32)
    nq = len(counts)
    qs = [rng.choice(20, size=int(rng.integers(20, 60)), p=wl.BACKGROUND).astype(np.uint8) for _ in range(nq)]
    hits = np.zeros((nq, stride), capi.PF_HIT_DTYPE)
    hits["id"] = rng.integers(0, len(tl), size=(nq, stride))
    hits["score"] = rng.integers(15, 200, size=(nq, stride))
    for i in range(nq):
        hits[i, counts[i]:] = np.zeros((), capi.PF_HIT_DTYPE)
    d_hits = torch.from_numpy(hits.view(np.int32).reshape(nq, stride, 3).copy()).cuda()
    d_counts = torch.from_numpy(counts.astype(np.int32)).cuda()
    swq = [dict(q=q, comp_bias=None, min_start_score=30) for q in qs]
    fused = gpu.sw_prepare_from_lists(v["mat"], 11, 1, swq, d_hits.data_ptr(), d_counts.data_ptr(), stride, mode=1)
    fused.run()
    fr = fused.fetch().reshape(nq, stride)
    host_q = [dict(q=q, comp_bias=None, targets=hits[i]["id"][:counts[i]].copy(), min_start_score=30) for i, q in enumerate(qs)]
    sep = gpu.sw_prepare(v["mat"], 11, 1, host_q, mode=1)
    sep.run()
    sr = sep.fetch()
    assert fused.pairs == sep.pairs == int(counts.sum()) and fused.cells == sep.cells
    off = 0
    for i in range(nq):
        n = int(counts[i])
        for f in FIELDS:
            assert np.array_equal(fr[i, :n][f], sr[off:off + n][f]), (stride, i, f)
        assert np.all(fr[i, n:]["score"] == 0)
        off += n
    assert (sr["score"] > 0).sum() > sr.size // 2 and (sr["q_start"] >= 0).any()
    fused.free()
    sep.free()
    del d_hits, d_counts
