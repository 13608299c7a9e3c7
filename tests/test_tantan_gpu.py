"""tantan masking on the device (mmgpu_pf_mask_targets, tantan_kernel.hip) at its edges.  Every comparison is exact: the masked bytes
and the returned count.  What the device is compared with:
  * its own repeat probabilities, float for float, through the public call (the two-threshold method, test 1);
  * tests/golden/tantan_edge_vectors.npz, recorded from the compiled reference (test 2);
  * the restatement oracle/tantan_oracle.c, which tests/test_tantan.py and tests/test_tantan_edges.py pin to the compiled reference
    (all others; the nucleotide table of test 7 is synthetic, so that one is device against restatement and nothing more).
The inputs are the sets of tests/tantan_cases.py; nothing here reads the reference tree."""
import os
import time

import numpy as np
import pytest

from tests import tantan_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F09, F05 = float(np.float32(0.9)), float(np.float32(0.5))
TABLES = ("vtml80", "blosum62")


@pytest.fixture(scope="module")
def edge():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "tantan_edge_vectors.npz")))


def device_mask(gpu, res, off, lr, thr, mask_letter=20, load=True):
    if load:
        gpu.load_targets(res, off, lr.shape[0])
    n = gpu.pf_mask_targets(lr, thr, mask_letter)
    return gpu.pf_debug_masked_targets(off), n


def restated_probs(oracle, seqs, lr):
    return np.concatenate([oracle.tantan_probs(t, lr) for t in seqs] + [np.zeros(0, np.float32)])


def assert_device_equals_restatement(gpu, oracle, seqs, lr, thr=F09, mask_letter=20):
    res, off = tc.pack(seqs)
    got, n = device_mask(gpu, res, off, lr, thr, mask_letter)
    want, n_want = oracle.tantan_mask(res, off, lr, thr, mask_letter)
    assert n == n_want
    assert np.array_equal(got, want)
    return n


# ---- 1. exact probabilities through the public call ----
@pytest.mark.parametrize("table", TABLES)
def test_every_probability_of_the_probe_set_is_the_restatements_float(gpu, oracle, edge, table):
    """The call returns masks, not probabilities; but a mask at threshold v says of every letter whether its float is >= v.  For every
    distinct probability v of the probe set (8 sequences in one wavefront: periods 7 and 37, a homopolymer run, an X, background,
    lengths 15 16 17 49 50 51) the device masks once at float64(v) and once at the next float above v; each mask must be
    {k : p_k >= threshold} of the restatement's p.  The first says the device's float of every letter with p_k = v is >= v, the
    second that it is below the next float: it is v.  A letter whose device float were off by one ulp or more fails one of the
    two masks of its own value.
    Measured on one MI355X: 320 (VTML80) and 326 (BLOSUM62) distinct values among the 388 letters, so 640 and 652 calls, 0.65 ms
    per call (the masking call 0.6 ms, the rest is reading the mask back): half a second per table."""
    lr = edge[table + "_likelihood_ratios"]
    seqs = tc.probe_set()
    res, off = tc.pack(seqs)
    assert len(res) <= 400 and len(seqs) <= 8
    p = restated_probs(oracle, seqs, lr)
    p64 = p.astype(np.float64)
    values = np.unique(p)
    assert len(values) > len(res) // 2      # (not a set of a few repeated values: nearly every letter is pinned on its own)
    gpu.load_targets(res, off, 21)
    t0 = time.perf_counter()
    for v in values:
        for thr in (float(np.float64(v)), float(np.float64(np.nextafter(np.float32(v), np.float32(np.inf))))):
            want = p64 >= thr
            got, n = device_mask(gpu, res, off, lr, thr, load=False)
            assert n == int(want.sum()), (table, float(v), thr)
            assert np.array_equal(got, np.where(want, 20, res).astype(np.uint8)), (table, float(v), thr)
    dt = time.perf_counter() - t0
    print("probe set, %s: %d letters, %d distinct probabilities, %d calls, %.3f ms per call" % (
        table, len(res), len(values), 2 * len(values), 1e3 * dt / (2 * len(values))))


# ---- 2. the recorded edge vectors ----
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("name", tc.SET_NAMES + ("all",))
def test_device_equals_the_recorded_edge_vectors(gpu, edge, name, table):
    lr = edge[table + "_likelihood_ratios"]
    names = tc.SET_NAMES if name == "all" else (name,)
    res = np.concatenate([edge[s + "_res"] for s in names])
    lens = np.concatenate([np.diff(edge[s + "_off"].astype(np.int64)) for s in names])
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    gpu.load_targets(res, off, 21)
    for key, thr in (("09", F09), ("05", F05)):
        want = np.concatenate([edge["%s_%s_masked_%s" % (s, table, key)] for s in names])
        n_want = sum(int(edge["%s_%s_n_%s" % (s, table, key)]) for s in names)
        got, n = device_mask(gpu, res, off, lr, thr, load=False)
        assert n == n_want and n_want > 0, (name, table, key)
        assert np.array_equal(got, want), (name, table, key)


# ---- 3. thresholds ----
def test_thresholds_from_everything_to_nothing(gpu, oracle, edge):
    """0.0 masks every letter whose float is >= 0 - the ones that are exactly 0 included (the set has 52: every first letter);
    1.0 only a float of exactly 1 (the set has some 300); 1.5 nothing."""
    lr = edge["vtml80_likelihood_ratios"]
    seqs = tc.periods_set()
    p = restated_probs(oracle, seqs, lr)
    assert (p == 0).any() and (p == 1).any()      # (the first letter of a sequence can be in no repeat)
    counts = []
    for thr in (0.0, F05, 0.99, 1.0, 1.5):
        n = assert_device_equals_restatement(gpu, oracle, seqs, lr, thr)
        assert n == int((p.astype(np.float64) >= thr).sum())
        counts.append(n)
    assert counts[0] == int((p >= 0).sum()) and counts[0] > counts[1] > counts[2] >= counts[3] >= 0 and counts[4] == 0


# ---- 4. wavefront composition ----
@pytest.mark.parametrize("n_seqs", [1, 63, 64, 65, 129])
def test_database_sizes_around_one_wavefront(gpu, oracle, edge, n_seqs):
    assert assert_device_equals_restatement(gpu, oracle, tc.mixed_lengths(n_seqs, 800 + n_seqs), edge["vtml80_likelihood_ratios"]) > 0


def test_lanes_of_very_different_lengths_share_a_wavefront(gpu, oracle, edge):
    rng = np.random.default_rng(811)
    seqs = [tc.background(rng, n) for n in (3000, 50, 16, 1, 0)]
    tc.plant(rng, seqs[0], 2900, 23, 95)
    tc.plant(rng, seqs[0], 5, 2, 30)
    tc.plant(rng, seqs[1], 10, 4, 40)
    tc.plant(rng, seqs[2], 0, 1, 16)
    assert assert_device_equals_restatement(gpu, oracle, seqs, edge["vtml80_likelihood_ratios"]) > 100


def test_a_wavefront_of_equal_lengths_and_empty_sequences_at_both_ends(gpu, oracle, edge):
    lr = edge["vtml80_likelihood_ratios"]
    rng = np.random.default_rng(812)
    same = [tc.background(rng, 77) for _ in range(64)]
    for k in range(0, 64, 5):
        tc.plant(rng, same[k], k % 30, 1 + k % 50, 40)
    assert assert_device_equals_restatement(gpu, oracle, same, lr) > 100
    ends = [np.zeros(0, np.uint8)] + tc.mixed_lengths(20, 813) + [np.zeros(0, np.uint8)]
    assert assert_device_equals_restatement(gpu, oracle, ends, lr) > 0


# ---- 5. the longest admitted sequence ----
def test_the_longest_sequences(gpu, oracle, edge):
    """65 535 letters (4096 scale slots), 65 520 (a multiple of 16: the last letter rescales) and 65 519 beside a 1-letter sequence in
    one wavefront, repeats planted at 10 .. 200 and 65 000 .. 65 400.  Measured on one MI355X: the masking call of this database
    with its read back 0.25 s, the call for the 65 535-letter sequence alone 0.22 - 0.26 s (one lane of one wavefront for
    2 x 65 535 steps, whatever else shares the wavefront): all three lengths stay."""
    lr = edge["vtml80_likelihood_ratios"]
    rng = np.random.default_rng(821)
    seqs = [tc.long_sequence(65535, 41), tc.background(rng, 1), tc.long_sequence(65520, 42), tc.long_sequence(65519, 43)]
    res, off = tc.pack(seqs)
    gpu.load_targets(res, off, 21)
    t0 = time.perf_counter()
    got, n = device_mask(gpu, res, off, lr, F09, load=False)
    print("longest sequences: masking call + read back %.3f s" % (time.perf_counter() - t0))
    want, n_want = oracle.tantan_mask(res, off, lr, F09)
    assert n == n_want and n_want > 600
    assert np.array_equal(got, want)


# ---- 6. chunking ----
def test_every_wavefront_its_own_chunk(gpu, oracle, edge, monkeypatch):
    """MMGPU_TANTAN_SCRATCH_MB=0: no two wavefronts fit the scratch, so each of the three (64 + 64 + 2 sequences) is launched on its
    own, the partial one last, into scratch that the one before just used."""
    lr = edge["vtml80_likelihood_ratios"]
    seqs = tc.mixed_lengths(130, 831, max_len=400)
    res, off = tc.pack(seqs)
    whole, n_whole = device_mask(gpu, res, off, lr, F09)
    monkeypatch.setenv("MMGPU_TANTAN_SCRATCH_MB", "0")
    chunked, n_chunked = device_mask(gpu, res, off, lr, F09)
    want, n_want = oracle.tantan_mask(res, off, lr, F09)
    assert n_chunked == n_whole == n_want and n_want > 500
    assert np.array_equal(chunked, whole) and np.array_equal(chunked, want)


# ---- 7. another alphabet, another mask letter ----
def test_nucleotide_alphabet_and_mask_letter(gpu, oracle):
    """Device against restatement only: the 5 x 5 table is synthetic (3.5 match, 0.4 mismatch, 1 against N), no reference data is
    involved.  Alphabet 5 (rows of the table 5 wide, LDS rows 32), mask letter 4, planted periods 1 .. 50."""
    lr = tc.nucleotide_table()
    seqs = tc.nucleotide_set()
    for thr in (F09, F05):
        n = assert_device_equals_restatement(gpu, oracle, seqs, lr, thr, mask_letter=4)
        assert n > 2000
    p09 = restated_probs(oracle, seqs, lr).astype(np.float64) >= F09
    off = tc.pack(seqs)[1].astype(np.int64)
    for p in range(1, 51):      # every planted period is found
        a, n = tc.period_layout(p)
        assert p09[off[p - 1] + a:off[p - 1] + a + n].sum() >= p, p


@pytest.mark.parametrize("name", tc.SET_NAMES)
def test_protein_sets_with_mask_letter_3(gpu, oracle, edge, name):
    """Device against restatement: the reference always masks with X."""
    seqs = tc.all_sets()[name]
    assert assert_device_equals_restatement(gpu, oracle, seqs, edge["vtml80_likelihood_ratios"], F09, mask_letter=3) > 0


# ---- 8. state ----
def test_masking_again_replaces_the_mask(gpu, oracle, edge):
    lr = edge["vtml80_likelihood_ratios"]
    res, off = edge["periods_res"], edge["periods_off"]
    m05, n05 = device_mask(gpu, res, off, lr, F05)
    m09, n09 = device_mask(gpu, res, off, lr, F09, load=False)
    assert n05 == int(edge["periods_vtml80_n_05"]) and n09 == int(edge["periods_vtml80_n_09"]) and n09 < n05
    assert np.array_equal(m05, edge["periods_vtml80_masked_05"])
    assert np.array_equal(m09, edge["periods_vtml80_masked_09"])      # not the union with the 0.5f mask


def test_unmasking_and_masking_again(gpu, edge):
    lr = edge["vtml80_likelihood_ratios"]
    res, off = edge["periods_res"], edge["periods_off"]
    first, n_first = device_mask(gpu, res, off, lr, F09)
    assert n_first == int(edge["periods_vtml80_n_09"]) and not np.array_equal(first, res)
    assert gpu.pf_mask_targets(None) == 0
    assert np.array_equal(gpu.pf_debug_masked_targets(off), res)
    assert gpu.pf_mask_targets(None) == 0      # unmasking the unmasked
    assert np.array_equal(gpu.pf_debug_masked_targets(off), res)
    again, n_again = device_mask(gpu, res, off, lr, F09, load=False)
    assert n_again == n_first and np.array_equal(again, first)


def test_unmasking_through_the_multi_context(edge):
    from mmseqs2_amd import capi
    lr = edge["vtml80_likelihood_ratios"]
    m = capi.MMGpuMulti([0, 0])
    try:
        m.load_targets(edge["periods_res"], edge["periods_off"], 21)
        n_want = int(edge["periods_vtml80_n_09"])
        assert m.pf_mask_targets(lr, F09, 20) == n_want
        assert m.pf_mask_targets(None) == 0
        assert m.pf_mask_targets(lr, F09, 20) == n_want
    finally:
        m.close()


def test_refused_arguments(gpu, edge):
    from mmseqs2_amd.capi import MMGpuError
    lr = edge["vtml80_likelihood_ratios"]
    gpu.load_targets(edge["letters_res"], edge["letters_off"], 21)
    with pytest.raises(MMGpuError, match="alphabet differs from the loaded targets"):
        gpu.pf_mask_targets(tc.nucleotide_table(), F09, 4)
    with pytest.raises(MMGpuError, match="mask letter outside the alphabet"):
        gpu.pf_mask_targets(lr, F09, 21)
    with pytest.raises(MMGpuError, match="mask letter outside the alphabet"):
        gpu.pf_mask_targets(lr, F09, -1)
    # a refused call leaves the resident targets as they were
    got, n = device_mask(gpu, edge["letters_res"], edge["letters_off"], lr, F09, load=False)
    assert n == int(edge["letters_vtml80_n_09"]) and np.array_equal(got, edge["letters_vtml80_masked_09"])
