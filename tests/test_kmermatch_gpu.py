"""GPU tests of linclust's k-mer matching stage (mmgpu_kmermatch_*): the device's CSR against the lists recorded from the stock binary
(tests/golden/kmermatch.npz), byte for byte, and against the serial restatement (tests/kmermatch_cases.py) on generated databases the
fixture cannot hold; the engineered cases; the lifecycle; the hand-over to the ungapped rescoring.  Everything is integers and is
compared exactly."""
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import kmermatch_cases as kc
from tests import rescore_cases as rc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    return kc.Golden()


def assert_csr(got, want, tag=""):
    (off, rec), (want_off, want_rec) = got, want
    assert off.dtype == np.uint64 and rec.dtype == kc.HIT_DTYPE
    bad = np.flatnonzero(off != want_off)
    assert len(bad) == 0, (tag, "offsets", bad[:5], off[bad[:5]], want_off[bad[:5]])
    bad = np.flatnonzero(rec != want_rec)
    assert len(bad) == 0, (tag, "records", [(int(k), rec[k].tolist(), want_rec[k].tolist()) for k in bad[:5]])
    assert off.tobytes() == want_off.tobytes() and rec.tobytes() == want_rec.tobytes(), tag


def device_equals_restatement(gpu, seqs, par, tag=""):
    gpu.load_targets(*kc.pack(seqs), 21)
    got = gpu.kmermatch(par)
    assert_csr(got, kc.kmermatch(seqs, par), tag)
    return got


# ---- 1. the recorded lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_device_lists_equal_the_recorded_lists(gpu, k):
    G = golden()
    gpu.load_targets(*kc.pack(G.seqs), 21)
    assert_csr(gpu.kmermatch(G.params(G.settings[k])), G.expected(k), G.settings[k]["name"])


# ---- 2. generated databases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
def test_lognormal_database(gpu, seed):
    """2 000 sequences: more than one tile of every scan, sequences shorter than k, windows with X, families"""
    seqs = kc.lognormal_database(seed)
    par = kc.identity_params(k=10, kmers_per_seq=20, scale=0.05 if seed == 12 else 0.0)
    off, rec = device_equals_restatement(gpu, seqs, par)
    assert len(rec) > len(seqs) + 100 and min(len(s) for s in seqs) < 10 and max(len(s) for s in seqs) > 500


def test_longest_admitted_sequence(gpu):
    """32 766 residues: positions and lengths at the end of their 16 bits; with a scale the selection runs both histogram levels"""
    rng = np.random.default_rng(3)
    long_seq = kc.random_seq(rng, 32766)
    seqs = [kc.random_seq(rng, 100), long_seq, kc.mutate(rng, long_seq, 0.02)[7:20000], kc.mutate(rng, long_seq, 0.02)[20000:], long_seq[-50:].copy()]
    off, rec = device_equals_restatement(gpu, seqs, kc.identity_params(k=14, kmers_per_seq=20, scale=0.1, cov_thr=0.001))
    assert off[2] - off[1] >= 3 and int(rec["diagonal"].astype(np.int16).max()) >= 20000
    gpu.load_targets(*kc.pack(seqs + [kc.random_seq(rng, 32767)]), 21)
    with pytest.raises(capi.MMGpuError, match="32 767"):
        gpu.kmermatch(kc.identity_params())


def test_sixty_four_copies_of_one_sequence(gpu):
    """one group per k-mer, 64 records each; in the vote every (0, member) run is as long as a sequence's records"""
    rng = np.random.default_rng(4)
    s = kc.random_seq(rng, 200)
    off, rec = device_equals_restatement(gpu, [s.copy() for _ in range(64)], kc.identity_params(k=14))
    assert off[1] == 64 and rec["id"][:64].tolist() == list(range(64)) and len(set(rec["score"][1:64].tolist())) == 1 and rec["score"][1] > 10


def test_no_two_sequences_share_a_kmer(gpu):
    """every list a singleton: nothing is emitted, the compactions and the second sort see nothing"""
    rng = np.random.default_rng(5)
    seqs = [kc.random_seq(rng, n) for n in rng.integers(20, 200, 300)]
    par = kc.identity_params(k=14)
    gpu.load_targets(*kc.pack(seqs), 21)
    b = gpu.kmermatch_prepare(par)
    b.run()
    c = b.counts()
    got = b.fetch()
    b.free()
    assert c["n_pairs"] == 0 and c["n_entries"] == len(seqs) and c["n_records"] > len(seqs)
    assert_csr(got, kc.kmermatch(seqs, par))
    assert got[0].tolist() == list(range(len(seqs) + 1))


# ---- 3. the engineered cases -------------------------------------------------------------------------------------------------
def test_surplus_in_the_last_bin(gpu):
    """the threshold drops by one once the surplus is used up: the later windows of the last bin are not taken"""
    par = kc.identity_params(k=12, kmers_per_seq=300)
    s = kc.find_last_bin_sequence(par, seed=7)
    assert kc.last_bin_surplus(s, par) > 0
    rng = np.random.default_rng(8)
    seqs = [s, kc.mutate(rng, s, 0.01), s[100:].copy(), kc.random_seq(rng, 400)]
    for kps in (300, 250, 301):
        device_equals_restatement(gpu, seqs, dict(par, kmers_per_seq=kps), kps)


def test_two_diagonals_with_equal_counts(gpu):
    """the vote takes the last, i.e. the largest, of the diagonals that tie"""
    par = kc.identity_params(k=14)
    rep, member = kc.find_tied_family(par, seed=9)
    assert kc.tied_diagonal_pairs([rep, member], par) == [(0, 1)]
    off, rec = device_equals_restatement(gpu, [rep, member], par)
    diags = sorted(d for a, b, d in kc.group(kc.extract([rep, member], par), par) if (a, b) == (0, 1))
    assert int(rec[1]["id"]) == 1 and int(rec[1]["diagonal"].astype(np.int16)) == max(diags) != min(diags)


# ---- 4. lifecycle ------------------------------------------------------------------------------------------------------------
def test_repeat_run_reload_and_refusals(gpu):
    G = golden()
    par = G.params(G.settings[0])
    gpu.load_targets(*kc.pack(G.seqs), 21)
    b = gpu.kmermatch_prepare(par)
    with pytest.raises(capi.MMGpuError, match="has not been run"):
        b.fetch()
    b.run()
    first = b.fetch()
    b.run()
    assert_csr(b.fetch(), first)
    assert_csr(first, G.expected(0))
    total, stages = b.stage_ms()
    assert total > 0 and set(stages) == set(capi.KMERMATCH_STAGES) and all(v >= 0 for v in stages.values())
    c = b.counts()
    assert c["n_seqs"] == len(G.seqs) and c["n_entries"] == len(first[1]) and c["n_records"] >= c["n_pairs"] > 0
    gpu.load_targets(*kc.pack(G.seqs[:100]), 21)
    for call in (b.run, b.fetch, b.counts, b.stage_ms, lambda: b.rescore_prepare(G.g["mat_blosum62"], 0)):
        with pytest.raises(capi.MMGpuError, match="reloaded"):
            call()
    b.free()
    rng = np.random.default_rng(6)
    gpu.load_targets(rng.integers(0, 4, 400).astype(np.uint8), np.array([0, 200, 400], np.uint64), 5)
    with pytest.raises(capi.MMGpuError, match="protein sequences only"):
        gpu.kmermatch(par)
    gpu.load_targets(*kc.pack(G.seqs), 21)
    with pytest.raises(capi.MMGpuError, match="cov_mode"):
        gpu.kmermatch(dict(par, cov_mode=6))
    with pytest.raises(capi.MMGpuError, match="2\\^63"):
        gpu.kmermatch(dict(par, k=18))


# ---- 5. the hand-over to the ungapped rescoring ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [rc.HAMMING, rc.SUBSTITUTION, rc.ALIGNMENT])
def test_handover_records_equal_those_of_the_host_list(gpu, mode):
    G = golden()
    mat = G.g["mat_blosum62"]
    gpu.load_targets(*kc.pack(G.seqs), 21)
    b = gpu.kmermatch_prepare(G.params(G.settings[0]))
    b.run()
    off, hits = b.fetch()
    rb = b.rescore_prepare(mat, mode)
    rb.run()
    got = rb.fetch()
    rb.free()
    b.free()
    lists = [np.stack([hits["id"][int(off[q]):int(off[q + 1])].astype(np.int64), hits["diagonal"][int(off[q]):int(off[q + 1])].astype(np.int64)], axis=1)
             for q in range(len(G.seqs))]
    want = gpu.rescore_batch(mat, G.seqs, lists, mode)
    assert len(got) == len(want) == len(hits) and got.tobytes() == want.tobytes()
    assert (got["score"] > 0).sum() >= len(G.seqs)


@pytest.mark.parametrize("c", range(len(golden().chains)), ids=["%s_mode_%d" % (c["name"], c["rescore_mode"]) for c in golden().chains])
def test_linclust_prefilter_equals_the_recorded_chain(gpu, c):
    G = golden()
    chain = G.chains[c]
    gpu.load_targets(*kc.pack(G.seqs), 21)
    off, hits, lines = capi.linclust_prefilter(gpu, G.g["mat_blosum62"], G.params(G.settings[chain["setting"]]), chain["rescore_mode"],
                                               min_seq_id=chain["min_seq_id"], cov=chain["cov"])
    assert_csr((off, hits), G.expected(chain["setting"]))
    rc.assert_lines(lines, G.chain_expected(c), chain["rescore_mode"], chain["name"])
