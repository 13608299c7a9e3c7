"""GPU tests of linclust's k-mer matching stage over nucleotides (mmgpu_nuclmatch_*): the device's CSR against the lists recorded from
the stock binary (tests/golden/nuclmatch.npz), byte for byte, and against the serial restatement (tests/nuclmatch_cases.py) on
generated databases the fixture cannot hold; the edges; the lifecycle and the refusals.  Everything is integers and is compared
exactly."""
import functools

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import kmermatch_cases as kc
from tests import nuclmatch_cases as nc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    return nc.Golden()


def assert_csr(got, want, tag=""):
    (off, rec), (want_off, want_rec) = got, want
    assert off.dtype == np.uint64 and rec.dtype == nc.HIT_DTYPE
    bad = np.flatnonzero(off != want_off)
    assert len(bad) == 0, (tag, "offsets", bad[:5], off[bad[:5]], want_off[bad[:5]])
    bad = np.flatnonzero(rec != want_rec)
    assert len(bad) == 0, (tag, "records", [(int(k), rec[k].tolist(), want_rec[k].tolist()) for k in bad[:5]])
    assert off.tobytes() == want_off.tobytes() and rec.tobytes() == want_rec.tobytes(), tag


def device_equals_restatement(gpu, seqs, par, tag=""):
    gpu.load_targets(*nc.pack(seqs), 5)
    got = gpu.nuclmatch(par)
    assert_csr(got, nc.nuclmatch(seqs, par), tag)
    return got


# ---- 1. the recorded lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_device_lists_equal_the_recorded_lists(gpu, k):
    G = golden()
    gpu.load_targets(*nc.pack(G.seqs), 5)
    assert_csr(gpu.nuclmatch(G.params(G.settings[k])), G.expected(k), G.settings[k]["name"])


# ---- 2. generated databases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
def test_lognormal_database(gpu, seed):
    """2 000 sequences, a third of them copies and half of those reverse-complemented: more than one tile of every scan, sequences
    shorter than k, windows with N.  The seeds are ones without a strand tie, so every list is compared"""
    seqs = nc.lognormal_database(seed)
    par = nc.params(k=17, kmers_per_seq=60, scale=0.2 if seed == 12 else 0.0)
    assert nc.strand_ties(seqs, par) == []
    off, rec = device_equals_restatement(gpu, seqs, par)
    assert len(rec) > len(seqs) + 300 and (rec["score"] < 0).sum() > 100 and min(len(s) for s in seqs) < 17 and max(len(s) for s in seqs) > 500


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def longest_database():
    rng = np.random.default_rng(3)
    long_seq = nc.random_seq(rng, 32766)
    return [nc.random_seq(rng, 100), long_seq, nc.mutate(rng, long_seq, 0.02)[7:20000], nc.revcomp(nc.mutate(rng, long_seq, 0.02)[20000:]),
            nc.revcomp(long_seq[-50:]), nc.mutate(rng, long_seq, 0.01)[24000:32000],
            np.concatenate([nc.random_seq(rng, 25000), nc.mutate(rng, long_seq, 0.01)[:5000]])]      # its k-mers lie 25 000 further in than the representative's


@pytest.mark.parametrize("k", [17, 31])
def test_longest_admitted_sequence(gpu, k):
    """32 766 residues with forward and reverse-complemented pieces of it: positions and lengths at the end of their 15 bits, both
    histogram levels of the selection, diagonals beyond +-20 000"""
    seqs = longest_database()
    off, rec = device_equals_restatement(gpu, seqs, nc.params(k=k, kmers_per_seq=60, scale=0.2, cov_thr=0.001))
    diag = rec["diagonal"].astype(np.int16)
    assert off[2] - off[1] >= 6 and int(diag.max()) >= 20000 and int(diag.min()) <= -20000 and (rec["score"] < 0).sum() >= 2


def test_sequence_of_32767_residues_is_refused(gpu):
    rng = np.random.default_rng(5)
    gpu.load_targets(*nc.pack([nc.random_seq(rng, 100), nc.random_seq(rng, 32767)]), 5)
    with pytest.raises(capi.MMGpuError, match="32 767"):
        gpu.nuclmatch(nc.params())


def test_sixty_four_copies_of_one_sequence(gpu):
    """one group per k-mer, 64 records each, half of them on the other strand"""
    rng = np.random.default_rng(4)
    s = nc.random_seq(rng, 300)
    seqs = [s.copy() if i % 2 == 0 else nc.revcomp(s) for i in range(64)]
    off, rec = device_equals_restatement(gpu, seqs, nc.params(k=17))
    assert off[1] == 64 and rec["id"][:64].tolist() == list(range(64))
    assert set(rec["score"][1:64:2].tolist()) == {int(rec["score"][1])} and rec["score"][1] < -10 and set(rec["score"][2:64:2].tolist()) == {0}


def test_all_sequences_shorter_than_k(gpu):
    """identity records only: duplicates meet, nothing else does"""
    rng = np.random.default_rng(6)
    seqs = [nc.random_seq(rng, n) for n in rng.integers(1, 17, 200)]
    seqs += [seqs[3].copy(), seqs[10].copy(), nc.revcomp(seqs[20])]
    par = nc.params(k=17)
    gpu.load_targets(*nc.pack(seqs), 5)
    b = gpu.nuclmatch_prepare(par)
    b.run()
    c = b.counts()
    got = b.fetch()
    b.free()
    assert c["n_records"] == len(seqs) and c["n_entries"] >= len(seqs) + 2
    assert_csr(got, nc.nuclmatch(seqs, par))


def test_database_of_n(gpu):
    seqs = [np.full(n, nc.N, np.uint8) for n in (5, 17, 64, 100, 100, 300)]
    off, rec = device_equals_restatement(gpu, seqs, nc.params(k=17))
    assert off[-1] == len(seqs) + 1 and rec[int(off[3]) + 1].tolist()[:3] == (4, 0, 0)      # the two of 100 meet through the identity record: same hash, same bit 63, so the run starts as-it-is


def test_sequence_followed_by_its_reverse_complement(gpu):
    """NOT reference parity: in S + revcomp(S) every window ties with its own reverse strand under the reference's comparator, whose
    order between the two is unspecified.  Held against the documented rule only: such records keep the order they were born in"""
    rng = np.random.default_rng(7)
    s = nc.random_seq(rng, 200)
    hairpin = np.concatenate([s, nc.revcomp(s)])
    seqs = [hairpin, nc.mutate(rng, hairpin, 0.02)[5:380], nc.revcomp(nc.mutate(rng, hairpin, 0.02)[10:390])]
    par = nc.params(k=17, cov_thr=0.5)
    assert len(nc.strand_ties(seqs, par)) > 20
    off, rec = device_equals_restatement(gpu, seqs, par)
    assert off[1] == 3


# ---- 4. lifecycle and refusals -----------------------------------------------------------------------------------------------
def test_repeat_run_reload_and_refusals(gpu):
    import torch
    G = golden()
    par = G.params(G.settings[0])
    gpu.load_targets(*nc.pack(G.seqs), 5)
    b = gpu.nuclmatch_prepare(par)
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
    d_off = torch.zeros(len(G.seqs) + 1, dtype=torch.int64, device="cuda")
    d_rec = torch.zeros((c["n_entries"], 3), dtype=torch.int32, device="cuda")
    b.fetch_device(d_off.data_ptr(), d_rec.data_ptr())
    gpu.synchronize()
    assert d_off.cpu().numpy().tobytes() == first[0].tobytes() and d_rec.cpu().numpy().tobytes() == first[1].tobytes()
    gpu.load_targets(*nc.pack(G.seqs[:100]), 5)
    for call in (b.run, b.fetch, b.counts, b.stage_ms):
        with pytest.raises(capi.MMGpuError, match="reloaded"):
            call()
    b.free()
    rng = np.random.default_rng(6)
    gpu.load_targets(*kc.pack([kc.random_seq(rng, 200), kc.random_seq(rng, 200)]), 21)
    with pytest.raises(capi.MMGpuError, match="nucleotide sequences only"):
        gpu.nuclmatch(par)
    gpu.load_targets(*nc.pack(G.seqs), 5)
    with pytest.raises(capi.MMGpuError, match="cov_mode 1"):
        gpu.nuclmatch(dict(par, cov_mode=1))
    with pytest.raises(capi.MMGpuError, match="k must be"):
        gpu.nuclmatch(dict(par, k=32))
