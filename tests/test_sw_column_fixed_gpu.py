"""GPU parity (pytest -m gpu) at the shapes where the per-block head letters and the boundary row of the multi-tile bodies
(sw_kernel.hip: letter_block, boundary16) can go wrong: against the plain-C oracle - score, both ends, both starts and
`word`, bit for bit, with min_start_score = 0 so that every positive pair is scanned backwards too.

Letter blocks: a block is four columns, and the padding letter is put in per block, only from the block on that reaches past
the shortest target of the wavefront.  So: targets of every length mod 4, of less than one block and of exactly one and two
blocks, next to a long one, with halves of a group left empty; forward ends and reverse starts at every byte of a letter word,
and t_end < 3 (the reverse direction's clamped first word).  One query per single-tile kernel (R = 2, 16, 28).
Boundary row: stretches of 16 columns; targets whose lengths straddle every stretch boundary and the partial last stretch, in
lists of more than 8 so that the groups of a wavefront hold different column counts; two resident tiles, three rebuilt ones,
four tiles."""
import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from tests.test_sw_gpu import GO, GE, _check, _round_cb

pytestmark = pytest.mark.gpu

SINGLE_QLENS = [24, 250, 448]                 # R = 2, 16, 28
SINGLE_TLENS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 300]
MULTI_QLENS = [449, 1153, 1345]               # two tiles (resident), three tiles (rebuilt per tile), four tiles
MULTI_TLENS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100]


def _background(rng, n):
    return rng.choice(20, size=n, p=wl.BACKGROUND).astype(np.uint8)


def _cut_homolog(rng, q, n):
    """n residues of a homolog of q: a window of it, or (where the homolog is shorter) the homolog inside background."""
    h = wl.mutate(rng, q, 0.7)
    if len(h) >= n:
        a = int(rng.integers(0, len(h) - n + 1))
        return h[a:a + n].copy()
    t = _background(rng, n)
    a = int(rng.integers(0, n - len(h) + 1))
    t[a:a + len(h)] = h
    return t


def _query(rng, oracle, matrices, qlen):
    q = _background(rng, qlen)
    return q, _round_cb(oracle, matrices, q)


def _single_case(oracle, matrices, qlen):
    rng = np.random.default_rng(5100 + qlen)
    q, cb = _query(rng, oracle, matrices, qlen)
    tl = [_background(rng, n) for n in SINGLE_TLENS] + [_cut_homolog(rng, q, n) for n in SINGLE_TLENS]
    return q, cb, tl


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("qlen", SINGLE_QLENS)
def test_every_block_length_single_tile(gpu, oracle, matrices, qlen, mode):
    mat = matrices["blosum62_sw"]
    q, cb, tl = _single_case(oracle, matrices, qlen)
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    ids = np.random.default_rng(qlen).permutation(len(tl)).astype(np.uint32)
    out = gpu.sw_batch(mat, GO, GE, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=mode)
    _check(out, oracle, mat, q, cb, tres, toff, ids, mode == 1, "blocks q%d mode %d" % (qlen, mode))
    if mode == 1:
        assert (out["score"] > 0).sum() >= len(SINGLE_TLENS) // 2 and (out["t_start"] >= 0).any()


# ids into the targets of _single_case: 0 = 1 residue background, 14 = 300 background, 15 = 1 residue of the homolog, 29 = 300 homolog
SHORT_LISTS = [[29], [15], [14, 0], [29, 15], [0, 14], [29, 15, 0], [14, 0, 29], [29, 14, 0, 15, 1, 2, 4, 13, 16], [0, 15, 29, 1, 16, 3, 18, 14, 17]]


@pytest.mark.parametrize("qlen", SINGLE_QLENS)
def test_one_and_300_residues_in_one_group_and_empty_halves(gpu, oracle, matrices, qlen):
    """Lists of one, two, three and nine targets: the list is ordered by length, so the 300-residue target shares its group with
    a 1-residue one or with nothing, the last group of three has an empty half, and the ninth target sits alone in a second
    chunk - padding from block 0 in a half while the other still runs, and blocks without padding in the wavefront next to it."""
    mat = matrices["blosum62_sw"]
    q, cb, tl = _single_case(oracle, matrices, qlen)
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    queries = [dict(q=q, comp_bias=cb, targets=np.array(l, np.uint32), min_start_score=0) for l in SHORT_LISTS]
    out = gpu.sw_batch(mat, GO, GE, queries, mode=1)
    off = 0
    for k, l in enumerate(SHORT_LISTS):
        _check(out[off:off + len(l)], oracle, mat, q, cb, tres, toff, np.array(l, np.uint32), True, "short list %d q%d" % (k, qlen))
        off += len(l)
    assert off == len(out)


@pytest.mark.parametrize("qlen", SINGLE_QLENS)
def test_short_device_resident_lists(gpu, oracle, matrices, qlen):
    """The same short lists handed over on the device (mmgpu_sw_prepare_from_lists): the jobs are cut for the lists' stride and
    clipped to the counts inside the kernel, which leaves empty halves and empty chunks of its own."""
    import torch
    from mmseqs2_amd import capi
    mat = matrices["blosum62_sw"]
    q, cb, tl = _single_case(oracle, matrices, qlen)
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    lists = [[]] + SHORT_LISTS
    stride = 16
    hits = np.zeros((len(lists), stride), capi.PF_HIT_DTYPE)
    counts = np.array([len(l) for l in lists], np.uint32)
    for i, l in enumerate(lists):
        hits["id"][i, :len(l)] = l
        hits["score"][i, :len(l)] = 50
    d_hits = torch.from_numpy(hits.view(np.int32).reshape(len(lists), stride, 3).copy()).cuda()
    d_counts = torch.from_numpy(counts.astype(np.int32)).cuda()
    swq = [dict(q=q, comp_bias=cb, min_start_score=0) for _ in lists]
    b = gpu.sw_prepare_from_lists(mat, GO, GE, swq, d_hits.data_ptr(), d_counts.data_ptr(), stride, mode=1)
    b.run()
    out = b.fetch().reshape(len(lists), stride)
    for i, l in enumerate(lists):
        _check(out[i, :len(l)], oracle, mat, q, cb, tres, toff, np.array(l, np.uint32), True, "device list %d q%d" % (i, qlen))
        assert np.all(out[i, len(l):]["score"] == 0)
    b.free()
    del d_hits, d_counts


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("qlen", MULTI_QLENS)
def test_every_stretch_boundary_multi_tile(gpu, oracle, matrices, qlen, mode):
    rng = np.random.default_rng(5200 + qlen)
    mat = matrices["blosum62_sw"]
    q, cb = _query(rng, oracle, matrices, qlen)
    tl = [_background(rng, n) for n in MULTI_TLENS] + [_cut_homolog(rng, q, n) for n in (593, 600, 607, 16, 33, 48)]
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    ids = rng.permutation(len(tl)).astype(np.uint32)
    out = gpu.sw_batch(mat, GO, GE, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=mode)
    _check(out, oracle, mat, q, cb, tres, toff, ids, mode == 1, "stretches q%d mode %d" % (qlen, mode))
    if mode == 1:
        assert (out["score"] > 100).sum() >= 3 and (out["q_start"] >= 0).any()
