"""GPU parity (pytest -m gpu) on both sides of the rule that decides which multi-tile jobs keep the profiles of all their tiles in
LDS (sw_multi_resident, mmgpu_internal.h): against the plain-C oracle - score, both ends, both starts and `word`, bit for bit.

With 21 letters and the default budget of 64 KB a query of two tiles is resident at any R, one of three tiles up to R = 24; three
tiles of R >= 25 and four or more tiles rebuild the profile per tile as before.  A resident job runs without a barrier in its chunk
loop and deals its chunks of 8 hits to the wavefronts as they finish; the others stay in step."""
import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from tests.test_sw_gpu import GO, GE, _check, _round_cb

pytestmark = pytest.mark.gpu


def _ragged_targets(rng, q, n, max_len):
    """n targets of 1 .. max_len residues, every third one a cut homolog of q."""
    tl = []
    for k in range(n):
        if k % 3 == 0:
            h = wl.mutate(rng, q, float(rng.uniform(0.3, 0.95)))
            a = int(rng.integers(0, len(h) // 2))
            tl.append(h[a:a + int(rng.integers(20, min(len(h), max_len)))])
        else:
            tl.append(rng.choice(20, size=int(rng.integers(1, max_len + 1)), p=wl.BACKGROUND).astype(np.uint8))
    tl[1] = tl[1][:1]          # the ends of the range are present whatever the draw
    if len(tl[2]) < max_len:
        tl[2] = rng.choice(20, size=max_len, p=wl.BACKGROUND).astype(np.uint8)
    return tl


def _query(rng, oracle, matrices, qlen):
    q = rng.choice(20, size=qlen, p=wl.BACKGROUND).astype(np.uint8)
    return q, _round_cb(oracle, matrices, q)


# qlen: tiles x rows per lane, resident?
#  896: 2 x R 28, the largest resident footprint (56 320 bytes of profiles)     yes
#  897: 3 x R 19                                                                yes
# 1152: 3 x R 24, the largest resident job of three tiles                       yes
# 1153: 3 x R 25                                                                no
# 1345: 4 tiles                                                                 no
@pytest.mark.parametrize("qlen", [896, 897, 1152, 1153, 1345])
def test_each_side_of_the_rule_vs_oracle(gpu, oracle, matrices, qlen):
    rng = np.random.default_rng(4100 + qlen)
    mat = matrices["blosum62_sw"]
    q, cb = _query(rng, oracle, matrices, qlen)
    tres, toff = wl.seqs_from_list(_ragged_targets(rng, q, 70, 1500))
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(70, dtype=np.uint32)
    out = gpu.sw_batch(mat, GO, GE, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=1)
    _check(out, oracle, mat, q, cb, tres, toff, ids, True, "resident%d" % qlen)


def test_score_and_end_only(gpu, oracle, matrices):
    """The forward-only kernel of the multi-tile group (mode 0) on the largest resident footprint."""
    rng = np.random.default_rng(4100 + 896)      # the inputs of the 896 case above
    mat = matrices["blosum62_sw"]
    q, cb = _query(rng, oracle, matrices, 896)
    tres, toff = wl.seqs_from_list(_ragged_targets(rng, q, 70, 1500))
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(70, dtype=np.uint32)
    out = gpu.sw_batch(mat, GO, GE, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=0)
    _check(out, oracle, mat, q, cb, tres, toff, ids, False, "resident896 mode 0")
    assert np.all(out["q_start"] == -1) and np.all(out["t_start"] == -1)


def test_resident_and_rebuilding_jobs_in_one_launch(gpu, oracle, matrices):
    """A 449-row query (2 x R 15, resident) and a 1400-row query (4 tiles, rebuilt per tile) in one batch: the launch's LDS is
    sized by the first, and the workgroups of the second take the other path inside the same kernel."""
    rng = np.random.default_rng(4200)
    mat = matrices["blosum62_sw"]
    qa, cba = _query(rng, oracle, matrices, 449)
    qb, cbb = _query(rng, oracle, matrices, 1400)
    tl = _ragged_targets(rng, qa, 35, 1500) + _ragged_targets(rng, qb, 35, 1500)
    tres, toff = wl.seqs_from_list(tl)
    gpu.load_targets(tres, toff, 21)
    ids = np.arange(70, dtype=np.uint32)
    queries = [dict(q=qa, comp_bias=cba, targets=ids, min_start_score=0), dict(q=qb, comp_bias=cbb, targets=ids[::-1].copy(), min_start_score=0)]
    out = gpu.sw_batch(mat, GO, GE, queries, mode=1).reshape(2, 70)
    _check(out[0], oracle, mat, qa, cba, tres, toff, queries[0]["targets"], True, "mixed449")
    _check(out[1], oracle, mat, qb, cbb, tres, toff, queries[1]["targets"], True, "mixed1400")


def test_chunks_dealt_over_several_rounds(gpu, oracle, matrices):
    """One 449-row query against 150 targets of 1 .. 800 residues: about 27 M cells, below the 60 M at which a job is cut, so one
    job of 19 chunks on four wavefronts - each wavefront comes back for a chunk several times - and the last chunk holds 6 hits."""
    rng = np.random.default_rng(4300)
    mat = matrices["blosum62_sw"]
    q, cb = _query(rng, oracle, matrices, 449)
    tres, toff = wl.seqs_from_list(_ragged_targets(rng, q, 150, 800))
    gpu.load_targets(tres, toff, 21)
    ids = rng.permutation(150).astype(np.uint32)
    out = gpu.sw_batch(mat, GO, GE, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0)], mode=1)
    _check(out, oracle, mat, q, cb, tres, toff, ids, True, "chunks449")
