"""GPU parity (pytest -m gpu) of the f16 forward scan of the single-tile kernels (sw_half_kernel.hip) around its overflow
limit, against the plain-C oracle: score, both ends, both starts and `word`, bit for bit, through gpu.sw_batch in modes 0 and 1
(whatever kernels the default dispatch picks for them).

The f16 scan is exact up to a score of LIMIT = 2048 - 256 = 1792; a pair that scores more is marked and scanned again in int16
by the workgroup that found it (sw_body.h).  So: one query per register group (100, 300 and 440 residues: R = 7, 19, 28), with
composition bias zero so that a target's score can be engineered - a prefix of the query scores the sum of its diagonal entries,
and substitutions take it down to the value wanted.  About 40 targets per query, whose scores step through LIMIT - 3 .. LIMIT + 3,
through 2047, 2048 and 2049, and up to the query's self-score (the test asserts that the oracle's scores hold these values).

The host sorts a list by target length, so targets with neighbouring scores are neighbours in a wavefront: with the whole list and
the list without its longest target, LIMIT and LIMIT + 1 share a 16-lane group (its lo and hi halves) in one of the two and sit
in neighbouring groups of one wavefront in the other.  Further lists hold no pair above the limit (the workgroup's flag stays
down) and exactly one.

BLOSUM62 cannot take 100 residues past 1100, so the 100-residue query runs with 4 x BLOSUM62 plus a small symmetric perturbation
(which also gives substitutions of every size mod 4).  No matrix of tests/sw_param_cases.py has entries near +-127; its widest,
PAM30 25/2, is scaled by 7 here (entries -119 .. 91, gap costs 175 / 14), and a profile query gets rows of 11 x BLOSUM62
(-44 .. 121): their scores are multiples of large steps, so these two cases straddle the limits with consecutive prefixes instead
of exact values."""
import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from tests import sw_param_cases as pc

pytestmark = pytest.mark.gpu

LIMIT = 2048 - 256
WANTED = list(range(LIMIT - 3, LIMIT + 4)) + [2047, 2048, 2049]
FIELDS = ("score", "q_end", "t_end", "q_start", "t_start", "word")
RICH = {"W": 0.25, "C": 0.25, "H": 0.125, "Y": 0.125, "P": 0.125, "I": 0.125}     # BLOSUM62 diagonal 11, 9, 8, 7, 7, 4


def _rich_query(rng, matrices, n):
    aa = [chr(c) for c in matrices["num2aa"]]
    return rng.choice([aa.index(k) for k in RICH], size=n, p=list(RICH.values())).astype(np.uint8)


def _engineered(q, mat, values):
    """a target per value: a prefix of q whose self-score reaches it, with substitutions that take off the excess"""
    m = mat.astype(int)
    S = np.concatenate([[0], np.cumsum(m[q, q])])
    out = []
    for v in values:
        n0 = int(np.searchsorted(S, v))
        assert n0 < len(S), "the query's self-score %d does not reach %d" % (S[-1], v)
        for n in range(n0, min(n0 + 4, len(q)) + 1):       # a longer prefix where no set of substitutions takes off the excess exactly
            t, excess = q[:n].copy(), int(S[n]) - v
            reach = {0: []}              # sum taken off -> [(position, letter)], at most one substitution per position
            for pos in range(4, n - 4):
                if excess in reach:
                    break
                a = int(q[pos])
                for s0, path in list(reach.items()):
                    for b in range(20):
                        d = m[a, a] - m[a, b]
                        if d > 0 and s0 + d <= excess and s0 + d not in reach:
                            reach[s0 + d] = path + [(pos, b)]
            if excess in reach:
                break
        for pos, b in reach.get(excess, []):
            t[pos] = b
        out.append(t)
    return out


def _case(matrices, name):
    """-> dict(mat, go, ge, q, profile or None, targets)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    b62 = matrices["blosum62_sw"]
    if name in ("q100", "q300", "q440"):
        n = int(name[1:])
        mat, go, ge = b62, 11, 1
        if n == 100:
            J = np.triu(rng.integers(0, 4, (21, 21)), 1)
            mat, go, ge = (4 * b62.astype(int) + J + J.T).astype(np.int8), 44, 4
        q = _rich_query(rng, matrices, n) if n != 440 else rng.choice(20, size=n, p=wl.BACKGROUND).astype(np.uint8)
        S = np.concatenate([[0], np.cumsum(mat.astype(int)[q, q])])
        prefixes = sorted(set(np.linspace(1, n, 30).astype(int).tolist()))
        return dict(mat=mat, go=go, ge=ge, q=q, profile=None, targets=_engineered(q, mat, WANTED) + [q[:k].copy() for k in prefixes], S=S)
    n = 300
    if name == "pam30x7":
        mat, go, ge = (7 * pc.load_param_vectors()["pam30_25_2"]["mat"].astype(int)).astype(np.int8), 175, 14
        q = rng.choice(20, size=n, p=wl.BACKGROUND).astype(np.uint8)
        prof, S = None, np.concatenate([[0], np.cumsum(mat.astype(int)[q, q])])
    else:
        assert name == "profile"
        mat, go, ge = b62, 130, 12
        q = rng.choice(20, size=n, p=wl.BACKGROUND).astype(np.uint8)
        prof = (11 * b62.astype(int))[:20, q].astype(np.int8)            # [letter][position]
        S = np.concatenate([[0], np.cumsum(prof.astype(int)[q, np.arange(n)])])
    around = []
    for v in (LIMIT, 2048):            # consecutive prefixes on either side of the limit and of 2048
        k = int(np.searchsorted(S, v))
        around += list(range(max(k - 8, 1), min(k + 5, n) + 1))
    prefixes = sorted(set(around + np.linspace(1, n, 16).astype(int).tolist()))
    return dict(mat=mat, go=go, ge=ge, q=q, profile=prof, targets=[q[:k].copy() for k in prefixes], S=S)


_CACHE = {}


def _case_with_expectation(oracle, matrices, name):
    """the case and the oracle's record of every target (with start positions), computed once per case"""
    if name not in _CACHE:
        c = _case(matrices, name)
        cb = np.zeros(len(c["q"]), np.int8)
        exp = []
        for t in c["targets"]:
            if c["profile"] is None:
                r = oracle.sw_align(c["q"], cb, t, c["mat"], c["go"], c["ge"], need_start=True)
            else:
                r = oracle.sw_align_profile(c["profile"], c["q"], t, 21, c["go"], c["ge"], need_start=True)
            exp.append(tuple(int(r[f]) for f in FIELDS))
        c["cb"], c["exp"] = cb, exp
        _CACHE[name] = c
    return _CACHE[name]


def _lists(c):
    """id lists: everything; everything but the longest target (the other lo / hi pairing); nothing above the limit; exactly one"""
    score = np.array([e[0] for e in c["exp"]])
    ids = np.arange(len(score), dtype=np.uint32)
    longest = int(np.argmax([len(t) for t in c["targets"]]))
    under, over = ids[score <= LIMIT], ids[score > LIMIT]
    assert len(under) >= 8 and len(over) >= 5
    just_over = over[np.argmin(score[over])]
    return [ids, ids[ids != longest], under, np.append(under[::2], just_over).astype(np.uint32), over]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", ["q100", "q300", "q440", "pam30x7", "profile"])
def test_scores_around_the_f16_limit(gpu, oracle, matrices, name, mode):
    c = _case_with_expectation(oracle, matrices, name)
    score = sorted(e[0] for e in c["exp"])
    if name.startswith("q"):
        assert set(WANTED) <= set(score), "engineered scores missing: %s" % sorted(set(WANTED) - set(score))
    else:
        assert sum(s <= LIMIT for s in score) >= 5 and sum(LIMIT < s < 2048 for s in score) >= 1 and sum(s > 2048 for s in score) >= 5
    assert score[-1] == int(c["S"][-1]) and score[-1] > 2049            # the self-score
    tres, toff = wl.seqs_from_list(c["targets"])
    gpu.load_targets(tres, toff, 21)
    lists = _lists(c)
    queries = [dict(q=c["q"], comp_bias=c["cb"] if c["profile"] is None else None, targets=l, min_start_score=0) for l in lists]
    if c["profile"] is not None:
        for qd in queries:
            qd["profile"] = c["profile"]
    out = gpu.sw_batch(c["mat"], c["go"], c["ge"], queries, mode=mode)
    off = 0
    for li, l in enumerate(lists):
        for k, tid in enumerate(l):
            got = tuple(int(out[off + k][f]) for f in FIELDS)
            exp = c["exp"][int(tid)]
            if mode == 0 or exp[0] == 0:
                exp = exp[:3] + (-1, -1) + exp[5:]
            assert got == exp, (name, mode, li, k, int(tid), got, exp)
        off += len(l)
    assert off == len(out)
