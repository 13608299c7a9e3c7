"""CPU tests of the nucleotide alignment step away from gap 5/2, z-drop 40 and the stock matrix: the restatement
(oracle/nucl_oracle.c) and the kernel source on emulated lanes (nucl_core.h, nucl_wave.h through tests/nucl_emu.cpp) against
tests/golden/nucl_param_vectors.npz, which tests/golden/make_nucl_param_golden.py recorded from the real
BandedNucleotideAligner at every setting of tests/nucl_param_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import nucl_param_cases as npc
from tests import test_nucl_emu as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [s[0] for s in npc.NUCL_PARAM_SETS]


@pytest.fixture(scope="module")
def vectors():
    return npc.load_param_vectors()


def test_fixture_holds_every_setting_and_its_long_alignments(vectors):
    assert list(vectors) == KEYS
    mats = set()
    for key, go, ge, zdrop, mkey in npc.NUCL_PARAM_SETS:
        v = vectors[key]
        assert len(v["cases"]) == 120 and len(v["wrapped"]) == (72 if key in npc.WRAPPED_SETS else 0)
        assert bytes(v["serialized"]) == npc.serialized(mkey) and v["mat"].shape == (5, 5) and v["mat"].dtype == np.int8
        # the conditions the recorder asserted: real extensions, not only seeds, at every setting
        assert sum(len(c[7]) > 100 for c in v["cases"]) >= 8 and sum(len(c[7]) > 1000 for c in v["cases"]) >= 2, key
        assert {len(c[0]) for c in v["cases"]} >= set(npc.LENGTHS) and {c[3] for c in v["cases"]} == {0, 1}
        assert {c[4] for c in v["cases"]} == set(range(5)) == {c[5] for c in v["cases"]}
        mats.add(v["mat"].tobytes())
    assert len(mats) == 5
    m = vectors["transitions_5_2_z40"]["mat"]
    assert m[0, 3] != m[0, 1] and m[1, 2] != m[1, 0]                       # unequal off-diagonal entries
    assert vectors["x0_5_2_z40"]["mat"][0, 4] != vectors["x0_5_2_z40"]["mat"][0, 1]     # an N column that is not the mismatch
    assert os.path.getsize(npc.FIXTURE) < 300 * 1000


@pytest.mark.parametrize("key", KEYS)
def test_oracle_matches_param_vectors(vectors, key):
    v = vectors[key]
    orc = po.NuclOracle()
    for wrapped, cases in ((False, v["cases"]), (True, v["wrapped"])):
        for k, (q, t, diag, rev, pq, pt, exp, bt) in enumerate(cases):
            res, s = orc.align(q, t, v["mat"].reshape(-1), v["reverse"], v["go"], v["ge"], v["zdrop"], diag, rev, pq, pt, wrapped=wrapped)
            assert res == exp and s == bt, (key, wrapped, k, len(q), len(t), diag, rev, res, exp)


@pytest.mark.parametrize("lanes,wave", [(16, False), (64, True)])
@pytest.mark.parametrize("key", KEYS)
def test_kernel_source_on_emulated_lanes_matches_param_vectors(vectors, key, lanes, wave):
    v = vectors[key]
    L = te._lib(lanes, wave)
    for wrapped, cases in ((False, v["cases"]), (True, v["wrapped"])):
        if not cases:
            continue
        pairs = [(i, i, c[2], c[3], npc.past_end_byte(c[4], c[5])) for i, c in enumerate(cases)]
        hits, strs = te.emu_align(L, v["mat"], v["reverse"], [c[0] for c in cases], [c[1] for c in cases], pairs, 2, 1,
                                  v["go"], v["ge"], v["zdrop"], wrapped=wrapped)
        for k, (c, h, s) in enumerate(zip(cases, hits, strs)):
            assert h["status"] == 0 and npc.hit_tuple(h) == c[6][:6] and s == c[7], (key, wrapped, k, len(c[0]), len(c[1]), c[2], c[3],
                                                                                      npc.hit_tuple(h), c[6])


def test_lengths_around_the_lane_counts_on_both_emulated_forms():
    """Both forms count identities with every lane on a chunk of the string (nucl_core.h count_identities): queries and targets
    of 1 ... 65 letters give strings shorter than, as long as and just longer than 16 and 64 lanes - a mutated copy (substitutions,
    one deletion and one insertion, so that the chunks start behind gaps) and an unrelated sequence per pair of lengths, stock
    settings, all six result fields and the string against the restatement (oracle/nucl_oracle.c)."""
    from tests import nucl_common as nc
    g = nc.golden()
    mat, rl = np.asarray(g["mat"]).reshape(5, 5), np.asarray(g["reverse"])
    lengths = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65]
    rng = np.random.default_rng(77)
    queries, targets = [], []
    for qn in lengths:
        for tn in lengths:
            base = rng.integers(0, 4, size=max(qn, tn)).astype(np.uint8)
            copy = np.where(rng.random(tn) < 0.08, rng.integers(0, 4, size=tn), base[:tn]).astype(np.uint8)
            if tn >= 15:      # one letter out, one in: the length stays
                copy = np.concatenate([copy[:tn // 3], copy[tn // 3 + 1:2 * tn // 3], rng.integers(0, 4, size=1), copy[2 * tn // 3:]]).astype(np.uint8)
            for t in (copy, rng.integers(0, 4, size=tn).astype(np.uint8)):
                queries.append(base[:qn].copy())
                targets.append(t)
    assert {(len(q), len(t)) for q, t in zip(queries, targets)} == {(a, b) for a in lengths for b in lengths}
    pairs = [(i, i, 0, 0) for i in range(len(queries))]
    orc = po.NuclOracle()
    expected = [orc.align(q, t, mat.reshape(-1), rl, 5, 2, 40, 0, 0, 4, 4) for q, t in zip(queries, targets)]
    assert {len(e[1]) for e in expected} >= {1, 2, 15, 16, 17, 63, 64, 65} and sum("I" in e[1] or "D" in e[1] for e in expected) >= 10
    for lanes, wave in ((16, False), (64, True)):
        hits, strs = te.emu_align(te._lib(lanes, wave), mat, rl, queries, targets, pairs, 4, 4)
        for k, (e, h, s) in enumerate(zip(expected, hits, strs)):
            assert h["status"] == 0 and npc.hit_tuple(h) == e[0][:6] and s == e[1], (lanes, k, len(queries[k]), len(targets[k]),
                                                                                  npc.hit_tuple(h), e[0], s, e[1])


def test_emulator_ucontext_fallback_matches_param_vectors(vectors):
    """tests/nucl_emu.cpp switches lanes with its own stack switch on x86-64 and with ucontext elsewhere (-DEMU_UCONTEXT forces
    it): the fallback is built here and gives the recorded results too (the short cases of one setting: it is ten times slower)"""
    import ctypes
    so = os.path.join(ROOT, "tests", "_build", "libnuclemu64w_ucontext.so")
    src = os.path.join(ROOT, "tests", "nucl_emu.cpp")
    deps = [src] + [os.path.join(ROOT, "mmseqs2_amd", "csrc", f) for f in ("nucl_core.h", "nucl_wave.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-DEMU_LANES=64", "-DEMU_WAVE", "-DEMU_UCONTEXT",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mmseqs2_amd", "csrc"), src, "-o", so])
    v = vectors["stock_10_1_z40"]
    cases = [c for c in v["cases"] if len(c[0]) + len(c[1]) <= 500]
    assert len(cases) >= 60 and sum(len(c[7]) > 100 for c in cases) >= 2
    pairs = [(i, i, c[2], c[3], npc.past_end_byte(c[4], c[5])) for i, c in enumerate(cases)]
    hits, strs = te.emu_align(ctypes.CDLL(so), v["mat"], v["reverse"], [c[0] for c in cases], [c[1] for c in cases], pairs, 2, 1,
                              v["go"], v["ge"], v["zdrop"])
    for k, (c, h, s) in enumerate(zip(cases, hits, strs)):
        assert npc.hit_tuple(h) == c[6][:6] and s == c[7], (k, npc.hit_tuple(h), c[6])


def test_param_vectors_are_consistent(vectors):
    """size-independent properties of the recorded alignments (tests/test_nucl_oracle.py test_golden_vectors_are_consistent): the
    backtrace spans exactly the reported rectangle and the identity count is what the string says"""
    n = 0
    for key, v in vectors.items():
        rl = v["reverse"]
        for q, t, diag, rev, pq, pt, exp, bt in v["cases"]:
            score, qs, qe, ts, te_, ident = exp[:6]
            if not bt:
                continue
            assert bt.count("M") + bt.count("I") == qe - qs + 1, key
            assert bt.count("M") + bt.count("D") == te_ - ts + 1, key
            qa = npc.revcomp(q, rl) if rev else q
            qp, tp, ids = qs, ts, 0
            for c in bt:
                if c == "M":
                    ids += int(qa[qp] == t[tp])
                    qp += 1
                    tp += 1
                elif c == "I":
                    qp += 1
                else:
                    tp += 1
            assert ids == ident, key
            n += 1
    assert n >= 400          # the identical pairs alone (40 per setting) all have a string


@pytest.mark.skipif(not (po.ref_available() and po.ref_matrix_available()), reason="needs oracle/_ref and /root/reference/data")
def test_recorder_reproduces_one_setting(vectors, tmp_path):
    """one setting recorded again from the real reference, in a child process as the recorder itself does it"""
    key = "transitions_5_2_z40"
    out = str(tmp_path / "one.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_nucl_param_golden.py"), "--setting", key, "--out", out],
                   check=True, cwd=ROOT, stdout=subprocess.PIPE, timeout=300)
    again, committed = np.load(out), np.load(npc.FIXTURE)
    names = [n for n in committed.files if n.startswith(key + "/")]
    assert sorted(again.files) == sorted(names) and len(names) == 12
    for n in names:
        assert again[n].dtype == committed[n].dtype and np.array_equal(again[n], committed[n]), n
