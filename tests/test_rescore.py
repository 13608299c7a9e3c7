"""Ungapped diagonal rescoring on the CPU: the C-ABI's new symbols; mmgpu_host_rescore_accept and capi's list building over the serial
restatement of tests/rescore_cases.py reproduce every list the stock binary's `rescorediagonal` recorded in tests/golden/rescore.npz;
the kernel's summary merge, restated, equals the serial walk under every split of a diagonal - the tie rules are where a parallel
form of that loop goes wrong; the ungapped E-value parameters give the recorded E-values and bit scores."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from mmseqs2_amd import capi, evalue
from tests import rescore_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mmgpu_rescore_prepare", "mmgpu_rescore_run", "mmgpu_rescore_fetch", "mmgpu_rescore_fetch_device", "mmgpu_rescore_last_kernel_ms",
               "mmgpu_rescore_free", "mmgpu_rescore_batch"]


@functools.lru_cache(maxsize=None)
def golden():
    return rc.Golden()


def test_symbols_declared_listed_exported_and_answered_by_the_client():
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmgpu_[a-z0-9_]+)\s*\(", hdr))
    L = capi.load_library()
    for sym in NEW_SYMBOLS + ["mmgpu_host_rescore_accept"]:
        assert sym in declared and sym in capi.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert {s for s in declared if s.startswith("mmgpu_rescore_")} == set(NEW_SYMBOLS)
    # a binary linked against the client library still resolves the batch's entry points; nothing of them crosses the socket
    client = ctypes.CDLL(os.path.join(os.path.dirname(capi.library_path()), "libmmgpu_client.so"))
    b = ctypes.c_void_p(1)
    assert client.mmgpu_rescore_prepare(None, None, None, 0, None, None, ctypes.byref(b)) == -4 and b.value is None
    assert client.mmgpu_rescore_run(None, None) == -4
    assert client.mmgpu_rescore_fetch(None, None, None) == -4
    assert client.mmgpu_rescore_fetch_device(None, None, None) == -4
    assert client.mmgpu_rescore_last_kernel_ms(None, None, None) == -4
    assert client.mmgpu_rescore_batch(None, None, None, 0, None, None, None) == -4
    client.mmgpu_rescore_free.restype = None
    client.mmgpu_rescore_free(None, None)


def test_mirrors_have_the_c_sizes(tmp_path):
    structs = [("mmgpu_rescore_params", ctypes.sizeof(capi.RescoreParams)), ("mmgpu_rescore_query", ctypes.sizeof(capi.RescoreQuery)),
               ("mmgpu_rescore_accept_params", ctypes.sizeof(capi.RescoreAcceptParams)), ("mmgpu_rescore_verdict", ctypes.sizeof(capi.RescoreVerdict)),
               ("mmgpu_rescore_pair", capi.RESCORE_PAIR_DTYPE.itemsize), ("mmgpu_rescore_hit", capi.RESCORE_HIT_DTYPE.itemsize)]
    last = [("mmgpu_rescore_accept_params", "score_per_col_thr", capi.RescoreAcceptParams.score_per_col_thr.offset),
            ("mmgpu_rescore_verdict", "t_end", capi.RescoreVerdict.t_end.offset), ("mmgpu_rescore_hit", "ident", capi.RESCORE_HIT_DTYPE.fields["ident"][1])]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmgpu.h"\nint main(void) {\n'
           + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in structs)
           + "".join('    printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, f, _ in last) + "    return 0;\n}\n")
    c = tmp_path / "sizes.c"
    c.write_text(src)
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    out = dict(l.split() for l in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    for n, size in structs:
        assert size == int(out[n]), (n, size, out[n])
    for n, f, off in last:
        assert off == int(out[n + "." + f]), (n, f)


# ---- the recording ----------------------------------------------------------------------------------------------------------------
def test_recording_holds_the_settings_and_the_awkward_entries():
    G = golden()
    have = {(s["mode"], s["e"], s["min_seq_id"], s["seq_id_mode"], s["cov"], s["cov_mode"], s["min_aln_len"], s["filter_hits"], s["sort_results"],
             s["backtrace"], s["same_db"]) for s in G.settings}
    for want in ([(0, 0.001, 0.0, m, 0.0, 0, 0, 0, 0, 0, 0) for m in (0, 1, 2)] + [(0, 0.001, 0.5, 0, 0.0, 0, 0, 0, 0, 0, 0), (0, 0.001, 0.9, 0, 0.0, 0, 0, 0, 0, 0, 0)]
                 + [(0, 0.001, 0.0, 0, 0.8, m, 0, 0, 0, 0, 0) for m in (0, 1, 2)] + [(1, e, 0.0, 0, 0.0, 0, 0, 0, 0, 0, 0) for e in (0.001, 10.0, 1e-10)]
                 + [(1, 0.001, 0.5, 0, 0.8, m, 0, 1, 0, 0, 0) for m in (0, 1)] + [(2, e, 0.0, 0, 0.0, 0, 0, 0, 0, 0, 0) for e in (0.001, 10.0, 1e-10)]
                 + [(2, 10.0, 0.0, 0, 0.0, 0, 30, 0, 0, 0, 0), (2, 10.0, 0.0, 0, 0.0, 0, 0, 0, 0, 1, 0), (2, 10.0, 0.0, 0, 0.0, 0, 0, 0, 1, 0, 0),
                    (2, 0.001, 0.0, 0, 0.0, 0, 0, 0, 0, 0, 1)]):
        assert want in have, want
    assert all(s["score_per_col_thr"] > 0 for s in G.settings if s["filter_hits"])
    assert [s["effective_mode"] for s in G.settings if s["name"] == "hamming_filter"] == [rc.SUBSTITUTION]
    s = G.settings[0]
    kept, rec = rc.golden_records(G, s)
    diag = np.concatenate([h[:, 1] for h in kept])
    qlen = np.concatenate([np.full(len(h), len(q)) for q, h in zip(G.queries, kept)])
    tlen = np.array([len(G.targets[t]) for t in np.concatenate([h[:, 0] for h in kept])])
    valid = ((diag & 0xFFFF) < qlen) | (65536 - (diag & 0xFFFF) < tlen)      # (no sequence of the recording is longer than 65536)
    assert (diag < 0).sum() > 50 and (~valid).sum() >= 10      # negative diagonals; diagonals valid for neither sign or one past an end
    assert ((rec["score"] == 0) & (rec["start"] == -1) & (rec["diagonal"] == 0) & (rec["diag_len"] == 0)).sum() == (rec["score"] == 0).sum() > (~valid).sum()
    assert not (rec["score"][~valid] != 0).any()
    assert (valid & (diag == qlen - 1)).sum() >= 5 and (valid & (diag == -(tlen - 1)) & (tlen > 1)).sum() >= 5      # the extreme valid ones
    assert (~valid & (diag == qlen)).sum() >= 5 and (~valid & (diag == -tlen)).sum() >= 5                          # one past each end
    for s in G.settings:      # a same-database list holds the query's own target, and no identity hit scores 0
        if s["same_db"]:
            kept, rec = rc.golden_records(G, s)
            own = np.concatenate([h[:, 0] == i for i, h in enumerate(kept)])
            assert own.sum() == len(G.queries) and (rec["score"][own] > 0).all()


@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_accept_and_list_building_reproduce_the_recorded_lists(k):
    G = golden()
    s = G.settings[k]
    tl = np.array([len(t) for t in G.setting_targets(s)], np.int64)
    kept, rec = rc.golden_records(G, s)
    got = capi.rescore_lists(rec, [len(q) for q in G.queries], kept, tl, int(tl.sum()), s["effective_mode"], identity=G.identity(s), **G.options(s))
    rc.assert_lines(got, G.expected(k), s["effective_mode"], s["name"])
    if s["effective_mode"] == rc.ALIGNMENT and s["filter_hits"]:      # a hit kept only by --filter-hits is written with seqId 0
        assert any(x[2] == 0.0 and x[3] > s["e"] for lines in got for x in lines)


def test_host_accept_equals_its_restatement():
    G = golden()
    n = 0
    for s in G.settings:
        tl = np.array([len(t) for t in G.setting_targets(s)], np.int64)
        kept, rec = rc.golden_records(G, s)
        opt = {k: v for k, v in G.options(s).items() if k not in ("sort_results", "backtrace")}
        at = 0
        for qi, hs in enumerate(kept):
            for target, _ in hs:
                r = rec[at]
                at += 1
                if r["score"] == 0 and s["effective_mode"] == rc.ALIGNMENT:
                    continue      # start = end = -1: the reference's coverage of that is unsigned wrap-around, not a behaviour to pin
                own = bool(s["same_db"]) and int(target) == qi
                ev = evalue.evalue(int(r["score"]), len(G.queries[qi]), int(tl.sum()), evalue.BLOSUM62_UNGAPPED)
                a = capi.host_rescore_accept(r, len(G.queries[qi]), int(tl[target]), own, ev, s["effective_mode"], **opt)
                b = rc.accept(r, len(G.queries[qi]), int(tl[target]), own, ev, s["effective_mode"], **opt)
                for f in a:
                    same = a[f] == b[f] or (isinstance(a[f], float) and np.isnan(a[f]) and np.isnan(b[f]))
                    assert same, (s["name"], qi, int(target), f, a, b)
                n += 1
    assert n > 5000
    L = capi.load_library()
    assert L.mmgpu_host_rescore_accept(None, 10, 10, 0, 0.0, None, None) == -1


def test_filter_hits_turns_hamming_into_substitution():
    assert capi.rescore_effective_mode(0, True) == 1 and capi.rescore_effective_mode(0, False) == 0
    assert capi.rescore_effective_mode(2, True) == 2 and capi.rescore_effective_mode(1, False) == 1


def test_ungapped_evalue_and_bit_score_equal_the_recorded_values():
    G = golden()
    assert evalue.BLOSUM62_UNGAPPED != evalue.BLOSUM62_11_1 and evalue.BLOSUM62_UNGAPPED[0] > evalue.BLOSUM62_11_1[0]
    n = 0
    for k, s in enumerate(G.settings):
        if s["effective_mode"] == rc.HAMMING:
            continue
        tl = np.array([len(t) for t in G.setting_targets(s)], np.int64)
        kept, rec = rc.golden_records(G, s)
        at = 0
        raw = []      # per query: (target, diagonal written) -> raw score
        for qi, hs in enumerate(kept):
            d = {}
            for target, _ in hs:
                r = rec[at]
                at += 1
                d.setdefault((int(target), ((int(r["diagonal"]) & 0xFFFF) ^ 0x8000) - 0x8000 if s["effective_mode"] == 1 else int(r["score"])), int(r["score"]))
            raw.append(d)
        for qi, lines in enumerate(G.expected(k)):
            for x in lines:
                if s["effective_mode"] == rc.SUBSTITUTION:
                    score = raw[qi][(x[0], x[2])]
                    assert int(evalue.bit_score(score, evalue.BLOSUM62_UNGAPPED) + 0.5) == x[1]
                else:
                    cand = [sc for (t, sc) in raw[qi] if t == x[0] and int(evalue.bit_score(sc, evalue.BLOSUM62_UNGAPPED) + 0.5) == x[1]]
                    assert cand, (s["name"], qi, x)
                    assert any(abs(evalue.evalue(sc, len(G.queries[qi]), int(tl.sum()), evalue.BLOSUM62_UNGAPPED) - x[3]) <= 1e-3 * x[3] for sc in cand), (s["name"], qi, x)
                n += 1
    assert n > 500
    # the gapped set would not give these numbers
    assert int(evalue.bit_score(50, evalue.BLOSUM62_11_1) + 0.5) != int(evalue.bit_score(50, evalue.BLOSUM62_UNGAPPED) + 0.5)


# ---- the summary merge --------------------------------------------------------------------------------------------------------------
def serial(cells):
    score, start, end = rc.walk([int(c) for c in cells])
    return score, start, end


def assert_every_split(cells, rng=None, random_splits=0):
    cells = [int(c) for c in cells]
    want = serial(cells)
    n = len(cells)
    assert rc.split_walk(cells, [])[:3] == want
    for cut in range(0, n + 1):      # (a cut at 0 or n: an empty run on one side)
        assert rc.split_walk(cells, [cut])[:3] == want, (cells, cut)
    for _ in range(random_splits):
        cuts = sorted(int(x) for x in rng.integers(0, n + 1, int(rng.integers(2, 9))))
        assert rc.split_walk(cells, cuts)[:3] == want, (cells, cuts)
    assert rc.split_walk(cells, list(range(1, n)))[:3] == want      # one cell per run
    assert rc.split_walk(cells, rc.lane_cuts(n))[:3] == want         # the kernel's own cuts


def test_combine_pins_the_tie_rules():
    rng = np.random.default_rng(31)
    seg = [5, -2, 4, 6]
    cases = [
        [3],                                         # length 1
        [-3], [0],
        [-1, -4, -2, -7],                            # all negative: nothing scores above 0
        [0, 0, 0],
        [2, -2] + seg,                               # a zero-sum stretch right before the best segment: the start moves behind it
        [4, -1, -3] + seg,                           # the prefix returns to its minimum exactly
        [-5, 1, -1, 2, -2] + seg + [-9, 1],          # several ties of the prefix minimum: the latest one starts the segment
        seg + [-20] + seg,                           # two equal maxima: the earlier one ends the alignment
        seg + [-13] + seg + [-13] + seg,
        [7, -7, 7, -7, 7],                           # equal maxima that each start on a minimum tie
        [3, -1, 1, -1, 1],                           # the maximum attained again later by the same segment going on
        [1, 1, -2, 1, 1, -2, 1, 1],
    ]
    for cells in cases:
        assert_every_split(cells, rng, 20)
    assert serial([2, -2] + seg) == (13, 2, 5) and serial(seg + [-20] + seg) == (13, 0, 3) and serial([-1, -4]) == (0, 0, 0)
    assert serial([3, -1, 1, -1, 1]) == (3, 0, 0) and serial([7, -7, 7, -7, 7]) == (7, 0, 0)


def test_combine_equals_the_serial_walk_on_random_diagonals():
    rng = np.random.default_rng(32)
    for n in list(range(1, 20)) + [63, 64, 65, 130, 257]:
        for lo, hi in ((-4, 5), (-1, 2), (-11, 12)):      # small ranges: many ties
            cells = rng.integers(lo, hi, n)
            assert_every_split(cells, rng, 6 if n < 70 else 2)
    cells = rng.integers(-3, 4, 40)      # matches are counted over all runs
    eq = rng.integers(0, 2, 40)
    assert rc.split_walk(cells, [7, 7, 19, 33], eq)[3] == int(eq.sum())


def test_combine_is_associative_on_the_summaries():
    rng = np.random.default_rng(33)
    for _ in range(200):
        cells = [int(c) for c in rng.integers(-2, 3, 12)]
        a, b = sorted(int(x) for x in rng.integers(0, 13, 2))
        A, B, C = rc.fold(cells, 0, a), rc.fold(cells, a, b), rc.fold(cells, b, 12)
        left, right = rc.combine(rc.combine(A, B), C), rc.combine(A, rc.combine(B, C))
        whole = rc.fold(cells, 0, 12)
        # (where nothing scores above 0 the positions of `best` are not read)
        cut = lambda S: S if S[5] > 0 else S[:5] + (S[5],) + S[8:]
        assert cut(left) == cut(right) == cut(whole), (cells, a, b)


def test_serial_restatement_on_small_cases():
    mat = golden().mat
    A, W = 0, int(np.argmax(np.diag(mat)[:20]))
    q = np.array([A, W, A, A, W], np.uint8)
    t = np.array([W, A, A, W, A, A], np.uint8)
    # diagonal 1: q[1:] against t: W A A W | W A A W A A
    assert rc.rescore_hit(q, t, 1, mat, 0) == (4, 1, 4, -1, -1, 4)
    assert rc.rescore_hit(q, t, 1, mat, 2)[:5] == (2 * int(mat[W, W]) + 2 * int(mat[A, A]), 1, 4, 0, 3)
    assert rc.rescore_hit(q, t, 1, mat, 1)[3:] == (-1, -1, 0)
    assert rc.rescore_hit(q, t, 5, mat, 0) == rc.DEFAULT_RECORD                  # one past the query's end
    assert rc.rescore_hit(q, t, 65536 - 6, mat, 0) == rc.DEFAULT_RECORD          # one past the target's end
    assert rc.rescore_hit(q, t, 65536 - 5, mat, 0) == (1, -5, 1, -1, -1, 1)      # q[0] = A against t[5] = A
    assert rc.rescore_hit(q, t, 4, mat, 0) == (1, 4, 1, -1, -1, 1)               # q[4] = W against t[0] = W
    assert rc.rescore_hit(q, np.array([5, 6, 7], np.uint8), 0, mat, 0) == rc.DEFAULT_RECORD      # valid, all mismatches
    assert rc.rescore_hit(np.array([A, A], np.uint8), np.array([W, W], np.uint8), 0, mat, 2) == rc.DEFAULT_RECORD      # valid, all negative
