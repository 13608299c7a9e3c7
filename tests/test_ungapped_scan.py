"""CPU tests of the exhaustive ungapped scan (mmgpu_scan_*, `mmseqs ungappedprefilter`): the C-ABI's new symbols, the numpy
restatement (tests/ungapped_scan_cases.py) against the lists recorded from the stock binary (tests/golden/ungapped_scan.npz),
the coverage window against the reference's predicate per target, the flat descriptor layout."""
import ctypes
import os
import re

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import ungapped_scan_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mmgpu_scan_prepare", "mmgpu_scan_run", "mmgpu_scan_fetch", "mmgpu_scan_fetch_device", "mmgpu_scan_last_kernel_ms",
               "mmgpu_scan_free", "mmgpu_scan_batch", "mmgpu_scan_debug_scores")


@pytest.fixture(scope="module")
def G():
    return uc.Golden()


@pytest.fixture(scope="module")
def all_scores(G):
    """(matrix, comp_bias, same_db) -> uint8 [queries][targets], computed once"""
    out = {}
    for s in G.settings:
        key = (s["matrix"], s["comp_bias"], s["same_db"])
        if key not in out:
            out[key] = np.stack([uc.scores_one_query(G.mat(s), qd["q"], qd["comp_bias"], G.setting_targets(s)) for qd in G.setting_queries(s)])
    return out


def test_scan_symbols_declared_listed_exported_and_answered_by_the_client():
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmgpu_[a-z0-9_]+)\s*\(", hdr))
    L = capi.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in capi.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert {s for s in declared if s.startswith("mmgpu_scan_")} == set(NEW_SYMBOLS)
    # a binary linked against the client library still resolves the whole header; nothing of the scan crosses the socket
    client = ctypes.CDLL(os.path.join(os.path.dirname(capi.library_path()), "libmmgpu_client.so"))
    b = ctypes.c_void_p(1)
    assert client.mmgpu_scan_prepare(None, None, None, 0, ctypes.byref(b)) == -4 and b.value is None
    assert client.mmgpu_scan_run(None, None) == -4
    assert client.mmgpu_scan_fetch(None, None, None, 0, None) == -4
    assert client.mmgpu_scan_fetch_device(None, None, None, 0, None) == -4
    assert client.mmgpu_scan_last_kernel_ms(None, None, None) == -4
    assert client.mmgpu_scan_batch(None, None, None, 0, None, 0, None) == -4
    assert client.mmgpu_scan_debug_scores(None, None, 0, None, 0) == -4
    client.mmgpu_scan_free.restype = None
    client.mmgpu_scan_free(None, None)


def test_recording_is_worth_keeping(G):
    """saturated pairs, lists cut inside a score class, an identity entry at or below the threshold, an empty list, a target dropped
    by a coverage setting - and the settings the issue names"""
    shown = uc.check_recording(G)
    assert shown["saturated"] >= 8 and shown["cut_in_class"] >= 3
    have = {(s["matrix"], s["comp_bias"], s["min_score"], s["max_seqs"], s["cov"], s["cov_mode"], s["same_db"]) for s in G.settings}
    for want in [("blosum62", 1, 15, 300, 0.0, 0, 0), ("blosum62", 0, 15, 300, 0.0, 0, 0), ("blosum62", 1, 60, 300, 0.0, 0, 0),
                 ("blosum62", 1, 0, 300, 0.0, 0, 0), ("blosum62", 1, 15, 10, 0.0, 0, 0), ("blosum62", 1, 15, 1000, 0.0, 0, 0),
                 ("blosum62", 1, 15, 300, 0.8, 0, 0), ("blosum62", 1, 15, 300, 0.8, 1, 0), ("blosum62", 1, 15, 300, 0.8, 2, 0)]:
        assert want in have, want
    assert any(s["same_db"] for s in G.settings) and any(s["matrix"] != "blosum62" for s in G.settings)
    assert max(s["max_seqs"] for s in G.settings) > len(G.targets)


def test_restatement_equals_every_recorded_list(G, all_scores):
    """ids and scores, at every setting.  Where they differ the restatement is wrong, not the file."""
    for k, s in enumerate(G.settings):
        sc = all_scores[(s["matrix"], s["comp_bias"], s["same_db"])]
        qs = G.setting_queries(s)
        for qi, (ids, scores) in enumerate(G.expected(k)):
            win = uc.float32_window(s["cov"], s["cov_mode"], len(qs[qi]["q"]), G.setting_tlens(s))
            gi, gs = uc.select_list(sc[qi], G.setting_tlens(s), win, s["min_score"], s["max_seqs"], qs[qi]["identity_id"])
            assert np.array_equal(gi, ids) and np.array_equal(gs, scores), (s["name"], qi)


def test_vector_form_equals_the_cell_recurrence(G):
    """the restatement's all-targets-at-once form against the recurrence written cell by cell, saturated pairs included"""
    s = G.settings[0]
    qs = G.setting_queries(s)
    picks = [(4, 10), (4, 11), (7, 13), (0, 100), (2, 40), (3, 110), (5, 111), (1, 105)]
    for qi, ti in picks:
        a = int(uc.scores_one_query(G.mat(s), qs[qi]["q"], qs[qi]["comp_bias"], [G.targets[ti]])[0])
        assert a == uc.pair_score_cells(G.mat(s), qs[qi]["q"], qs[qi]["comp_bias"], G.targets[ti]), (qi, ti)
    assert int(uc.scores_one_query(G.mat(s), qs[0]["q"], None, [np.zeros(0, np.uint8)])[0]) == 0


@pytest.mark.parametrize("cov_mode", [0, 1, 2, 3, 4, 5])
def test_coverage_window_is_the_predicate_per_target(cov_mode):
    """all six modes, thresholds 0, 0.5, 0.8 and 1.0, lengths 1 to 2000: the admitted set is one interval and the window names it"""
    tl = np.arange(1, 2001)
    for thr in (0.0, 0.5, 0.8, 1.0):
        for qlen in (1, 2, 3, 7, 10, 99, 100, 101, 333, 1000, 1999, 2000, 3001):
            ok = np.array([uc.can_be_covered(thr, cov_mode, qlen, int(t)) for t in tl])      # the test module's own restatement
            lo, hi = capi.coverage_window(thr, cov_mode, qlen, tl)      # raises if the set is not one interval
            assert np.array_equal(ok, (tl >= lo) & (tl <= hi)), (thr, qlen)
            # a database that holds only some of the lengths: the window admits exactly the admitted ones among those present
            sub = tl[::7]
            lo, hi = capi.coverage_window(thr, cov_mode, qlen, sub)
            assert np.array_equal(ok[::7], (sub >= lo) & (sub <= hi))
            if thr == 0.0 and cov_mode not in (3, 4):
                assert (lo, hi) == (0, 0xFFFFFFFF)


def test_predicate_is_float32_like_the_reference():
    """Util::canBeCovered divides and compares floats: 4 / 5 against 0.8 is decided in float32 (where both round to the same
    number), not in double (where float32(0.8) lies above 4 / 5)"""
    for q, t in [(4, 5), (8, 10), (80, 100), (400, 500), (5, 4)]:
        want = (np.float32(q) / np.float32(t)) >= np.float32(0.8)
        assert bool(capi._can_be_covered(0.8, 1, q, np.array([t]))[0]) == bool(want)


def test_flat_scan_descriptor_matches_the_struct_layout(tmp_path):
    import subprocess
    dt, st = capi.SCAN_QUERY_DTYPE, capi.ScanQuery
    assert dt.itemsize == ctypes.sizeof(st)
    for name, _ in st._fields_:
        assert dt.fields[name][1] == getattr(st, name).offset, name
    # ... and both have the C compiler's layout
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmgpu.h"\nint main(void) {\n'
           '    printf("%zu %zu %zu %zu\\n", sizeof(mmgpu_scan_params), sizeof(mmgpu_scan_query), offsetof(mmgpu_scan_params, max_hits),\n'
           '           offsetof(mmgpu_scan_query, max_tlen));\n    return 0;\n}\n')
    c = tmp_path / "sizes.c"
    c.write_text(src)
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out == [ctypes.sizeof(capi.ScanParams), ctypes.sizeof(st), capi.ScanParams.max_hits.offset, st.max_tlen.offset]
