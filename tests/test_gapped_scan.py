"""The exhaustive gapped scan on the CPU: the restatement of tests/gapped_scan_cases.py (the plain-C Gotoh oracle, the identity sum,
the list rule with both thresholds) reproduces every list the stock binary's `gappedprefilter` recorded in
tests/golden/gapped_scan.npz, and the recording shows what the device tests rely on."""
import functools

import numpy as np
import pytest

from tests import gapped_scan_cases as gc


@functools.lru_cache(maxsize=None)
def golden():
    return gc.Golden()


def test_recording_exercises_what_is_new(oracle):
    shown = gc.check_recording(golden(), oracle)
    assert shown["above_255"] >= 8 and shown["identity_entries"] == len(golden().queries)


@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_restatement_equals_the_recorded_lists(oracle, k):
    G = golden()
    got, want = gc.restated_lists(oracle, G, k), G.expected(k)
    assert len(got) == len(want) == len(G.queries)
    for i, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (G.settings[k]["name"], i, gi[:12], wi[:12], gs[:12], ws[:12])


def test_min_evalue_score_is_the_smallest_passing_score():
    ev = lambda s, qlen: 1000.0 * qlen * 2.0 ** (-s / 2.0)      # falls monotonically in the score
    for qlen, e in ((8, 10.0), (100, 1e-3), (700, 1e-10)):
        s = gc.min_evalue_score(ev, qlen, e)
        assert ev(s, qlen) <= e and (s == 0 or ev(s - 1, qlen) > e)
    assert gc.min_evalue_score(ev, 100, 1e30) == 0 and gc.min_evalue_score(ev, 100, -1.0) == gc.NEVER


def test_identity_sum_wraps_as_int16(oracle):
    G = golden()
    mat = G.g["mat_blosum62"]
    w = int(np.argmax(np.diag(mat)[:20]))      # the letter with the highest self score (W: 11)
    q = np.full(3000, w, np.uint8)
    plain = 3000 * int(mat[w, w])
    assert plain > 32767
    assert gc.score_identical(oracle, mat, dict(q=q), q) == ((plain + 32768) % 65536) - 32768 < 0
    prof = np.full((20, 3000), int(mat[w, w]), np.int8)
    assert gc.score_identical(oracle, mat, dict(q=q, profile=prof), q) == ((plain + 32768) % 65536) - 32768
