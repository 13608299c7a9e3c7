"""tantan repeat masking at its edges, on the CPU: the restatement (oracle/tantan_oracle.c) against the compiled reference where the
recorded vectors of tests/test_tantan.py do not reach - every length 0 .. 70 (each max_offset of the partial first 50 positions), one
planted repeat per period 1 .. 52 (every history word, every repeat state), the X cases, a second likelihood-ratio table (BLOSUM62)
and a second threshold (0.5f): tests/golden/tantan_edge_vectors.npz, recorded by tests/golden/make_tantan_edge_golden.py; and, where
oracle/_ref and the reference's data are present, the longest admitted sequence against the library itself.  The device tests
(tests/test_tantan_gpu.py) compare with the restatement, so what is pinned here is what they stand on."""
import os

import numpy as np
import pytest

from tests import tantan_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("vtml80", "blosum62")
THRESHOLDS = (("09", float(np.float32(0.9))), ("05", float(np.float32(0.5))))


@pytest.fixture(scope="module")
def edge():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "tantan_edge_vectors.npz")))


def test_the_recorded_inputs_are_the_generated_ones(edge):
    for name, seqs in tc.all_sets().items():
        res, off = tc.pack(seqs)
        assert np.array_equal(res, edge[name + "_res"]) and np.array_equal(off, edge[name + "_off"]), name
    lens = np.diff(edge["lengths_off"].astype(np.int64))
    assert sorted(lens.tolist()) == sorted(3 * list(range(71)))
    assert sum(len(t) for t in tc.probe_set()) <= 400 and len(tc.probe_set()) <= 8
    assert {15, 16, 17, 49, 50, 51} <= {len(t) for t in tc.probe_set()}


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("name", tc.SET_NAMES)
def test_restatement_equals_the_recorded_edge_probabilities_and_masks(oracle, edge, name, table):
    res, off, lr = edge[name + "_res"], edge[name + "_off"], edge[table + "_likelihood_ratios"]
    want_p = edge["%s_%s_probs" % (name, table)]
    n_bits = 0
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        p = oracle.tantan_probs(res[a:b], lr)
        assert np.array_equal(p.view(np.uint32), want_p[a:b].view(np.uint32)), (name, table, i)
        n_bits += b - a
    assert n_bits == len(res)
    for key, thr in THRESHOLDS:
        masked, n = oracle.tantan_mask(res, off, lr, thr)
        assert n == int(edge["%s_%s_n_%s" % (name, table, key)]), (name, table, key)
        assert np.array_equal(masked, edge["%s_%s_masked_%s" % (name, table, key)]), (name, table, key)
        # the recorded count is the number of letters at or above the threshold, whatever letter they were
        assert n == int((want_p.astype(np.float64) >= thr).sum())


def test_the_periods_set_is_not_vacuous(edge):
    """With VTML80 at 0.9f the planted repeat of every period the model has a state for (1 .. 50) is found, at least one unit of it;
    the repeats of period 51 and 52 are beyond the model and stay unmasked.  A history letter read from the wrong place therefore
    changes a mask of this set, whichever state it belongs to."""
    off = edge["periods_off"].astype(np.int64)
    p09 = edge["periods_vtml80_probs"].astype(np.float64) >= float(np.float32(0.9))
    assert len(off) - 1 == tc.MAX_PERIOD
    for p in range(1, tc.MAX_PERIOD + 1):
        a, n = tc.period_layout(p)
        n_masked = int(p09[off[p - 1] + a:off[p - 1] + a + n].sum())
        if p <= 50:
            assert n_masked >= p, (p, n_masked)
        else:
            assert n_masked == 0, (p, n_masked)


def test_the_letters_set_masks_letters_that_already_are_the_mask_letter(edge):
    off = edge["letters_off"].astype(np.int64)
    res = edge["letters_res"]
    p09 = edge["letters_vtml80_probs"].astype(np.float64) >= float(np.float32(0.9))
    a, b = off[4], off[5]      # the repeat made of X
    assert int((p09[a:b] & (res[a:b] == tc.X)).sum()) >= 10
    changed = int((edge["letters_vtml80_masked_09"] != res).sum())
    assert int(edge["letters_vtml80_n_09"]) > changed


def test_restatement_equals_the_compiled_reference_on_the_longest_sequences(oracle):
    from oracle import pyoracle
    if not (pyoracle.ref_available() and pyoracle.ref_matrix_available()):
        pytest.skip("real reference (oracle/_ref + /root/reference/data) not available here")
    ref = pyoracle.RefPrefilter()
    mp = float(np.float32(0.9))
    for n, seed in ((65535, 41), (65520, 42)):
        res, off = tc.pack([tc.long_sequence(n, seed)])
        want, n_want, lr, want_p = ref.tantan_mask(res, off, mp)
        got_p = oracle.tantan_probs(res, lr)
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), n
        got, n_got = oracle.tantan_mask(res, off, lr, mp)
        assert n_got == n_want and np.array_equal(got, want), n
        m = got != res
        assert m[10:200].sum() >= 60 and m[65000:65400].sum() >= 100 and m[300:64900].sum() < m.sum() // 4, n
