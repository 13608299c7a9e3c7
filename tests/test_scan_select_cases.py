"""The inputs of the selection tests over several compaction rounds and over a full key array (tests/ungapped_scan_cases.py,
tests/gapped_scan_cases.py: rounds_case, full_case), checked on the expectations alone before a device sees them: the tie class lies
on both sides of the round boundaries, every chosen max_hits cuts it where it is meant to, and the full case admits more than the key
array holds."""
import numpy as np
import pytest

from tests import gapped_scan_cases as gc
from tests import ungapped_scan_cases as uc


def cases(scan, oracle):
    if scan == "ungapped":
        return uc.rounds_case(), uc.full_case(), uc.select_list
    return gc.rounds_case(oracle), gc.full_case(oracle), gc.select_list


@pytest.mark.parametrize("scan", ["ungapped", "gapped"])
def test_rounds_case_cuts_the_tie_class_at_the_round_boundaries(oracle, scan):
    C, _, select = cases(scan, oracle)
    R = uc.SELECT_ROUND
    assert len(C["targets"]) == 2100 and all(5 <= n <= 40 for n in C["tlens"])
    tie = uc.ROUNDS_TIE_IDS
    assert tie.min() < R <= tie[tie >= R].min() < 2 * R and (tie < 2 * R).any() and tie.max() >= 2 * R
    # the class is a class: one score, which no other target has, with admitted targets above it in every round and below it
    raw = C["raw"][0]
    s = int(raw[tie[0]])
    assert (raw[tie] == s).all() and np.array_equal(np.flatnonzero(raw == s), tie) and s > uc.ROUNDS_MIN_SCORE
    above = np.flatnonzero(raw > s)
    assert all(((above >= lo) & (above < lo + R)).any() for lo in (0, R, 2 * R))
    assert ((raw < s) & (raw > uc.ROUNDS_MIN_SCORE)).sum() > 100
    M = C["max_hits"]
    last = {}
    for tag in "abcd":
        lists = uc.case_lists(C, select, M[tag])
        assert all(len(ids) == M[tag] for ids, _ in lists)      # both queries' lists are cut
        last[tag], kept = uc.last_tie_member(lists[0][0])
        assert 0 < kept < len(tie) and lists[0][1][-1] == s         # the cut is inside the class
    assert last["a"] < R - 1 and last["b"] == R - 1 and last["c"] == R and 2 * R <= last["d"] < tie.max()
    lists = uc.case_lists(C, select, M["all"])
    assert all(len(ids) < M["all"] for ids, _ in lists) and uc.last_tie_member(lists[0][0]) == (int(tie.max()), len(tie))
    assert len(lists[1][0]) > R      # the unrelated query's list spans rounds too


@pytest.mark.parametrize("scan", ["ungapped", "gapped"])
def test_full_case_admits_more_than_the_key_array_holds(oracle, scan):
    _, C, select = cases(scan, oracle)
    assert len(C["targets"]) == 4200 and all(5 <= n <= 20 for n in C["tlens"])
    assert C["max_hits"] == dict(full=uc.SELECT_KEYS) and C["rule"]["min_score"] == -1
    for k, (ids, sc) in enumerate(uc.case_lists(C, select, uc.SELECT_KEYS)):
        raw = C["raw"][k]
        assert (raw > -1).sum() == 4200 > uc.SELECT_KEYS and len(ids) == uc.SELECT_KEYS
        # the cut class is the lowest score, cut by id: its kept members are its lowest ids, and some are left out
        low = np.flatnonzero(raw == raw.min())
        kept = ids[sc == raw.min()]
        assert sc[-1] == raw.min() and 0 < len(kept) < len(low) and np.array_equal(kept, low[:len(kept)])
