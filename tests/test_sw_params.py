"""CPU tests: the plain-C Smith-Waterman restatement (oracle/sw_oracle.c) and its acceptance rule against the real reference
away from BLOSUM62 11/1 - the table of matrices and gap costs of tests/sw_param_cases.py, engineered ties, saturated hits and
sequences of the maximal 65535 residues.  The reference-backed tests skip where oracle/_ref was not built;
test_restatement_matches_param_goldens carries the pin to machines without the reference tree."""
import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from tests import sw_param_cases as pc

PAIRS_PER_SET = 3000
# settings at which the composition bias of two-letter / homopolymer queries leaves the rule so often that the 20 % cap on
# excluded queries would be at risk: keep every k-th such pair (sw_param_cases.generate_pairs)
LOW_COMPLEXITY_EVERY = {"blosum62_5_2": 2}

FWD = ["score", "q_end", "t_end", "word"]
START = ["q_start", "t_start"]


def _ref_for(mfile, go, ge, comp_bias=True):
    from oracle import pyoracle
    if not (pyoracle.ref_available() and pyoracle.ref_matrix_available()):
        pytest.skip("real reference (oracle/_ref + its data directory) not available here")
    return pyoracle.RefLib(mfile, 2.0, 0.0, gap_open=go, gap_extend=ge, comp_bias=comp_bias)


def _same(a, b, mode, tag):
    """reference result a == restatement result b in the fields the mode defines"""
    if a["score"] == 0:
        assert b["score"] == 0 and b["t_end"] == -1, tag
        return
    keys = FWD + (START if mode >= 1 else []) + (["bt", "ident"] if mode >= 2 else [])
    for k in keys:
        assert a[k] == b[k], (tag, mode, k, a[k], b[k])


@pytest.mark.parametrize("key", [s[0] for s in pc.SW_PARAM_SETS])
def test_restatement_equals_reference_over_parameters(oracle, key):
    """Every field of every pair whose query the acceptance rule admits, modes 0 and 1 (mode 2 for one pair in eight); at most
    20 % of the queries may be outside the rule."""
    _, mfile, go, ge = pc.set_by_key(key)
    ref = _ref_for(mfile, go, ge)
    mat = ref.matrix()
    pairs = pc.generate_pairs(4242, PAIRS_PER_SET, LOW_COMPLEXITY_EVERY.get(key, 1))
    n_out = n_word = n_long = n_scored = 0
    for i, (kind, q, t) in enumerate(pairs):
        ref.sw_set_query(q)
        cb = oracle.round_comp_bias(ref.comp_bias(q))
        if not pc.rule_accepts(oracle, mat, cb, len(q), go, ge):
            n_out += 1
            continue
        for mode in (0, 1, 2) if i % 8 == 0 else (0, 1):
            a = ref.sw_align(t, mode)
            b = oracle.sw_align(q, cb, t, mat, go, ge, need_start=mode >= 1, need_bt=mode >= 2)
            _same(a, b, mode, (key, i, kind, len(q), len(t)))
        n_word += a["word"]
        n_long += len(q) > 512
        n_scored += a["score"] > 0
    print("%s: %d pairs, %d outside the rule, %d int16-range, %d queries above 512 rows" % (key, len(pairs), n_out, n_word, n_long))
    assert n_out <= pc.MAX_REFUSED_SHARE * len(pairs), (key, n_out)
    assert n_word > 100 and n_long > 100 and n_scored > len(pairs) // 2, (n_word, n_long, n_scored)


def test_saturated_hit_start_positions_vs_reference(oracle):
    """A self hit beyond 32767: the int16 pass saturates, the reverse scan stops at the first column that reaches 32767."""
    ref = _ref_for("blosum62.out", 11, 1, comp_bias=False)
    mat = ref.matrix()
    q, targets = pc.saturating_pair()
    ref.sw_set_query(q)
    scores = []
    for k, t in enumerate(targets):
        for mode in (0, 1):
            a = ref.sw_align(t, mode)
            b = oracle.sw_align(q, None, t, mat, 11, 1, need_start=mode >= 1)
            _same(a, b, mode, ("saturated", k))
            assert a["word"] == 1
        scores.append(a["score"])
    assert scores[0] == 32767 and scores[2] < 32767 and scores[1] < 32767


def test_maximal_length_ties_vs_reference(oracle):
    """65535 residues: the last column / row index is 65534, one below the 0xFFFF the result key of the kernels reserves."""
    ref = _ref_for("blosum62.out", 11, 1, comp_bias=False)
    mat = ref.matrix()
    for name, q, t, (q_end, t_end) in pc.maximal_length_cases():
        ref.sw_set_query(q)
        for mode in (0, 1):
            a = ref.sw_align(t, mode)
            b = oracle.sw_align(q, None, t, mat, 11, 1, need_start=mode >= 1)
            _same(a, b, mode, name)
        assert (a["q_end"], a["t_end"]) == (q_end, t_end), (name, a)
        assert (a["q_end"] - a["q_start"], a["t_end"] - a["t_start"]) == (299, 299), (name, a)


def test_acceptance_rule_is_sufficient(oracle):
    """gap_open == gap_extend: the reference's int16 pass is not the plain recurrence (differing pairs below, forward scan; its
    start-position pass exits the process on them), so mmo_sw_check_params must refuse these settings for every query - as it
    must refuse a matrix whose minimum leaves the rule (PAM30 at 11/1)."""
    rng = np.random.default_rng(1)
    q = rng.choice(20, size=200, p=wl.BACKGROUND).astype(np.uint8)
    n_diff = {}
    for mfile, go, ge in pc.SW_REFUSED_EQUAL_GAPS:
        if (go, ge) == (3, 3):
            continue        # (its e-value set-up alone takes a minute; the rule is checked for it below)
        ref = _ref_for(mfile, go, ge)
        mat = ref.matrix()
        n_diff[(go, ge)] = 0
        for i, (kind, qq, t) in enumerate(pc.generate_pairs(1234, 600)):
            ref.sw_set_query(qq)
            cb = oracle.round_comp_bias(ref.comp_bias(qq))
            a = ref.sw_align(t, 0)
            b = oracle.sw_align(qq, cb, t, mat, go, ge)
            n_diff[(go, ge)] += any(a[k] != b[k] for k in FWD) and a["score"] > 0
    print("pairs that differ from the reference at gap_open == gap_extend:", n_diff)
    assert all(v > 0 for v in n_diff.values()), n_diff       # the reason for the rule: if this stops holding, revisit it
    mat62 = pc.load_param_vectors()["blosum62_11_1"]["mat"]
    for _, go, ge in pc.SW_REFUSED_EQUAL_GAPS + [("", 1, 2), ("", 0, 0), ("", 5, -1)]:
        assert not pc.rule_accepts(oracle, mat62, None, len(q), go, ge), (go, ge)
        assert not pc.rule_accepts(oracle, mat62, np.zeros(len(q), np.int8), len(q), go, ge), (go, ge)
    for go, ge in [(11, 1), (9, 2), (6, 5), (10, 9), (4, 1)]:
        assert pc.rule_accepts(oracle, mat62, None, len(q), go, ge), (go, ge)
    pam30 = pc.load_param_vectors()["pam30_25_2"]["mat"]
    assert int(pam30.min()) == -17
    assert not pc.rule_accepts(oracle, pam30, None, len(q), 11, 1) and pc.rule_accepts(oracle, pam30, None, len(q), 25, 2)
    # the composition bias counts: -4 + -6 + 2 > -8 fails
    cb = np.zeros(len(q), np.int8)
    cb[17] = -6
    assert pc.rule_accepts(oracle, mat62, cb, len(q), 9, 2) and not pc.rule_accepts(oracle, mat62, cb, len(q), 8, 2)


def test_restatement_matches_param_goldens(oracle):
    """The recorded reference results of every set (tests/golden/sw_param_vectors.npz, make_sw_param_golden.py): all fields, the
    backtrace and the identity count included; every recorded query lies inside the acceptance rule."""
    sets = pc.load_param_vectors()
    assert sorted(sets) == sorted(s[0] for s in pc.SW_PARAM_SETS)
    for key, v in sets.items():
        n_word = n_tile = 0
        for i, (q, cb, t, exp) in enumerate(v["pairs"]):
            assert pc.rule_accepts(oracle, v["mat"], cb, len(q), v["go"], v["ge"]), (key, i)
            r = oracle.sw_align(q, cb, t, v["mat"], v["go"], v["ge"], need_start=True, need_bt=True)
            got = [r["score"], r["q_end"], r["t_end"], r["q_start"], r["t_start"], r["word"], r["ident"]]
            assert got == [int(x) for x in exp], (key, i, got, exp.tolist())
            assert r["bt"] == v["bt"][i], (key, i)
            n_word += r["word"]
            n_tile += len(q) > 512
        assert n_word >= 5 and n_tile >= 1, (key, n_word, n_tile)


@pytest.mark.parametrize("key", ["blosum62_11_1", "blosum62_5_2"])
def test_engineered_tie_constructions_hold_their_ties(oracle, key):
    """The constructions tests/test_sw_params_gpu.py test_engineered_ties sends to the device, without one: the test's own numpy DP
    equals the restatement on every pair, and every tie category occurs (forward scan in both sets, reverse scan at 5/2)."""
    v = pc.load_param_vectors()[key]
    n_fwd, n_rev = dict.fromkeys("abcd", 0), dict.fromkeys("abcd", 0)
    for name, q, t in pc.engineered_tie_pairs(v["mat"], v["go"]):
        fwd, rev, by_dp = pc.classify_ties(q, None, t, v["mat"], v["go"], v["ge"])
        r = oracle.sw_align(q, None, t, v["mat"], v["go"], v["ge"], need_start=True)
        assert (r["score"], r["q_end"], r["t_end"], r["q_start"], r["t_start"]) == by_dp, name
        for c in fwd:
            n_fwd[c] += 1
        for c in rev:
            n_rev[c] += 1
    assert all(n > 0 for n in n_fwd.values()) and n_rev["d"] > 0, (n_fwd, n_rev)
    if key == "blosum62_5_2":
        assert all(n > 0 for n in n_rev.values()), n_rev
