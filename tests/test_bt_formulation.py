"""CPU tests of the restatement the wave traceback kernel (mmseqs2_amd/csrc/bt_wave_kernel.hip) rests on - F as a max-plus
prefix scan over "H without its F term", with previous-row values read by column - as serial Python (oracle/bt_rows.py
banded_rows) against the literal restatement of banded_sw (oracle/sw_oracle.c), string for string, at every (matrix, gap open,
gap extend) setting of tests/sw_param_cases.py.  The kernel's comment argues that value AND tie flag of F stay equal "because
gap_open >= gap_extend": 6/5 and 10/9, where opening and extending differ by 1, are in the table.
The cases (tests/bt_cases.py, small form: at most ~260 rows) include bands that double twice and more, composition bias from
the set's own matrix, and periodic sequences whose paths run over exact ties.

What these tests do NOT pin is the `zero_last` rule (the previous-row H / E seen at a row's last column are 0).  It only acts
in rows i <= band + 1 that the target end cuts (counted below as `clipped`), where it lowers E of the cell in the LAST target
column.  That cell feeds nothing to its right, its E stays below the alignment score (so no pass reaches the score sooner or
later because of it), and the walk leaves the corner by a match and never enters the column again: the rule cannot be seen in
the backtrace string.  banded_rows with zero_last = False gives the same string on every case of this module."""
import numpy as np
import pytest

from oracle.bt_rows import banded_rows
from tests import bt_cases as bc
from tests import sw_param_cases as pc

N_OTHER = 120       # homolog / periodic / with-X / long-insertion pairs per set, on top of the 108 constructions


def _sub(c):
    r = c["r"]
    qs, qe, ts, te = r["q_start"], r["q_end"], r["t_start"], r["t_end"]
    return c["q"][qs:qe + 1], None if c["cb"] is None else c["cb"][qs:qe + 1], c["t"][ts:te + 1]


@pytest.mark.parametrize("key", [s[0] for s in pc.SW_PARAM_SETS])
def test_row_parallel_formulation_equals_restatement(oracle, key):
    v = pc.load_param_vectors()[key]
    cases, n_refused = bc.band_cases(oracle, v, 100 + sum(map(ord, key)), small=True, n_other=N_OTHER)
    tally, n_ties = bc.Tally(), dict.fromkeys(("hd", "ef", "ee", "ff"), 0)
    for k, c in enumerate(cases):
        r = c["r"]
        if not r["bt"]:
            continue
        q, cb, t = _sub(c)
        got, on_path = banded_rows(q, cb, t, v["mat"], v["go"], v["ge"], r["score"], ties=True)
        assert got == r["bt"], (key, k, c["label"], bc.classify(r), got[:80], r["bt"][:80])
        tally.add(r, c["cb"])
        for tie in on_path:
            n_ties[tie[3]] += 1
    print("%s: %s; %d pairs outside the acceptance rule; ties consulted on the paths %s" % (key, tally, n_refused, n_ties))
    assert n_refused <= pc.MAX_REFUSED_SHARE * (len(cases) + n_refused), (key, n_refused)
    assert tally.n >= 150 and tally.with_gap >= 60, str(tally)
    assert tally.doublings["2"] + tally.doublings[">=3"] >= 10 and tally.doublings[">=3"] >= 1, str(tally)
    assert tally.clipped >= 1 and tally.with_bias >= 40 and tally.multi_chunk >= 5, str(tally)
    assert sum(n_ties.values()) > 0, n_ties         # (which kinds occur depends on the costs; the engineered ones are pinned below)


@pytest.mark.parametrize("key", ["blosum62_11_1", "blosum62_5_2"])
def test_tie_constructions_hold_their_ties(oracle, key):
    """The engineered ties tests/test_bt_gpu.py sends to the device, without one: every kind the set admits, at every offset of
    bt_cases.TIE_OFFSETS (tie_cases() keeps a pair only when the model's walk consults the tie in the constructed cell and its
    string is the restatement's); 'ef' has no construction at 5/2 (|min score| = 4 = 2 gap_extend)."""
    v = pc.load_param_vectors()[key]
    cases, skipped = bc.tie_cases(oracle, v)
    kinds = [k for k in bc.TIE_KINDS if k not in skipped]
    assert kinds == (["hd", "ee", "ff", "ef"] if key == "blosum62_11_1" else ["hd", "ee", "ff"]), (kinds, skipped)
    assert sorted((c["kind"], c["x"]) for c in cases) == sorted((k, x) for k in kinds for x in bc.TIE_OFFSETS)
    assert all(2 * c["r"]["band"] + 1 > 128 for c in cases)


def test_final_band_reported_by_the_restatement(oracle):
    """r["band"]: the initial band |tlen - qlen| + 1 times a power of two, at least the path's deviation from the diagonal; the
    entry point without the out-parameter gives the same string."""
    import ctypes
    from oracle.pyoracle import _ptr
    v = pc.load_param_vectors()["blosum62_11_1"]
    cases, _ = bc.band_cases(oracle, v, 3, small=True, n_other=24)
    n = 0
    for c in cases:
        r = c["r"]
        if not r["bt"]:
            assert r["band"] == 0
            continue
        q, cb, t = _sub(c)
        bc.classify(r)             # asserts band == initial band << doublings
        assert r["band"] >= bc.path_deviation(r["bt"])
        buf = ctypes.create_string_buffer(len(q) + len(t) + 8)
        mat = np.ascontiguousarray(v["mat"], np.int8)
        ln = oracle.L.mmo_sw_banded_backtrace(_ptr(np.ascontiguousarray(t)), _ptr(np.ascontiguousarray(q)), _ptr(cb), len(t), len(q), r["score"],
                                              v["go"], v["ge"], _ptr(mat), mat.shape[0], buf, len(buf))
        assert ln == len(r["bt"]) and buf.value.decode() == r["bt"]
        n += 1
    assert n >= 80
