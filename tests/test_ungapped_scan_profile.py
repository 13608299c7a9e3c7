"""CPU tests of profile queries in the exhaustive ungapped scan (`mmgpu_scan_query::profile`): the numpy restatement
(tests/ungapped_scan_profile_cases.py) against the lists recorded from the stock binary with profile query databases
(tests/golden/ungapped_scan_profile.npz), the struct layout, the binding's marshalling."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import ungapped_scan_profile_cases as upc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    return upc.Golden()


@pytest.fixture(scope="module")
def group_scores(G):
    """group -> uint8 [queries][targets], computed once"""
    return {grp: np.stack([upc.scores_one_query(p, G.targets(grp)) for p in G.profiles(grp)]) for grp in G.groups}


def test_restatement_equals_every_recorded_list(G, group_scores):
    """ids and scores, at every setting of both groups.  Where they differ the restatement is wrong, not the file."""
    assert G.groups == ["A", "B"]
    for k, s in enumerate(G.settings):
        sc, tl, profs = group_scores[s["group"]], G.tlens(s["group"]), G.profiles(s["group"])
        exp = G.expected(k)
        assert len(exp) == len(profs)
        for qi, (ids, scores) in enumerate(exp):
            win = capi.coverage_window(s["cov"], s["cov_mode"], profs[qi].shape[1], tl)
            gi, gs = upc.select_list(sc[qi], tl, win, s["min_score"], s["max_seqs"])
            assert np.array_equal(gi, ids) and np.array_equal(gs, scores), (s["group"], s["name"], qi)


def test_vector_form_equals_the_cell_recurrence():
    """30 random small pairs: profiles with and without negative scores, 20 and 21 rows, targets that hold the letter without a row"""
    rng = np.random.default_rng(31)
    for k in range(30):
        letters = 21 if k % 5 == 4 else 20
        lo = 0 if k % 7 == 6 else -int(rng.integers(1, 40))
        prof = rng.integers(lo, 30, (letters, int(rng.integers(1, 40)))).astype(np.int8)
        t = upc.random_seq(rng, int(rng.integers(0, 50)), alphabet=21)
        assert int(upc.scores_one_query(prof, [t])[0]) == upc.pair_score_cells(prof, t), k


def test_recording_is_worth_keeping(G):
    """pairs at their query's cap, lists cut inside a score class, an empty list, a target dropped by the coverage setting, several
    values of B, byte-equal lists with and without the composition bias - and the settings and lengths the recording was to hold"""
    shown = upc.check_recording(G)
    assert shown["saturated"] >= 4 and shown["cut_in_class"] >= 2 and {1, 32} <= set(shown["biases"])
    have = {(s["group"], s["min_score"], s["max_seqs"], s["cov"], s["cov_mode"], s["comp_bias"]) for s in G.settings}
    for want in [("A", 15, 300, 0.0, 0, 1), ("A", 0, 300, 0.0, 0, 1), ("A", 15, 10, 0.0, 0, 1), ("A", 15, 300, 0.8, 0, 1),
                 ("A", 15, 300, 0.0, 0, 0), ("B", 15, 300, 0.0, 0, 1)]:
        assert want in have, want
    la = sorted(len(e) for e in G.entries("A"))
    assert 8 <= len(la) <= 10 and la[-1] > 512
    for edge in (128, 256, 512):
        assert any(n < edge for n in la) and any(n > edge for n in la)
    assert sum(len(e) >= 100 and upc.bias_of(upc.alignment_profile(e)) <= 8 for e in G.entries("B")) >= 3
    assert os.path.getsize(upc.GOLDEN) < 400 * 1000


def test_header_struct_and_flat_descriptor_agree_on_the_profile_fields(tmp_path):
    """mmgpu.h declares profile, then profile_letters, at the end of mmgpu_scan_query; the C compiler, capi.ScanQuery and
    SCAN_QUERY_DTYPE place them alike"""
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mmgpu_scan_query;", hdr).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields[-3:] == ["max_tlen", "profile", "profile_letters"], fields
    st, dt = capi.ScanQuery, capi.SCAN_QUERY_DTYPE
    assert [n for n, _ in st._fields_][-2:] == ["profile", "profile_letters"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmgpu.h"\nint main(void) {\n'
           '    printf("%zu %zu %zu\\n", sizeof(mmgpu_scan_query), offsetof(mmgpu_scan_query, profile),\n'
           '           offsetof(mmgpu_scan_query, profile_letters));\n    return 0;\n}\n')
    c = tmp_path / "offsets.c"
    c.write_text(src)
    exe = str(tmp_path / "offsets")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out == [ctypes.sizeof(st), st.profile.offset, st.profile_letters.offset]
    assert out == [dt.itemsize, dt.fields["profile"][1], dt.fields["profile_letters"][1]]


class _NoDevice(capi.MMGpu):
    """_scan_marshal touches nothing of the context"""

    def __init__(self):
        pass

    def __del__(self):
        pass


def test_marshal_places_a_strided_profile_and_accepts_a_missing_q():
    rng = np.random.default_rng(32)
    wide = rng.integers(-20, 20, (25, 70)).astype(np.int8)
    view = wide[:20, 3:63:2]                               # [20][30], neither row- nor column-contiguous
    assert not view.flags["C_CONTIGUOUS"]
    cons = upc.random_seq(rng, 30)
    mat = np.zeros((21, 21), np.int8)
    qs = [dict(profile=view, identity_id=7, window=(5, 90)), dict(q=cons, profile=view, comp_bias=np.ones(30, np.int8)),
          dict(q=cons, comp_bias=np.ones(30, np.int8))]
    par, arr, keep = _NoDevice()._scan_marshal(mat, qs, 15, 300)
    assert par.alphabet == 21 and par.max_hits == 300
    for k in (0, 1):
        a = arr[k]
        assert a.qlen == 30 and a.profile_letters == 20 and a.profile
        got = np.ctypeslib.as_array(ctypes.cast(a.profile, ctypes.POINTER(ctypes.c_int8)), (20 * 30,))
        assert np.array_equal(got.reshape(20, 30), view)      # letter-major, contiguous
    assert not arr[0].q and (arr[0].identity_id, arr[0].min_tlen, arr[0].max_tlen) == (7, 5, 90)
    assert arr[1].q and arr[1].comp_bias and arr[1].identity_id == 0xFFFFFFFF      # (passed on; the library ignores it)
    assert arr[2].q and arr[2].comp_bias and not arr[2].profile and arr[2].profile_letters == 0
    with pytest.raises(ValueError):
        _NoDevice()._scan_marshal(mat, [dict(q=cons[:29], profile=view)], 15, 300)
    with pytest.raises(ValueError):
        _NoDevice()._scan_marshal(mat, [dict(comp_bias=None)], 15, 300)
    del keep
