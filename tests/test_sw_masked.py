"""CPU tests of the masked alignment batch (mmgpu_sw_prepare_masked, --alt-ali's second alignments): the C-ABI's two new symbols,
the yardstick of the GPU tests (the oracle's chains against the vectors recorded from the real reference), and the span
bookkeeping of capi.alt_alignments."""
import os
import re

import numpy as np

from mmseqs2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mmgpu_sw_prepare_masked", "mmgpu_sw_debug_masked_target")
FIELDS = ("score", "q_end", "t_end", "q_start", "t_start", "word", "ident")


def load_alt_ali_vectors():
    """tests/golden/alt_ali_vectors.npz (make_alt_ali_golden.py) -> (scalars dict, list of families: q, cb, t, chain of (row, bt))"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "alt_ali_vectors.npz"))
    qoff, toff, coff = g["qoff"].astype(np.int64), g["toff"].astype(np.int64), g["chain_off"].astype(np.int64)
    bts = bytes(g["bt"]).decode().split("\n")
    fams = []
    for f in range(len(coff) - 1):
        chain = [([int(x) for x in g["expect"][k]], bts[k]) for k in range(coff[f], coff[f + 1])]
        fams.append(dict(q=g["qres"][qoff[f]:qoff[f + 1]], cb=g["cb"][qoff[f]:qoff[f + 1]], t=g["tres"][toff[f]:toff[f + 1]], chain=chain))
    par = {k: int(g[k]) for k in ("gap_open", "gap_extend", "threshold", "max_rounds", "mask_letter")}
    return par, fams


def test_masked_batch_symbols_declared_listed_and_exported():
    import mmseqs2_amd
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmgpu_[a-z0-9_]+)\s*\(", hdr))
    mmseqs2_amd.build_library()
    L = capi.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in capi.EXPORTED_SYMBOLS, sym
        assert hasattr(L, sym), sym
    for name in ("mmgpu_sw_span", "mmgpu_sw_masks"):
        assert re.search(r"\}\s*%s\s*;" % name, hdr), name
    # the client library answers both (MMGPU_ERR_UNSUPPORTED): a binary linked against it still resolves every symbol of the header
    import ctypes
    client = ctypes.CDLL(os.path.join(os.path.dirname(capi.library_path()), "libmmgpu_client.so"))
    b = ctypes.c_void_p(1)
    assert client.mmgpu_sw_prepare_masked(None, None, None, 0, 1, None, ctypes.byref(b)) == -4 and b.value is None
    assert client.mmgpu_sw_debug_masked_target(None, None, 0, None, 0, None) == -4


def test_oracle_chains_equal_the_recorded_reference_chains(oracle, matrices):
    """Align, overwrite [t_start, t_end) with X, align again: the restatement walks the chains the real reference walked, field by
    field.  The GPU tests compare the device with the restatement on masked targets; this pins the restatement there."""
    par, fams = load_alt_ali_vectors()
    mat = matrices["blosum62_sw"]
    assert [len(f["q"]) for f in fams] == [1, 5, 17, 37, 61, 130, 530]
    n = n_word = 0
    for f in fams:
        t = f["t"].copy()
        for k, (row, bt) in enumerate(f["chain"]):
            r = oracle.sw_align(f["q"], f["cb"], t, mat, par["gap_open"], par["gap_extend"], need_start=True, need_bt=True)
            if row[0] > 0:
                assert [r[x] for x in FIELDS] == row and r["bt"] == bt, (len(f["q"]), k)
                t[row[4]:row[2]] = par["mask_letter"]
            else:
                assert r["score"] == 0 and r["t_end"] == -1
            # the chain's own rule: it goes on while the score reaches the threshold, for max_rounds masked rounds at the most
            last = k + 1 == len(f["chain"])
            assert last == (k > 0 and (row[0] < par["threshold"] or k == par["max_rounds"])), (len(f["q"]), k)
            n += 1
            n_word += row[5]
        if len(f["q"]) > 1:
            assert sum(row[0] >= par["threshold"] for row, _ in f["chain"]) >= 2
    one = fams[0]["chain"]
    assert len(one) == 2 and one[0] == one[1] and one[0][0][4] == one[0][0][2]      # one residue: the empty span, the same alignment again
    assert n >= 20 and 4 <= n_word < n      # hits of the uint8 range and of the int16 range


def test_alt_next_spans():
    rec = np.zeros(4, capi.SW_HIT_DTYPE)
    rec["t_start"] = [3, 10, 7, 0]
    rec["t_end"] = [9, 10, 20, 5]
    s1 = capi.alt_next_spans([[], [], [(1, 2)], None], rec, [True, True, True, True])
    assert s1 == [[(3, 9)], [(10, 10)], [(1, 2), (7, 20)], None]      # accumulation, the empty span of a one-residue alignment, a pair that was out
    rec["t_start"] = [20, 10, 0, 0]
    rec["t_end"] = [30, 10, 3, 0]
    s2 = capi.alt_next_spans(s1, rec, np.array([True, True, False, True]))
    assert s2 == [[(3, 9), (20, 30)], [(10, 10), (10, 10)], None, None]      # a rejected pair drops out and stays out
    assert s1 == [[(3, 9)], [(10, 10)], [(1, 2), (7, 20)], None]             # (a pure function: its input is as it was)
    assert capi.alt_next_spans([], rec[:0], []) == []
