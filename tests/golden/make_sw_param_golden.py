#!/usr/bin/env python3
"""Generates tests/golden/sw_param_vectors.npz from the REAL reference (oracle/_ref/libmmref.so, `make -C oracle ref`), in the
style of make_golden.py: for every setting of tests/sw_param_cases.py SW_PARAM_SETS the int8 matrix the reference derives, its
background pBack, the serialized matrix, and PAIRS_PER_SET pairs of the shared generator with the reference's results in
modes 0 / 1 / 2.  Only queries inside the acceptance rule (oracle/sw_oracle.c) are recorded: outside it the reference's
numbers are not the recurrence the restatement and the kernels compute.

    python tests/golden/make_sw_param_golden.py

Keys of the .npz: "<set key>/<name>" with name in mat, pback, serialized, gap_open, gap_extend, qres, qoff, tres, toff, cb,
expect ([n, 7] int32: score, q_end, t_end, q_start, t_start, word, ident), bt (backtraces joined by newlines)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Oracle, RefLib  # noqa: E402
from mmseqs2_amd import workloads as wl  # noqa: E402
from tests import sw_param_cases as pc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PAIRS_PER_SET = 60
SEED = 20261016


def one_set(d, orc, index, key, mfile, go, ge):
    ref = RefLib(mfile, 2.0, 0.0, gap_open=go, gap_extend=ge)      # Alignment.cpp:152: bit factor 2, no score bias
    mat = ref.matrix()
    pb = np.zeros(ref.alphabet, np.float64)
    ref.L.mmref_get_pback.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    ref.L.mmref_get_pback(ref.c, pb.ctypes.data)
    qs, ts, cbs, rows, bts = [], [], [], [], []
    for kind, q, t in pc.generate_pairs(SEED + index, 4 * PAIRS_PER_SET):
        if len(qs) == PAIRS_PER_SET:
            break
        if len(q) > 700 and len(qs) % 6:       # a few multi-tile queries per set, not one pair in six (file size)
            q = q[:int(len(q) // 3)]
        ref.sw_set_query(q)
        cb = orc.round_comp_bias(ref.comp_bias(q))
        if not pc.rule_accepts(orc, mat, cb, len(q), go, ge):
            continue
        a0, a1, a2 = ref.sw_align(t, 0), ref.sw_align(t, 1), ref.sw_align(t, 2)
        assert a0["score"] == a1["score"] == a2["score"]
        # score 0: the reference returns before touching identicalAACnt (uninitialised, ssw_align_private :850-852)
        ident = a2["ident"] if a0["score"] > 0 else 0
        qs.append(q); ts.append(t); cbs.append(cb)
        rows.append([a0["score"], a0["q_end"], a0["t_end"], a1["q_start"], a1["t_start"], a0["word"], ident])
        bts.append(a2["bt"])
    assert len(qs) == PAIRS_PER_SET
    qres, qoff = wl.seqs_from_list(qs)
    tres, toff = wl.seqs_from_list(ts)
    d[key + "/mat"] = mat
    d[key + "/pback"] = pb
    d[key + "/serialized"] = np.frombuffer(ref.serialized_matrix(), np.uint8)
    d[key + "/gap_open"] = np.int32(go)
    d[key + "/gap_extend"] = np.int32(ge)
    d[key + "/qres"], d[key + "/qoff"], d[key + "/tres"], d[key + "/toff"] = qres, qoff, tres, toff
    d[key + "/cb"] = np.concatenate(cbs)
    d[key + "/expect"] = np.array(rows, np.int32)
    d[key + "/bt"] = np.frombuffer("\n".join(bts).encode(), np.uint8)
    print(key, "pairs", len(qs), "word-mode", int(np.array(rows)[:, 5].sum()), "score 0:", int((np.array(rows)[:, 0] == 0).sum()),
          "longest query", max(len(q) for q in qs))


if __name__ == "__main__":
    d = {}
    orc = Oracle()
    for index, (key, mfile, go, ge) in enumerate(pc.SW_PARAM_SETS):
        one_set(d, orc, index, key, mfile, go, ge)
    path = os.path.join(OUT, "sw_param_vectors.npz")
    np.savez_compressed(path, **d)
    print("sw_param_vectors.npz", os.path.getsize(path), "bytes")
