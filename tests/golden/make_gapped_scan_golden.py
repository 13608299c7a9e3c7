"""Records tests/golden/gapped_scan.npz from the STOCK binary: the sequences of the ungapped recording (make_ungapped_scan_golden.py's
make_sequences) -> FASTA -> `mmseqs_stock createdb --shuffle 0` -> `mmseqs_stock gappedprefilter --threads 1` (runFilterOnCpu with
alignmentMode 1) for every setting below -> the result databases read back with mmseqs2_amd/dbio.py.  The same-database run scans
the query set against itself.  Stored: the sequences, the int8 matrices, the rounded composition bias of every query, the settings,
per (setting, query) min_evalue_score - the smallest score whose E-value (RefLib.evalue with the setting's matrix, gap costs and
database residue count) passes -e - and the expected (target key, score) lists.
Run in the build container after __graft_entry__.build():  python tests/golden/make_gapped_scan_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from mmseqs2_amd import capi, dbio                                  # noqa: E402
from oracle import pyoracle                                         # noqa: E402
from tests import gapped_scan_cases as gc                           # noqa: E402
from tests import sw_param_cases as spc                             # noqa: E402
from tests import ungapped_scan_cases as uc                         # noqa: E402
import make_ungapped_scan_golden as ung                             # noqa: E402

MATRICES = {"blosum62": "blosum62.out", "blosum80": "blosum80.out"}      # (blosum80_11_1 of tests/sw_param_cases.py's table)
assert any(f == "blosum80.out" and (go, ge) == (11, 1) for _, f, go, ge in spc.SW_PARAM_SETS)

BASE = dict(matrix="blosum62", comp_bias=1, min_score=15, max_seqs=300, e=0.001, cov=0.0, cov_mode=0, same_db=0, gap_open=11, gap_extend=1)
SETTINGS = [dict(BASE, name="base"),
            dict(BASE, name="no_comp_bias", comp_bias=0),
            dict(BASE, name="e_10", e=10.0),
            dict(BASE, name="e_1e-10", e=1e-10),
            dict(BASE, name="e_1e30", e=1e30),
            dict(BASE, name="min_score_60", min_score=60),
            dict(BASE, name="min_score_0", min_score=0),
            dict(BASE, name="max_seqs_10", max_seqs=10),
            dict(BASE, name="max_seqs_1000", max_seqs=1000),
            dict(BASE, name="cov_mode_0", cov=0.8, cov_mode=0),
            dict(BASE, name="cov_mode_1", cov=0.8, cov_mode=1),
            dict(BASE, name="cov_mode_2", cov=0.8, cov_mode=2),
            dict(BASE, name="same_db", same_db=1),
            dict(BASE, name="gaps_9_2", gap_open=9, gap_extend=2),
            dict(BASE, name="blosum80", matrix="blosum80")]


def sub_mat_argument(fname):
    """blosum62.out is compiled into the binary; the others are read from the reference's data directory"""
    return fname if fname == "blosum62.out" else os.path.join(pyoracle.REFERENCE_ROOT, "data", fname)


def main():
    lib = capi.load_library()
    oracle = pyoracle.Oracle()
    qs, ts = ung.make_sequences()
    (qres, qoff), (tres, toff) = uc.pack(qs), uc.pack(ts)
    out = dict(qres=qres, qoff=qoff, tres=tres, toff=toff)
    letters = None
    for name, fname in MATRICES.items():
        ref = pyoracle.RefLib(matrix=fname, bit_factor=2.0, score_bias=0.0)      # SubstitutionMatrix(file, 2.0, 0.0), ungappedprefilter.cpp:541
        out["mat_" + name] = ref.matrix()
        letters = letters or ref.num2aa()
        assert ref.num2aa() == letters, "the matrices order their letters differently"
        out["qcb_" + name] = np.concatenate([ung.round_bias(lib, ref.comp_bias(q, 1.0)) for q in qs])
    with tempfile.TemporaryDirectory() as tmp:
        ung.write_fasta(os.path.join(tmp, "q.fasta"), qs, letters)
        ung.write_fasta(os.path.join(tmp, "t.fasta"), ts, letters)
        qdb, tdb = os.path.join(tmp, "qdb"), os.path.join(tmp, "tdb")
        ung.run("createdb", os.path.join(tmp, "q.fasta"), qdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        ung.run("createdb", os.path.join(tmp, "t.fasta"), tdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        for k, s in enumerate(SETTINGS):
            res = os.path.join(tmp, "res_%d" % k)
            ung.run("gappedprefilter", qdb, qdb if s["same_db"] else tdb, res, "--threads", 1, "--comp-bias-corr", s["comp_bias"],
                    "--min-ungapped-score", s["min_score"], "--max-seqs", s["max_seqs"], "-e", repr(s["e"]), "-c", s["cov"],
                    "--cov-mode", s["cov_mode"], "--gap-open", s["gap_open"], "--gap-extend", s["gap_extend"],
                    "--sub-mat", sub_mat_argument(MATRICES[s["matrix"]]), "-v", 1)
            db = dbio.read_db(res)
            off, ids, sc = [0], [], []
            for qi in range(len(qs)):
                for line in db[qi].decode().splitlines():
                    key, score, diag = line.split("\t")[:3]
                    assert int(diag) == 0
                    ids.append(int(key))
                    sc.append(int(score))
                off.append(len(ids))
            out["exp_off_%d" % k] = np.asarray(off, np.uint32)
            out["exp_ids_%d" % k] = np.asarray(ids, np.uint16)
            out["exp_scores_%d" % k] = np.asarray(sc, np.int32)
            # EvalueComputation(tdbr->getAminoAcidDBSize(), subMat, gapOpen, gapExtend), ungappedprefilter.cpp:542
            db_res = int(sum(len(x) for x in (qs if s["same_db"] else ts)))
            ev = pyoracle.RefLib(matrix=MATRICES[s["matrix"]], bit_factor=2.0, score_bias=0.0, gap_open=s["gap_open"], gap_extend=s["gap_extend"],
                                 comp_bias=bool(s["comp_bias"]), db_residues=db_res)
            out["minev_%d" % k] = np.asarray([gc.min_evalue_score(ev.evalue, len(q), s["e"]) for q in qs], np.int32)
            mat = out["mat_" + s["matrix"]]
            for i, q in enumerate(qs):      # every query inside the Gotoh acceptance rule of include/mmgpu.h
                cb = out["qcb_" + s["matrix"]][int(qoff[i]):int(qoff[i + 1])] if s["comp_bias"] else None
                assert spc.rule_accepts(oracle, mat, cb, len(q), s["gap_open"], s["gap_extend"]), (s["name"], i)
            print("%-14s %6d listed pairs, min_evalue_score %d .. %d" % (s["name"], len(ids), out["minev_%d" % k].min(), out["minev_%d" % k].max()))
    out["settings"] = np.frombuffer(json.dumps(SETTINGS).encode(), np.uint8)
    path = os.path.join(HERE, "gapped_scan.npz")
    np.savez_compressed(path, **out)
    G = gc.Golden(path)
    print("recording shows:", gc.check_recording(G, oracle))
    for k in range(len(SETTINGS)):      # the restatement reproduces every recorded list
        for i, ((gi, gs), (wi, ws)) in enumerate(zip(gc.restated_lists(oracle, G, k), G.expected(k))):
            assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (SETTINGS[k]["name"], i)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
