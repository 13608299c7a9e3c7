"""Records tests/golden/ungapped_scan.npz from the STOCK binary: numeric sequences -> FASTA -> `mmseqs_stock createdb --shuffle 0`
-> `mmseqs_stock ungappedprefilter --threads 1` on the CPU (runFilterOnCpu) for every setting below -> the result databases read
back with mmseqs2_amd/dbio.py.  The same-database run scans the query set against itself.  Stored: the sequences, the int8
matrices, the rounded composition bias of every query, the settings and per query the expected (target key, score) list.
The matrices and the float bias come from the reference's own objects (oracle/_ref/libmmref.so); the rounding is
mmgpu_host_round_comp_bias.  Run in the build container after __graft_entry__.build():  python tests/golden/make_ungapped_scan_golden.py"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mmseqs2_amd import capi, dbio                                  # noqa: E402
from oracle import pyoracle                                         # noqa: E402
from tests import ungapped_scan_cases as uc                         # noqa: E402

STOCK = os.path.join(ROOT, "oracle", "_ref", "mmseqs_stock")
MATRICES = {"blosum62": "blosum62.out", "vtml40": "VTML40.out"}

BASE = dict(matrix="blosum62", comp_bias=1, min_score=15, max_seqs=300, cov=0.0, cov_mode=0, same_db=0)
SETTINGS = [dict(BASE, name="base"),
            dict(BASE, name="no_comp_bias", comp_bias=0),
            dict(BASE, name="min_score_60", min_score=60),
            dict(BASE, name="min_score_0", min_score=0),
            dict(BASE, name="max_seqs_10", max_seqs=10),
            dict(BASE, name="max_seqs_1000", max_seqs=1000),
            dict(BASE, name="cov_mode_0", cov=0.8, cov_mode=0),
            dict(BASE, name="cov_mode_1", cov=0.8, cov_mode=1),
            dict(BASE, name="cov_mode_2", cov=0.8, cov_mode=2),
            dict(BASE, name="same_db", same_db=1, min_score=60),
            dict(BASE, name="vtml40", matrix="vtml40")]

QUERY_LENGTHS = [8, 12, 30, 45, 64, 80, 100, 120, 127, 128, 129, 150, 200, 255, 256, 257, 300, 383, 384, 385, 450, 512, 513, 700]
N_TARGETS = 400


def make_sequences():
    rng = np.random.default_rng(20261019)
    qs = [uc.random_seq(rng, n) for n in QUERY_LENGTHS]
    qs[3][10:14] = 20      # a few X in a query
    ts = [uc.random_seq(rng, int(n)) for n in rng.integers(20, 400, N_TARGETS)]
    # targets that hold one and two copies of a query of 60 residues or more: the pair saturates at 255 - B
    for k, qi in enumerate((4, 7, 12, 16)):
        q = qs[qi]
        ts[10 + 2 * k] = np.concatenate([uc.random_seq(rng, 17), q, uc.random_seq(rng, 9)])
        ts[11 + 2 * k] = np.concatenate([q, uc.random_seq(rng, 5), q])
    # homologs at several distances, short targets, a target of X only, a homopolymer
    for k, qi in enumerate((2, 5, 6, 9, 13, 17, 20, 22, 23)):
        ts[40 + 3 * k] = uc.mutate(rng, qs[qi], 0.8)
        ts[41 + 3 * k] = uc.mutate(rng, qs[qi], 0.5)[: max(5, len(qs[qi]) // 2)]
        ts[42 + 3 * k] = np.concatenate([uc.random_seq(rng, 30), uc.mutate(rng, qs[qi], 0.35)])
    for k, n in enumerate((1, 2, 3, 4, 5, 7, 9)):
        ts[100 + k] = uc.random_seq(rng, n)
    ts[110] = np.full(50, 20, np.uint8)
    ts[111] = np.full(40, 0, np.uint8)
    return qs, ts


def write_fasta(path, seqs, letters):
    with open(path, "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (k, "".join(letters[int(x)] for x in s)))


def run(*args):
    subprocess.run([STOCK] + [str(a) for a in args], check=True, stdout=subprocess.DEVNULL)


def round_bias(lib, bias):
    out = np.zeros(len(bias), np.int8)
    b = np.ascontiguousarray(bias, np.float32)
    assert lib.mmgpu_host_round_comp_bias(b.ctypes.data_as(ctypes.c_void_p), len(b), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def main():
    lib = capi.load_library()
    qs, ts = make_sequences()
    (qres, qoff), (tres, toff) = uc.pack(qs), uc.pack(ts)
    out = dict(qres=qres, qoff=qoff, tres=tres, toff=toff)
    letters = None
    for name, fname in MATRICES.items():
        ref = pyoracle.RefLib(matrix=fname, bit_factor=2.0, score_bias=0.0)      # SubstitutionMatrix(file, 2.0, 0.0), ungappedprefilter.cpp:541
        out["mat_" + name] = ref.matrix()
        letters = letters or ref.num2aa()
        assert ref.num2aa() == letters, "the matrices order their letters differently"
        out["qcb_" + name] = np.concatenate([round_bias(lib, ref.comp_bias(q, 1.0)) for q in qs])
    with tempfile.TemporaryDirectory() as tmp:
        write_fasta(os.path.join(tmp, "q.fasta"), qs, letters)
        write_fasta(os.path.join(tmp, "t.fasta"), ts, letters)
        qdb, tdb = os.path.join(tmp, "qdb"), os.path.join(tmp, "tdb")
        run("createdb", os.path.join(tmp, "q.fasta"), qdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        run("createdb", os.path.join(tmp, "t.fasta"), tdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        for k, s in enumerate(SETTINGS):
            res = os.path.join(tmp, "res_%d" % k)
            run("ungappedprefilter", qdb, qdb if s["same_db"] else tdb, res, "--threads", 1, "--comp-bias-corr", s["comp_bias"],
                "--min-ungapped-score", s["min_score"], "--max-seqs", s["max_seqs"], "-c", s["cov"], "--cov-mode", s["cov_mode"],
                "--sub-mat", MATRICES[s["matrix"]], "-v", 1)
            db = dbio.read_db(res)
            nq = len(qs)
            off, ids, sc = [0], [], []
            for qi in range(nq):
                for line in db[qi].decode().splitlines():
                    key, score, diag = line.split("\t")[:3]
                    assert int(diag) == 0
                    ids.append(int(key))
                    sc.append(int(score))
                off.append(len(ids))
            out["exp_off_%d" % k] = np.asarray(off, np.uint32)
            out["exp_ids_%d" % k] = np.asarray(ids, np.uint16)
            out["exp_scores_%d" % k] = np.asarray(sc, np.uint8)
            assert not sc or (0 <= min(sc) and max(sc) <= 255)
            print("%-14s %6d listed pairs" % (s["name"], len(ids)))
    out["settings"] = np.frombuffer(json.dumps(SETTINGS).encode(), np.uint8)
    path = os.path.join(HERE, "ungapped_scan.npz")
    np.savez_compressed(path, **out)
    print("recording shows:", uc.check_recording(uc.Golden(path)))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
