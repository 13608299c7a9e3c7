"""Records tests/golden/rescore.npz from the STOCK binary: the sequences of the ungapped scan's recording (make_ungapped_scan_golden.py's
make_sequences: the 20 amino acids and X, upper case - the reference counts identities on the ASCII letters, so ambiguity codes would
count differently from numeric residues) -> FASTA -> `mmseqs_stock createdb --shuffle 0` -> `mmseqs_stock prefilter --threads 1`
(queries against the targets, and the queries against themselves) -> the two prefilter result databases read back, hand-written
entries appended (wrong diagonals, the extreme valid diagonals, one past each end, a diagonal valid for neither sign, the same
target under several diagonals) and written again as data + .index + .dbtype -> `mmseqs_stock rescorediagonal --threads 1` for every
setting below -> the result databases read back with mmseqs2_amd/dbio.py.
BLOSUM62 only: for another matrix the reference estimates the ungapped ALP parameters at run time.
For every --filter-hits setting the reference's data/resources/CovSeqidQscPercMinDiag*.lib is parsed here as parsePrecisionLib
(rescorediagonal.cpp:20-43) parses it; only the resulting threshold is stored.
Run in the build container after __graft_entry__.build():  python tests/golden/make_rescore_golden.py"""
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
from tests import rescore_cases as rc                               # noqa: E402
from tests import ungapped_scan_cases as uc                         # noqa: E402
import make_ungapped_scan_golden as ung                             # noqa: E402

BASE = dict(mode=0, e=0.001, min_seq_id=0.0, seq_id_mode=0, cov=0.0, cov_mode=0, min_aln_len=0, filter_hits=0, sort_results=0, backtrace=0,
            same_db=0)
SETTINGS = [dict(BASE, name="hamming"),
            dict(BASE, name="hamming_sim1", seq_id_mode=1),
            dict(BASE, name="hamming_sim2", seq_id_mode=2),
            dict(BASE, name="hamming_id05", min_seq_id=0.5),
            dict(BASE, name="hamming_id05_sim1", min_seq_id=0.5, seq_id_mode=1),
            dict(BASE, name="hamming_id05_sim2", min_seq_id=0.5, seq_id_mode=2),
            dict(BASE, name="hamming_id09", min_seq_id=0.9),
            dict(BASE, name="hamming_id09_sim1", min_seq_id=0.9, seq_id_mode=1),
            dict(BASE, name="hamming_cov_mode_0", cov=0.8, cov_mode=0),
            dict(BASE, name="hamming_cov_mode_1", cov=0.8, cov_mode=1),
            dict(BASE, name="hamming_cov_mode_2", cov=0.8, cov_mode=2),
            dict(BASE, name="hamming_same_db", seq_id_mode=1, same_db=1),
            dict(BASE, name="subst", mode=1),
            dict(BASE, name="subst_e_10", mode=1, e=10.0),
            dict(BASE, name="subst_e_1e-10", mode=1, e=1e-10),
            dict(BASE, name="subst_filter_cov_mode_0", mode=1, filter_hits=1, min_seq_id=0.5, cov=0.8, cov_mode=0),
            dict(BASE, name="subst_filter_cov_mode_1", mode=1, filter_hits=1, min_seq_id=0.5, cov=0.8, cov_mode=1),
            dict(BASE, name="hamming_filter", mode=0, filter_hits=1, min_seq_id=0.5, cov=0.8, cov_mode=0),
            dict(BASE, name="aln", mode=2),
            dict(BASE, name="aln_e_10", mode=2, e=10.0),
            dict(BASE, name="aln_e_1e-10", mode=2, e=1e-10),
            dict(BASE, name="aln_min_aln_len_30", mode=2, e=10.0, min_aln_len=30),
            dict(BASE, name="aln_backtrace", mode=2, e=10.0, backtrace=1),
            dict(BASE, name="aln_sorted", mode=2, e=10.0, sort_results=1),
            dict(BASE, name="aln_id05_sim1", mode=2, e=10.0, min_seq_id=0.5, seq_id_mode=1),
            dict(BASE, name="aln_cov_mode_0", mode=2, e=10.0, cov=0.8, cov_mode=0),
            dict(BASE, name="aln_filter", mode=2, e=1e-10, filter_hits=1, min_seq_id=0.5, cov=0.8, cov_mode=0),
            dict(BASE, name="aln_same_db", mode=2, same_db=1)]


def precision_threshold(cov_mode, seq_id, cov, precision=0.99):
    """parsePrecisionLib (rescorediagonal.cpp:20-43) over the table the reference compiles in for the coverage mode"""
    fname = "CovSeqidQscPercMinDiag.lib" if cov_mode == 0 else "CovSeqidQscPercMinDiagTargetCov.lib"
    f = np.float32
    int_id = int((seq_id + 0.0001) * 100)
    want_id = f(int_id - int_id % 5) / f(100)
    want_cov = f(int((cov + 0.0001) * 10)) / f(10)
    eps = np.finfo(np.float32).eps
    with open(os.path.join(pyoracle.REFERENCE_ROOT, "data", "resources", fname)) as fh:
        for line in fh:
            v = line.split(" ")
            if abs(f(float(v[0])) - want_cov) < eps and abs(f(float(v[1])) - want_id) < eps and f(float(v[3])) >= precision:
                return float(f(float(v[2])))
    return 0.0


def read_prefilter(path, nq):
    out = []
    db = dbio.read_db(path)
    for qi in range(nq):
        out.append([(int(k), int(s), int(d)) for k, s, d in (line.split("\t")[:3] for line in db[qi].decode().splitlines())])
    return out


def write_result_db(path, entries, dbtype_from):
    """an MMseqs2 database by hand: `path` = the entries, each ended by a NUL; `path.index` = key, offset, length with the NUL;
    `path.dbtype` copied"""
    data, index = b"", []
    for key, lines in enumerate(entries):
        body = "".join("%d\t%d\t%d\n" % x for x in lines).encode() + b"\0"
        index.append("%d\t%d\t%d\n" % (key, len(data), len(body)))
        data += body
    open(path, "wb").write(data)
    open(path + ".index", "w").write("".join(index))
    open(path + ".dbtype", "wb").write(open(dbtype_from + ".dbtype", "rb").read())


def hand_written(qs, ts, lists, same_db):
    """entries appended to the prefilter's lists; a same-database list gains none for the query's own target (an identity hit on a
    wrong diagonal may score 0, and the reference then reads in front of the query)"""
    out = [list(x) for x in lists]

    def add(qi, ti, d):
        assert not (same_db and qi == ti)
        assert -32768 <= d <= 32767
        out[qi].append((ti, 0, d))

    # the homolog planted at 30 random residues into the target: its diagonal, its neighbours, the main diagonal
    pairs = [(5, 7)] if same_db else [(2, 42), (5, 45), (6, 48), (17, 57)]
    for qi, ti in pairs:
        for d in ((0, 1, -1, 17) if same_db else (-30, -29, -31, 0, -3)):
            add(qi, ti, d)
    for qi, ti in ((0, 3), (3, 9), (10, 20), (16, 2), (23, 11)):
        ql, tl = len(qs[qi]), len(ts[ti])
        for d in (0, ql - 1, ql, -(tl - 1), -tl, 30000, -32768, 1, -1):      # extreme valid, one past each end, valid for neither sign
            add(qi, ti, d)
    if not same_db:
        for ti in (100, 101, 104, 110, 111):      # targets of 1, 2 and 5 residues, of X only, a homopolymer
            add(3, ti, 0)
            add(3, ti, 10)
            add(12, ti, -(len(ts[ti]) - 1))
    return out


def main():
    qs, ts = ung.make_sequences()
    (qres, qoff), (tres, toff) = uc.pack(qs), uc.pack(ts)
    ref = pyoracle.RefLib(matrix="blosum62.out", bit_factor=2.0, score_bias=0.0)      # SubstitutionMatrix(file, 2.0, 0.0), rescorediagonal.cpp:88
    out = dict(qres=qres, qoff=qoff, tres=tres, toff=toff, mat_blosum62=ref.matrix())
    letters = ref.num2aa()
    assert set(letters[int(x)] for s in qs + ts for x in s) <= set("ACDEFGHIKLMNPQRSTVWYX")
    settings = []
    with tempfile.TemporaryDirectory() as tmp:
        ung.write_fasta(os.path.join(tmp, "q.fasta"), qs, letters)
        ung.write_fasta(os.path.join(tmp, "t.fasta"), ts, letters)
        qdb, tdb = os.path.join(tmp, "qdb"), os.path.join(tmp, "tdb")
        ung.run("createdb", os.path.join(tmp, "q.fasta"), qdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        ung.run("createdb", os.path.join(tmp, "t.fasta"), tdb, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        pref = {}
        for tag, db, seqs in (("other", tdb, ts), ("same", qdb, qs)):
            raw = os.path.join(tmp, "pref_raw_" + tag)
            ung.run("prefilter", qdb, db, raw, "--threads", 1, "-s", 7.5, "-v", 1)
            lists = hand_written(qs, seqs, read_prefilter(raw, len(qs)), tag == "same")
            pref[tag] = os.path.join(tmp, "pref_" + tag)
            write_result_db(pref[tag], lists, raw)
            out["hit_off_" + tag] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
            out["hit_target_" + tag] = np.asarray([x[0] for l in lists for x in l], np.uint16)
            out["hit_diag_" + tag] = np.asarray([x[2] for l in lists for x in l], np.int16)
            n_pref = sum(len(x) for x in read_prefilter(raw, len(qs)))
            print("%-6s %5d prefilter hits + %d hand-written" % (tag, n_pref, sum(len(x) for x in lists) - n_pref))
        for k, s in enumerate(SETTINGS):
            s = dict(s, effective_mode=capi.rescore_effective_mode(s["mode"], s["filter_hits"]),
                     score_per_col_thr=precision_threshold(s["cov_mode"], s["min_seq_id"], s["cov"]) if s["filter_hits"] else 0.0)
            settings.append(s)
            tag = "same" if s["same_db"] else "other"
            res = os.path.join(tmp, "res_%d" % k)
            ung.run("rescorediagonal", qdb, qdb if s["same_db"] else tdb, pref[tag], res, "--threads", 1, "--rescore-mode", s["mode"],
                    "-e", repr(s["e"]), "--min-seq-id", s["min_seq_id"], "--seq-id-mode", s["seq_id_mode"], "-c", s["cov"],
                    "--cov-mode", s["cov_mode"], "--min-aln-len", s["min_aln_len"], "--filter-hits", s["filter_hits"],
                    "--sort-results", s["sort_results"], "-a", s["backtrace"], "--sub-mat", "blosum62.out", "-v", 1)
            db = dbio.read_db(res)
            off, rows = [0], []
            for qi in range(len(qs)):
                rows += [line.split("\t") for line in db[qi].decode().splitlines()]
                off.append(len(rows))
            out["exp_off_%d" % k] = np.asarray(off, np.uint32)
            out["exp_key_%d" % k] = np.asarray([int(r[0]) for r in rows], np.uint16)
            out["exp_score_%d" % k] = np.asarray([int(r[1]) for r in rows], np.int32)
            if s["effective_mode"] != rc.ALIGNMENT:
                assert all(len(r) == 3 for r in rows)
                out["exp_diag_%d" % k] = np.asarray([int(r[2]) for r in rows], np.int16)
            else:
                assert all(len(r) == (11 if s["backtrace"] else 10) for r in rows)
                out["exp_seqid_%d" % k] = np.asarray([float(r[2]) for r in rows], np.float64)
                out["exp_evalue_%d" % k] = np.asarray([float(r[3]) for r in rows], np.float64)
                out["exp_pos_%d" % k] = np.asarray([[int(x) for x in r[4:10]] for r in rows], np.int32).reshape(-1, 6)
                if s["backtrace"]:
                    assert all(r[10].endswith("M") and r[10][:-1].isdigit() for r in rows)
                    out["exp_bt_%d" % k] = np.asarray([int(r[10][:-1]) for r in rows], np.int32)
            print("%-26s mode %d, %5d lines, score-per-column threshold %g" % (s["name"], s["effective_mode"], len(rows), s["score_per_col_thr"]))
    out["settings"] = np.frombuffer(json.dumps(settings).encode(), np.uint8)
    path = os.path.join(HERE, "rescore.npz")
    np.savez_compressed(path, **out)
    check(rc.Golden(path))
    size, largest = os.path.getsize(path), max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "rescore.npz")
    assert size <= largest, (size, largest)
    print("wrote", path, size, "bytes")


def check(G):
    """the serial restatement and capi's list building reproduce every recorded list; no recorded identity hit has score 0 (the
    reference then reads in front of the query: not a behaviour to pin); no two lines of a sorted list tie on the whole sort key (the
    reference's sort is not stable)"""
    for k, s in enumerate(G.settings):
        ts = G.setting_targets(s)
        tl = np.array([len(t) for t in ts], np.int64)
        kept, rec = rc.golden_records(G, s)
        at = 0
        for qi, hs in enumerate(kept):
            for target, _ in hs:
                assert not (s["same_db"] and int(target) == qi and int(rec[at]["score"]) == 0), (s["name"], qi)
                at += 1
        got = capi.rescore_lists(rec, [len(q) for q in G.queries], kept, tl, int(tl.sum()), s["effective_mode"], identity=G.identity(s), **G.options(s))
        want = G.expected(k)
        rc.assert_lines(got, want, s["effective_mode"], s["name"])
        if s["sort_results"]:
            for lines in want:      # (lines that tie on the whole key must be the same line)
                keys = [(x[3], x[1], x[9], x[0]) if s["effective_mode"] == rc.ALIGNMENT else (abs(x[1]), x[0]) for x in lines]
                assert len(set(keys)) == len(set(zip(keys, lines))), (s["name"], "tied sort keys")
    print("the restatement reproduces all %d recorded settings" % len(G.settings))


if __name__ == "__main__":
    main()
