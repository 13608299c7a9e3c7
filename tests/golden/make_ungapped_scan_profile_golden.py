"""Records tests/golden/ungapped_scan_profile.npz from the STOCK binary: `mmseqs_stock ungappedprefilter --threads 1` on the CPU
(runFilterOnCpu) with PROFILE query databases.

Group A, real profiles: a family-structured query set and its targets -> FASTA -> `createdb --shuffle 0` -> `search -a` ->
`result2profile`, all with the stock binary; the profile database is read back with mmseqs2_amd/dbio.py and its entries
([L][25] int8) are stored.  Settings: base, --min-ungapped-score 0, --max-seqs 10, -c 0.8 --cov-mode 0, --comp-bias-corr 0 and 1.
Group B, crafted entries: a profile database written by hand (data file: L * 25 bytes + NUL per entry; .index; .dbtype = 2) from
entries made like tests/test_profile_query.make_entry, at the lengths of make_ungapped_scan_golden.QUERY_LENGTHS, with three
saturating entries, one entry holding a single -128 byte (B = 32) and one whose lowest score is -1; base setting only.  If the stock
binary's lists for the hand-written database differ from the numpy restatement (which group A pins), group B is NOT stored and the
script says so.

Every entry's alignment profile is derived in numpy and compared with what the reference's own Sequence::mapProfile gives
(oracle/_ref/libmmref.so); every recorded list is compared with the numpy restatement (tests/ungapped_scan_profile_cases.py).
Run in the build container after __graft_entry__.build():  python tests/golden/make_ungapped_scan_profile_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from mmseqs2_amd import capi, dbio                                  # noqa: E402
from oracle import pyoracle                                         # noqa: E402
from tests import ungapped_scan_cases as uc                         # noqa: E402
from tests import ungapped_scan_profile_cases as upc                # noqa: E402
import make_ungapped_scan_golden as seq_golden                      # noqa: E402

STOCK = seq_golden.STOCK
BASE = dict(min_score=15, max_seqs=300, cov=0.0, cov_mode=0, comp_bias=1)
SETTINGS_A = [dict(BASE, group="A", name="base"),
              dict(BASE, group="A", name="min_score_0", min_score=0),
              dict(BASE, group="A", name="max_seqs_10", max_seqs=10),
              dict(BASE, group="A", name="cov_mode_0", cov=0.8, cov_mode=0),
              dict(BASE, group="A", name="comp_bias_0", comp_bias=0),
              dict(BASE, group="A", name="comp_bias_1", comp_bias=1)]
SETTINGS_B = [dict(BASE, group="B", name="base")]

A_QUERY_LENGTHS = [100, 127, 129, 200, 255, 257, 400, 511, 513, 700]      # both sides of 128, 256 and 512; one above 512
A_TARGETS = 300
B_TARGETS = 120


def group_a_sequences():
    """ten family founders and their targets: members at several distances (what `search` aligns and `result2profile` turns into
    the profile), 12 targets that hold the whole of query 0 and 12 that hold query 1 (lists cut inside the class of the cap), one
    and two copies of queries 2 and 3, random sequences"""
    rng = np.random.default_rng(20261019)
    qs = [uc.random_seq(rng, n) for n in A_QUERY_LENGTHS]
    ts = [uc.random_seq(rng, int(n)) for n in rng.integers(20, 400, A_TARGETS)]
    at = 0
    for qi, q in enumerate(qs):
        for keep in (0.9, 0.8, 0.7, 0.6, 0.5, 0.45):
            lo = int(rng.integers(0, max(1, len(q) - 380)))
            seg = q[lo:lo + min(len(q), int(rng.integers(200, 380)))]
            ts[at] = np.concatenate([uc.random_seq(rng, int(rng.integers(0, 12))), uc.mutate(rng, seg, keep)])
            at += 1
    for qi in (0, 1):
        for _ in range(12):
            ts[at] = np.concatenate([uc.random_seq(rng, int(rng.integers(1, 40))), qs[qi], uc.random_seq(rng, int(rng.integers(1, 40)))])
            at += 1
    for qi in (2, 3):
        ts[at] = np.concatenate([uc.random_seq(rng, 17), qs[qi], uc.random_seq(rng, 9)])
        ts[at + 1] = np.concatenate([qs[qi][:150], uc.random_seq(rng, 5), qs[qi][:150]])
        at += 2
    ts[at] = np.full(50, 20, np.uint8)      # X only
    assert at < A_TARGETS and max(len(t) for t in ts) <= 400
    return qs, ts


def group_b_entries(mat):
    """crafted entries at the sequence recording's query lengths and their targets"""
    rng = np.random.default_rng(20261020)
    lengths = seq_golden.QUERY_LENGTHS
    entries, cons = [], []
    for k, n in enumerate(lengths):
        if n == 150:
            e, c = upc.entry_with_one_minus_128(rng, mat, n)
        elif n == 200:
            e, c = upc.entry_with_lowest_minus_1(rng, mat, n)
        else:
            e, c = upc.make_entry(rng, mat, n, sharp=1.0 if n in (100, 120, 255) else 0.6)
        entries.append(e)
        cons.append(c)
    ts = [uc.random_seq(rng, int(n)) for n in rng.integers(20, 300, B_TARGETS)]
    at = 0
    for n in (100, 120, 255, 150, 200):      # one and two copies of the consensus: the pair saturates
        c = cons[lengths.index(n)]
        ts[at] = np.concatenate([uc.random_seq(rng, 11), c, uc.random_seq(rng, 7)])
        ts[at + 1] = np.concatenate([c[:100], uc.random_seq(rng, 3), c[:100]])
        at += 2
    for k in range(len(lengths)):      # homologs of every entry's consensus, whole and in part
        c = cons[k]
        ts[at] = uc.mutate(rng, c, 0.7)[:290]
        ts[at + 1] = np.concatenate([uc.random_seq(rng, 20), uc.mutate(rng, c, 0.5)[:len(c) // 2 + 3]])[:290]
        at += 2
    ts[at] = np.full(40, 20, np.uint8)
    assert at < B_TARGETS
    return entries, ts


def run(*args):
    subprocess.run([STOCK] + [str(a) for a in args], check=True, stdout=subprocess.DEVNULL)


def write_profile_db(path, entries):
    """a profile database by hand: DBReader::getSeqLen of a profile entry is (length - 1) / 25"""
    off = 0
    with open(path, "wb") as data, open(path + ".index", "w") as index:
        for key, e in enumerate(entries):
            raw = np.ascontiguousarray(e, np.int8).tobytes() + b"\0"
            data.write(raw)
            index.write("%d\t%d\t%d\n" % (key, off, len(raw)))
            off += len(raw)
    with open(path + ".dbtype", "wb") as fh:
        fh.write(np.int32(2).tobytes())      # Parameters::DBTYPE_HMM_PROFILE


def read_lists(res, nq):
    db = dbio.read_db(res)
    off, ids, sc = [0], [], []
    for qi in range(nq):
        for line in db[qi].decode().splitlines():
            key, score, diag = line.split("\t")[:3]
            assert int(diag) == 0
            ids.append(int(key))
            sc.append(int(score))
        off.append(len(ids))
    assert not sc or (0 <= min(sc) and max(sc) <= 255)
    return np.asarray(off, np.uint32), np.asarray(ids, np.uint16), np.asarray(sc, np.uint8)


def scan(qdb, tdb, res, s):
    run("ungappedprefilter", qdb, tdb, res, "--threads", 1, "--comp-bias-corr", s["comp_bias"], "--min-ungapped-score", s["min_score"],
        "--max-seqs", s["max_seqs"], "-c", s["cov"], "--cov-mode", s["cov_mode"], "-v", 1)


def restated_lists(profs, targets, s):
    tl = np.array([len(t) for t in targets], np.int64)
    out = []
    for p in profs:
        win = capi.coverage_window(s["cov"], s["cov_mode"], p.shape[1], tl)
        out.append(upc.select_list(upc.scores_one_query(p, targets), tl, win, s["min_score"], s["max_seqs"]))
    return out


def lists_equal(rec, want):
    off, ids, sc = (x.astype(np.int64) for x in rec)
    return all(np.array_equal(ids[off[i]:off[i + 1]], wi) and np.array_equal(sc[off[i]:off[i + 1]], ws) for i, (wi, ws) in enumerate(want))


def check_profiles(ref, entries):
    """numpy's alignment profile against the reference's own (Sequence::mapProfile through oracle/_ref/libmmref.so)"""
    profs = [upc.alignment_profile(e) for e in entries]
    for e, p in zip(entries, profs):
        assert np.array_equal(ref.sw_set_profile_query(e)[0], p)
    return profs


def main():
    ref = pyoracle.RefLib(comp_bias=False)
    letters = ref.num2aa()
    mat = np.load(os.path.join(HERE, "matrices.npz"))["blosum62_sw"]
    out, settings = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        def path(name):
            return os.path.join(tmp, name)

        # ---- group A ----
        qs, ts = group_a_sequences()
        seq_golden.write_fasta(path("aq.fasta"), qs, letters)
        seq_golden.write_fasta(path("at.fasta"), ts, letters)
        run("createdb", path("aq.fasta"), path("aq"), "--shuffle", 0, "--dbtype", 1, "-v", 1)
        run("createdb", path("at.fasta"), path("at"), "--shuffle", 0, "--dbtype", 1, "-v", 1)
        run("search", path("aq"), path("at"), path("ares0"), path("atmp0"), "-s", 5.7, "-a", "--threads", 1, "-v", 1)
        run("result2profile", path("aq"), path("at"), path("ares0"), path("aprof"), "--threads", 1, "-v", 1)
        assert dbio.dbtype(path("aprof")) & 0x7FFFFFFF == 2
        db = dbio.read_db(path("aprof"))
        entries = [np.frombuffer(db[k], np.int8).reshape(-1, upc.ENTRY_BYTES).copy() for k in range(len(qs))]
        assert [len(e) for e in entries] == A_QUERY_LENGTHS
        profs = check_profiles(ref, entries)
        out.update(A_entries=np.concatenate(entries), A_eoff=np.cumsum([0] + [len(e) for e in entries]).astype(np.uint32))
        out["A_tres"], out["A_toff"] = uc.pack(ts)
        for s in SETTINGS_A:
            res = path("ares_%s" % s["name"])
            scan(path("aprof"), path("at"), res, s)
            rec = read_lists(res, len(qs))
            assert lists_equal(rec, restated_lists(profs, ts, s)), "group A, %s: the restatement differs from the stock binary" % s["name"]
            k = len(settings)
            out["exp_off_%d" % k], out["exp_ids_%d" % k], out["exp_scores_%d" % k] = rec
            settings.append(s)
            print("A %-12s %6d listed pairs" % (s["name"], len(rec[1])))

        # ---- group B ----
        entries, ts = group_b_entries(mat)
        profs = check_profiles(ref, entries)
        assert sorted({upc.bias_of(p) for p in profs})[:1] == [1] and 32 in {upc.bias_of(p) for p in profs}
        seq_golden.write_fasta(path("bt.fasta"), ts, letters)
        run("createdb", path("bt.fasta"), path("bt"), "--shuffle", 0, "--dbtype", 1, "-v", 1)
        write_profile_db(path("bprof"), entries)
        kept_b = True
        for s in SETTINGS_B:
            res = path("bres_%s" % s["name"])
            scan(path("bprof"), path("bt"), res, s)
            rec = read_lists(res, len(entries))
            if not lists_equal(rec, restated_lists(profs, ts, s)):
                kept_b = False
                print("group B: the stock binary's lists differ from the restatement - the hand-written database was not read as written; group B is left out")
                break
            k = len(settings)
            out["exp_off_%d" % k], out["exp_ids_%d" % k], out["exp_scores_%d" % k] = rec
            settings.append(s)
            print("B %-12s %6d listed pairs" % (s["name"], len(rec[1])))
        if kept_b:
            out.update(B_entries=np.concatenate(entries), B_eoff=np.cumsum([0] + [len(e) for e in entries]).astype(np.uint32))
            out["B_tres"], out["B_toff"] = uc.pack(ts)
    out["settings"] = np.frombuffer(json.dumps(settings).encode(), np.uint8)
    dest = os.path.join(HERE, "ungapped_scan_profile.npz")
    np.savez_compressed(dest, **out)
    print("recording shows:", upc.check_recording(upc.Golden(dest)))
    print("wrote", dest, os.path.getsize(dest), "bytes")
    assert os.path.getsize(dest) < 400 * 1000


if __name__ == "__main__":
    main()
