"""Records tests/golden/kmermatch.npz from the STOCK binary: the database of tests/kmermatch_cases.py's make_database (the 20 amino
acids and X, upper case) -> FASTA -> `mmseqs_stock createdb --shuffle 0` -> `mmseqs_stock kmermatcher --linclust-version 1
--threads 4` once per setting below -> the result databases read back with mmseqs2_amd/dbio.py.  Per setting the k and the alphabet
size the run chose (its parameter print-out) and the reduction table (its "Reduced amino acid alphabet" line: group i holds the
letters that map to reduced residue i; only the 21 numbers are stored) are kept beside the lists.  For three settings
`mmseqs_stock rescorediagonal` (modes 0 and 2, -c 0.8 --min-seq-id 0.5, the database against itself) is run over the recorded
result: the chain fixture.  A handful of (k-mer index, seed, hash) triples of the restatement's XXH64 are stored; the list parity
below is what vouches for them.
Run in the build container after __graft_entry__.build():  python tests/golden/make_kmermatch_golden.py"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mmseqs2_amd import capi, dbio                                  # noqa: E402
from oracle import pyoracle                                         # noqa: E402
from tests import kmermatch_cases as kc                             # noqa: E402

STOCK = os.path.join(ROOT, "oracle", "_ref", "mmseqs_stock")
BASE = dict(min_seq_id=0.0, k=0, kmers_per_seq=0, kmers_per_seq_scale=0.0, hash_shift=67, cov_thr=0.8, cov_mode=0, include_only_extendable=0)
SETTINGS = [dict(BASE, name="default"),
            dict(BASE, name="min_seq_id_09", min_seq_id=0.9),
            dict(BASE, name="min_seq_id_099", min_seq_id=0.99),
            dict(BASE, name="k_12", k=12),
            dict(BASE, name="kmer_per_seq_5", kmers_per_seq=5),
            dict(BASE, name="kmer_per_seq_40", kmers_per_seq=40),
            dict(BASE, name="kmer_per_seq_300", kmers_per_seq=300),
            dict(BASE, name="kmer_per_seq_scale_01", kmers_per_seq_scale=0.1),
            dict(BASE, name="c_05", cov_thr=0.5),
            dict(BASE, name="c_09", cov_thr=0.9),
            dict(BASE, name="cov_mode_1", cov_mode=1),
            dict(BASE, name="cov_mode_2", cov_mode=2),
            dict(BASE, name="cov_mode_5", cov_mode=5),
            dict(BASE, name="only_extendable", include_only_extendable=1),
            dict(BASE, name="hash_shift_5", hash_shift=5),
            dict(BASE, name="k_12_cov_mode_1_c_05", k=12, cov_mode=1, cov_thr=0.5)]
CHAIN_SETTINGS = ["default", "min_seq_id_099", "kmer_per_seq_300"]
CHAIN_RUNS = [dict(rescore_mode=0, cov=0.8, min_seq_id=0.5), dict(rescore_mode=2, cov=0.8, min_seq_id=0.5)]


def write_fasta(path, seqs, letters):
    with open(path, "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (k, "".join(letters[int(x)] for x in s)))


def run(*args):
    return subprocess.run([STOCK] + [str(a) for a in args], check=True, stdout=subprocess.PIPE).stdout.decode()


def kmermatcher(db, res, s):
    """-> (k, alphabet size, reduce[21] or None for the full alphabet) as the run chose them"""
    args = ["kmermatcher", db, res, "--linclust-version", 1, "--threads", 4, "-v", 3]
    for key, flag in (("min_seq_id", "--min-seq-id"), ("k", "-k"), ("kmers_per_seq", "--kmer-per-seq"), ("kmers_per_seq_scale", "--kmer-per-seq-scale"),
                      ("hash_shift", "--hash-shift"), ("cov_thr", "-c"), ("cov_mode", "--cov-mode"),
                      ("include_only_extendable", "--include-only-extendable")):
        if s[key] != BASE[key]:      # (an option at its default is left to the binary: it refuses `--kmer-per-seq 0`)
            args += [flag, s[key]]
    out = run(*args)
    k = int(re.findall(r"k-mer length\s+(\d+)", out)[-1])
    alph = int(re.findall(r"Alphabet size\s+aa:(\d+)", out)[-1])
    per_seq = int(re.findall(r"k-mers per sequence\s+(\d+)", out)[-1])
    groups = re.findall(r"Reduced amino acid alphabet: (.*)", out)
    return k, alph, per_seq, (groups[-1] if groups else None)


def reduce_table(line, letters):
    """"(A S T) (C) ... (X)" -> reduce[full numeric residue]"""
    groups = [g.split() for g in re.findall(r"\(([^)]*)\)", line)]
    table = []
    for r in range(21):
        hit = [i for i, g in enumerate(groups) if letters[r] in g]
        assert len(hit) == 1, (letters[r], line)
        table.append(hit[0])
    assert table[20] == len(groups) - 1      # X is the last reduced letter
    return table


def read_lists(path, n):
    db = dbio.read_db(path)
    return [[tuple(int(x) for x in line.split("\t")[:3]) for line in db[i].decode().splitlines()] for i in range(n)]


def main():
    ref = pyoracle.RefLib(matrix="blosum62.out", bit_factor=2.0, score_bias=0.0)
    letters = ref.num2aa()
    out, settings, chains = {}, [], []
    with tempfile.TemporaryDirectory() as tmp:
        # the 13-letter table does not depend on the database: a first run on two sequences tells it to the database generator
        rng = np.random.default_rng(1)
        write_fasta(os.path.join(tmp, "boot.fasta"), [kc.random_seq(rng, 50) for _ in range(2)], letters)
        run("createdb", os.path.join(tmp, "boot.fasta"), os.path.join(tmp, "boot"), "--shuffle", 0, "--dbtype", 1, "-v", 1)
        _, alph, _, line = kmermatcher(os.path.join(tmp, "boot"), os.path.join(tmp, "boot_res"), BASE)
        assert alph == 13
        seqs, special = kc.make_database(reduce_table(line, letters))
        assert set(letters[int(x)] for s in seqs for x in s) <= set("ACDEFGHIKLMNPQRSTVWYX")
        out["res"], out["off"] = kc.pack(seqs)
        n_res = int(out["off"][-1])
        write_fasta(os.path.join(tmp, "db.fasta"), seqs, letters)
        db = os.path.join(tmp, "db")
        run("createdb", os.path.join(tmp, "db.fasta"), db, "--shuffle", 0, "--dbtype", 1, "-v", 1)
        triples = []
        for i, s in enumerate(SETTINGS):
            res = os.path.join(tmp, "res_%d" % i)
            k, alph, per_seq, line = kmermatcher(db, res, s)
            s = dict(s, k=k, alph_size=alph, kmers_per_seq=per_seq, reduce=reduce_table(line, letters) if alph != 21 else list(range(21)),
                     requested_k=s["k"], n_residues=n_res)
            assert (line is None) == (alph == 21)
            settings.append(s)
            lists = read_lists(res, len(seqs))
            flat = [x for l in lists for x in l]
            out["exp_off_%d" % i] = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
            out["exp_id_%d" % i] = np.asarray([x[0] for x in flat], np.uint16)
            out["exp_score_%d" % i] = np.asarray([x[1] for x in flat], np.int16)
            out["exp_diag_%d" % i] = np.asarray([x[2] for x in flat], np.int16)
            par = {key: s[key] for key in ("k", "alph_size", "reduce", "kmers_per_seq", "kmers_per_seq_scale", "hash_shift", "cov_thr",
                                           "cov_mode", "include_only_extendable")}
            got = kc.kmermatch_lists(seqs, par)      # resolved against the reference before any device code exists
            assert got == lists, (s["name"], [(a, b) for a, b in zip(got, lists) if a != b][:3])
            assert (k, alph) == capi.kmermatch_defaults(s["min_seq_id"], n_res) or s["requested_k"], s["name"]
            if s["name"] == "kmer_per_seq_300":
                assert kc.last_bin_surplus(seqs[special["last_bin"][0]], par) > 0, "the database holds no sequence with a surplus in its last bin"
            if s["name"] == "min_seq_id_099":
                assert tuple(special["tied"]) in kc.tied_diagonal_pairs(seqs, par), "the database holds no pair with tied diagonals"
            red = np.asarray(par["reduce"], np.uint8)[seqs[150 + i]]
            idx = kc.windows(red, k, alph)[1][:2]
            triples += [(int(x), s["hash_shift"], kc.xxh64_u64(int(x), s["hash_shift"])) for x in idx]
            print("%-24s k %2d, %2d letters, %4d lines" % (s["name"], k, alph, len(flat)))
            if s["name"] not in CHAIN_SETTINGS:
                continue
            for c in CHAIN_RUNS:
                rr = os.path.join(tmp, "chain_%d" % len(chains))
                run("rescorediagonal", db, db, res, rr, "--threads", 1, "--rescore-mode", c["rescore_mode"], "-c", c["cov"], "--min-seq-id",
                    c["min_seq_id"], "--sub-mat", "blosum62.out", "-v", 1)
                rdb = dbio.read_db(rr)
                off, rows = [0], []
                for qi in range(len(seqs)):
                    rows += [line.split("\t") for line in rdb[qi].decode().splitlines()]
                    off.append(len(rows))
                j = len(chains)
                out["chain_off_%d" % j] = np.asarray(off, np.uint32)
                out["chain_key_%d" % j] = np.asarray([int(r[0]) for r in rows], np.uint16)
                out["chain_score_%d" % j] = np.asarray([int(r[1]) for r in rows], np.int32)
                if c["rescore_mode"] != 2:
                    out["chain_diag_%d" % j] = np.asarray([int(r[2]) for r in rows], np.int16)
                else:
                    out["chain_seqid_%d" % j] = np.asarray([float(r[2]) for r in rows], np.float64)
                    out["chain_evalue_%d" % j] = np.asarray([float(r[3]) for r in rows], np.float64)
                    out["chain_pos_%d" % j] = np.asarray([[int(x) for x in r[4:10]] for r in rows], np.int32).reshape(-1, 6)
                chains.append(dict(c, setting=i, name=s["name"]))
                print("    chain: rescore mode %d, %4d lines" % (c["rescore_mode"], len(rows)))
    out["mat_blosum62"] = ref.matrix()
    out["hash_triples"] = np.asarray(triples, np.uint64)
    out["settings"] = np.frombuffer(json.dumps(settings).encode(), np.uint8)
    out["special"] = np.frombuffer(json.dumps(special).encode(), np.uint8)
    out["chains"] = np.frombuffer(json.dumps(chains).encode(), np.uint8)
    path = os.path.join(HERE, "kmermatch.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print("wrote", path, size, "bytes; the restatement reproduces all %d recorded settings" % len(settings))


if __name__ == "__main__":
    main()
