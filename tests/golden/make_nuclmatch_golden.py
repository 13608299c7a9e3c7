"""Records tests/golden/nuclmatch.npz from the STOCK binary: the database of tests/nuclmatch_cases.py's make_database (A C G T and N)
-> FASTA -> `mmseqs_stock createdb --dbtype 2 --shuffle 0` -> `mmseqs_stock kmermatcher --linclust-version 1 --threads 4` once per
setting below -> the result databases read back with mmseqs2_amd/dbio.py.  Per setting the k and the k-mers per sequence the run
chose (its parameter print-out) are kept beside the lists.  Before anything is written the serial restatement has to reproduce every
recorded list and `strand_ties` has to be empty for every setting: the reference's sorts are not stable, so a database with such a
tie would record an order nobody specified.  If only a tie stands between the two, change make_database's seed.
Run in the build container after __graft_entry__.build():  python tests/golden/make_nuclmatch_golden.py"""
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
from tests import nuclmatch_cases as nc                             # noqa: E402

STOCK = os.path.join(ROOT, "oracle", "_ref", "mmseqs_stock")
BASE = dict(k=0, kmers_per_seq=0, kmers_per_seq_scale=0.2, hash_shift=67, cov_thr=0.8, cov_mode=0, include_only_extendable=0)
SETTINGS = [dict(BASE, name="default"),
            dict(BASE, name="k_18", k=18),
            dict(BASE, name="k_24", k=24),
            dict(BASE, name="k_31", k=31),
            dict(BASE, name="kmer_per_seq_5", kmers_per_seq=5),
            dict(BASE, name="kmer_per_seq_60", kmers_per_seq=60),
            dict(BASE, name="kmer_per_seq_300", kmers_per_seq=300),
            dict(BASE, name="kmer_per_seq_scale_0", kmers_per_seq_scale=0.0),
            dict(BASE, name="kmer_per_seq_scale_05", kmers_per_seq_scale=0.5),
            dict(BASE, name="c_05", cov_thr=0.5),
            dict(BASE, name="c_09", cov_thr=0.9),
            dict(BASE, name="cov_mode_2", cov_mode=2),
            dict(BASE, name="cov_mode_5", cov_mode=5),
            dict(BASE, name="only_extendable", include_only_extendable=1),
            dict(BASE, name="hash_shift_5", hash_shift=5),
            dict(BASE, name="k_18_cov_mode_2_c_05_scale_0", k=18, cov_mode=2, cov_thr=0.5, kmers_per_seq_scale=0.0)]
FASTA_LETTERS = "ACTGN"      # numeric residue -> letter (NucleotideMatrix: A C T G, N and every other letter -> 4)


def write_fasta(path, seqs):
    with open(path, "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (k, "".join(FASTA_LETTERS[int(x)] for x in s)))


def run(*args):
    return subprocess.run([STOCK] + [str(a) for a in args], check=True, stdout=subprocess.PIPE).stdout.decode()


def kmermatcher(db, res, s):
    """-> (k, k-mers per sequence) as the run chose them"""
    args = ["kmermatcher", db, res, "--linclust-version", 1, "--threads", 4, "-v", 3]
    for key, flag in (("k", "-k"), ("kmers_per_seq", "--kmer-per-seq"), ("kmers_per_seq_scale", "--kmer-per-seq-scale"), ("hash_shift", "--hash-shift"),
                      ("cov_thr", "-c"), ("cov_mode", "--cov-mode"), ("include_only_extendable", "--include-only-extendable")):
        if s[key] != BASE[key]:      # (an option at its default is left to the binary: it refuses `--kmer-per-seq 0`)
            args += [flag, s[key]]
    out = run(*args)
    return int(re.findall(r"k-mer length\s+(\d+)", out)[-1]), int(re.findall(r"k-mers per sequence\s+(\d+)", out)[-1])


def read_lists(path, n):
    db = dbio.read_db(path)
    return [[tuple(int(x) for x in line.split("\t")[:3]) for line in db[i].decode().splitlines()] for i in range(n)]


def main():
    seqs, special = nc.make_database()
    out, settings = {}, []
    out["res"], out["off"] = nc.pack(seqs)
    n_res = int(out["off"][-1])
    with tempfile.TemporaryDirectory() as tmp:
        write_fasta(os.path.join(tmp, "db.fasta"), seqs)
        db = os.path.join(tmp, "db")
        run("createdb", os.path.join(tmp, "db.fasta"), db, "--shuffle", 0, "--dbtype", 2, "-v", 1)
        for i, s in enumerate(SETTINGS):
            res = os.path.join(tmp, "res_%d" % i)
            k, per_seq = kmermatcher(db, res, s)
            s = dict(s, k=k, kmers_per_seq=per_seq, requested_k=s["k"], n_residues=n_res)
            settings.append(s)
            lists = read_lists(res, len(seqs))
            flat = [x for l in lists for x in l]
            out["exp_off_%d" % i] = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
            out["exp_id_%d" % i] = np.asarray([x[0] for x in flat], np.uint16)
            out["exp_score_%d" % i] = np.asarray([x[1] for x in flat], np.int16)
            out["exp_diag_%d" % i] = np.asarray([x[2] for x in flat], np.int16)
            par = {key: s[key] for key in ("k", "kmers_per_seq", "kmers_per_seq_scale", "hash_shift", "cov_thr", "cov_mode", "include_only_extendable")}
            ties = nc.strand_ties(seqs, par)
            got = nc.nuclmatch_lists(seqs, par)      # resolved against the reference before any device code exists
            assert got == lists, (s["name"], len(ties), [(a, b) for a, b in zip(got, lists) if a != b][:3])
            assert not ties, (s["name"], ties[:3])
            assert s["requested_k"] or k == capi.nuclmatch_defaults(n_res), s["name"]
            if s["name"] == "kmer_per_seq_300":
                assert nc.last_bin_surplus(seqs[special["last_bin"][0]], par) > 0, "the database holds no sequence with a surplus in its last bin"
            if s["name"] == "default":
                assert tuple(special["tied"]) in nc.runs_where(seqs, par, nc.tied_vote), "the database holds no pair with a tied vote"
                assert nc.runs_where(seqs, par, nc.starts_forward) and nc.runs_where(seqs, par, nc.starts_reverse_and_changes)
            print("%-32s k %2d, %3d k-mers per sequence, %4d lines, %4d with a negative score" % (s["name"], k, per_seq, len(flat), sum(x[1] < 0 for x in flat)))
    out["settings"] = np.frombuffer(json.dumps(settings).encode(), np.uint8)
    out["special"] = np.frombuffer(json.dumps(special).encode(), np.uint8)
    path = os.path.join(HERE, "nuclmatch.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print("wrote", path, size, "bytes; the restatement reproduces all %d recorded settings and none holds a strand tie" % len(settings))


if __name__ == "__main__":
    main()
