"""Records tests/golden/tantan_edge_vectors.npz from the REAL reference (oracle/_ref/libmmref.so = lib/tantan/tantan.cpp compiled with
the reference's AVX2 + FMA flags), like make_tantan_golden.py does for tantan_vectors.npz - for the edge sets of tests/tantan_cases.py
(every length 0 .. 70, one planted repeat per period 1 .. 52, the X cases) and for TWO likelihood-ratio tables: ProbabilityMatrix over
VTML80 (the k-mer matrix of a default search) and over BLOSUM62.  Per set S and table T the file holds
    S_res, S_off                     the input
    T_likelihood_ratios              the table [21, 21]
    S_T_probs                        tantan::getProbabilities per letter (float32)
    S_T_masked_09 / _05, S_T_n_09 / _05   Masker::maskSequence's output and count at --mask-prob 0.9f / 0.5f
Run in the build container:  python tests/golden/make_tantan_edge_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pyoracle                                        # noqa: E402
from tests import tantan_cases as tc                               # noqa: E402

TABLES = (("vtml80", "VTML80.out"), ("blosum62", "blosum62.out"))
THRESHOLDS = (("09", float(np.float32(0.9))), ("05", float(np.float32(0.5))))      # Parameters::maskProb is a float


def main():
    out = {}
    sets = tc.all_sets()
    for name, seqs in sets.items():
        out[name + "_res"], out[name + "_off"] = tc.pack(seqs)
    for tname, tfile in TABLES:
        ref = pyoracle.RefPrefilter(kmer_matrix=tfile)
        for name, seqs in sets.items():
            res, off = out[name + "_res"], out[name + "_off"]
            probs = np.zeros(len(res), np.float32)
            for i, t in enumerate(seqs):
                if len(t):
                    probs[int(off[i]):int(off[i + 1])] = ref.tantan_mask(*tc.pack([t]), 0.9)[3]
            out["%s_%s_probs" % (name, tname)] = probs
            for key, thr in THRESHOLDS:
                masked, n, lr, _ = ref.tantan_mask(res, off, thr)
                out["%s_%s_masked_%s" % (name, tname, key)] = masked
                out["%s_%s_n_%s" % (name, tname, key)] = np.uint64(n)
                out[tname + "_likelihood_ratios"] = lr
    path = os.path.join(HERE, "tantan_edge_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote tantan_edge_vectors.npz: %d bytes, %s" % (os.path.getsize(path), ", ".join(
        "%s %d sequences / %d letters" % (k, len(v), sum(len(t) for t in v)) for k, v in sets.items())))


if __name__ == "__main__":
    main()
