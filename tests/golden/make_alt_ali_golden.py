#!/usr/bin/env python3
"""Generates tests/golden/alt_ali_vectors.npz from the REAL reference (oracle/_ref/libmmref.so, `make -C oracle ref`): the chains
of alternative alignments Alignment::computeAlternativeAlignment (Alignment.cpp:569-601, --alt-ali) walks through - align, overwrite
the target residues [dbStartPos, dbEndPos) with X, align again - for seven multi-domain families.

    python tests/golden/make_alt_ali_golden.py

A family = a random query of length QUERY_LENS[f] and one target made of 2 - 6 copies of the query, each with a quarter of its
residues substituted, separated by 0 - 29 random residues; a family is drawn again until two records of its chain reach THRESHOLD
(the length-1 query never does).  Its chain: record 0 is Matcher::getSWResult (RefLib.sw_align, mode 2,
composition bias on) on the target as it stands; record k + 1 the same call after [t_start, t_end) of record k has been
overwritten with X (20) on top of the earlier masks.  The chain ends with the first record after record 0 whose score is below
THRESHOLD (that record is kept: it is what the loop's checkCriteria sees and rejects) or after MAX_ROUNDS masked records.  The
length-1 query aligns one residue (t_start == t_end): the span is empty, nothing is masked, and record 1 repeats record 0.

Keys of the .npz: qres, qoff, tres, toff (the unmasked targets), cb (the rounded composition bias of the queries, indexed like
qres), chain_off ([families + 1] first record of every family), expect ([records, 7] int32: score, q_end, t_end, q_start,
t_start, word, ident), bt (backtraces joined by newlines), gap_open, gap_extend, threshold, max_rounds, mask_letter."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Oracle, RefLib  # noqa: E402
from mmseqs2_amd import workloads as wl  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
QUERY_LENS = [1, 5, 17, 37, 61, 130, 530]
THRESHOLD, MAX_ROUNDS, MASK_LETTER = 20, 8, 20
SEED = 20261018


def family(rng, qlen):
    q = rng.choice(20, size=qlen, p=wl.BACKGROUND).astype(np.uint8)
    parts = []
    for _ in range(int(rng.integers(2, 7))):
        parts.append(rng.choice(20, size=int(rng.integers(0, 30)), p=wl.BACKGROUND).astype(np.uint8))
        copy = q.copy()
        hit = rng.random(qlen) < 0.25
        copy[hit] = rng.choice(20, size=int(hit.sum()), p=wl.BACKGROUND).astype(np.uint8)
        parts.append(copy)
    parts.append(rng.choice(20, size=int(rng.integers(0, 30)), p=wl.BACKGROUND).astype(np.uint8))
    return q, np.concatenate(parts)


def chain_of(align, t):
    """align(target) -> record dict; the chain described above, on a private copy of t"""
    t = t.copy()
    out = [align(t)]
    for _ in range(MAX_ROUNDS):
        last = out[-1]
        if last["score"] > 0:
            t[last["t_start"]:last["t_end"]] = MASK_LETTER
        out.append(align(t))
        if out[-1]["score"] < THRESHOLD:
            break
    return out


if __name__ == "__main__":
    rng = np.random.default_rng(SEED)
    ref = RefLib("blosum62.out", 2.0, 0.0, gap_open=11, gap_extend=1)      # Alignment.cpp:152: bit factor 2, no score bias
    orc = Oracle()
    mat = ref.matrix()
    qs, ts, cbs, rows, bts, chain_off = [], [], [], [], [], [0]
    for qlen in QUERY_LENS:
        while True:      # (a five-residue query reaches the threshold twice only with heavy letters: drawn until it does)
            q, t = family(rng, qlen)
            ref.sw_set_query(q)
            chain = chain_of(lambda x: ref.sw_align(x, 2), t)
            if qlen == 1 or sum(r["score"] >= THRESHOLD for r in chain) >= 2:
                break
        cb = orc.round_comp_bias(ref.comp_bias(q))
        mine = chain_of(lambda x: orc.sw_align(q, cb, x, mat, 11, 1, need_start=True, need_bt=True), t)
        for a, b in zip(chain, mine):
            # score 0: the reference returns before touching identicalAACnt (uninitialised, ssw_align_private :850-852)
            ident = a["ident"] if a["score"] > 0 else 0
            rows.append([a["score"], a["q_end"], a["t_end"], a["q_start"], a["t_start"], a["word"], ident])
            bts.append(a["bt"])
            if a["score"] > 0:
                assert rows[-1] == [b[k] for k in ("score", "q_end", "t_end", "q_start", "t_start", "word", "ident")] and a["bt"] == b["bt"], (qlen, a, b)
        assert len(chain) == len(mine)
        above = sum(r["score"] >= THRESHOLD for r in chain)
        assert above >= 2 or qlen == 1, (qlen, [r["score"] for r in chain])
        qs.append(q); ts.append(t); cbs.append(cb)
        chain_off.append(len(rows))
        print("query length", qlen, "target length", len(t), "scores", [r["score"] for r in chain], "word", [r["word"] for r in chain])
    e = np.array(rows, np.int32)
    one = e[chain_off[0]:chain_off[1]]
    assert len(one) == 2 and one[0][4] == one[0][2] and (one[0] == one[1]).all(), one      # the empty span: the same alignment again
    assert (e[:, 5] == 0).any() and (e[:, 5] == 1).sum() >= 4      # hits of the uint8 and of the int16 range
    d = dict(gap_open=np.int32(11), gap_extend=np.int32(1), threshold=np.int32(THRESHOLD), max_rounds=np.int32(MAX_ROUNDS),
             mask_letter=np.int32(MASK_LETTER), chain_off=np.array(chain_off, np.int32), expect=e,
             bt=np.frombuffer("\n".join(bts).encode(), np.uint8), cb=np.concatenate(cbs))
    d["qres"], d["qoff"] = wl.seqs_from_list(qs)
    d["tres"], d["toff"] = wl.seqs_from_list(ts)
    path = os.path.join(OUT, "alt_ali_vectors.npz")
    np.savez_compressed(path, **d)
    print("alt_ali_vectors.npz", os.path.getsize(path), "bytes,", len(rows), "records")
