"""Check (CPU, against the oracle) of the row-parallel formulation of banded_sw used by the wave traceback kernel
(oracle/bt_rows.py banded_rows) over random alignments at one setting: a quick loop for work on the formulation.  The pinned form
- every (matrix, gap open, gap extend) setting of tests/sw_param_cases.py, band classes counted - is
tests/test_bt_formulation.py.
usage: bt_formulation_check.py [seed [iterations [gap_open gap_extend]]]"""
import sys, os
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Oracle
from oracle.bt_rows import banded_rows
from mmseqs2_amd import workloads as wl


def main():
    orc = Oracle()
    m = dict(np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz")))
    mat = m["blosum62_sw"]
    rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    go, ge = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (11, 1)
    n = bad = 0
    for it in range(int(sys.argv[2]) if len(sys.argv) > 2 else 400):
        L = int(rng.integers(8, 260))
        q = rng.choice(20, size=L, p=wl.BACKGROUND).astype(np.uint8)
        kind = it % 4
        if kind == 0:
            t = wl.mutate(rng, q, float(rng.uniform(0.4, 0.95)), max_indels=6, max_indel_len=25)
        elif kind == 1:     # a long insertion: big |tlen - qlen|, wide first band, band clipped by the target end
            p = int(rng.integers(1, L))
            ins = rng.choice(20, size=int(rng.integers(20, 120)), p=wl.BACKGROUND).astype(np.uint8)
            t = np.concatenate([q[:p], ins, q[p:]])
        elif kind == 2:     # a long deletion
            a = int(rng.integers(1, max(2, L // 2)))
            t = np.concatenate([q[:a], q[min(L - 1, a + int(rng.integers(5, 90))):]])
        else:               # offsetting indels: band 1 must double several times
            t = wl.mutate(rng, q, 0.9, max_indels=4, max_indel_len=15)
        cb = rng.integers(-3, 4, size=L).astype(np.int8) if it % 3 == 0 else None
        r = orc.sw_align(q, cb, t, mat, go, ge, need_start=True, need_bt=True)
        if r["score"] <= 0 or not r["bt"]:
            continue
        qs, qe, ts, te = r["q_start"], r["q_end"], r["t_start"], r["t_end"]
        got = banded_rows(q[qs:qe + 1], None if cb is None else cb[qs:qe + 1], t[ts:te + 1], mat, go, ge, r["score"])
        n += 1
        if got != r["bt"]:
            bad += 1
            if bad < 4:
                print("MISMATCH", it, kind, L, len(t), r["score"], got[:60], r["bt"][:60])
    print("compared %d backtraces, %d differ" % (n, bad))
    return bad


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
