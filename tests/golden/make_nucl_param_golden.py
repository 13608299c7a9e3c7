#!/usr/bin/env python3
"""Generates tests/golden/nucl_param_vectors.npz from the REAL reference (oracle/_ref/libmmref.so, `make -C oracle ref`): for
every setting of tests/nucl_param_cases.py NUCL_PARAM_SETS the matrix text this script writes, the int8 matrix the reference
derives from it, and the reference's BandedNucleotideAligner::align results for the cases of the shared generator (plus the
--wrapped-scoring cases for WRAPPED_SETS).

    python tests/golden/make_nucl_param_golden.py                       the whole file
    python tests/golden/make_nucl_param_golden.py --setting KEY --out F   one setting into F (what the parent runs per setting)

Every setting is recorded by a child process: the reference's e-value set-up aborts the process for gap costs it has no
statistics for, and the parent then names the setting instead of dying with it.  The archive is written with fixed time
stamps, so the same inputs give the same bytes.

Keys of the .npz: "<set key>/<name>" with name in costs (open, extend, z-drop), mat, reverse, serialized, qres, qoff, tres, toff,
meta ([n, 4]: diagonal, reverse, past-end letter of the query, of the target), expected ([n, 7]: score, q_start, q_end, t_start,
t_end, ident, cigar length), bt, boff; the wrapped cases under "<set key>/w_<name>"."""
import argparse
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from tests import nucl_param_cases as npc  # noqa: E402

MIN_LONGER_THAN_100, MIN_LONGER_THAN_1000 = 8, 2
MAX_BYTES = 300 * 1000


def save_npz(path, d):
    """np.savez_compressed with fixed time stamps: byte-equal archives from equal arrays"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in d.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def letters(a):
    return "".join(po.NUCL_LETTERS[int(x)] for x in a)


def record(ref, cases, wrapped):
    exp, bts = [], []
    for q, t, diag, reverse, pq, pt in cases:
        ref.set_query(letters(q), pq)
        r, bt = ref.align(letters(t), diag, reverse, pt, wrapped=wrapped)
        exp.append(r)
        bts.append(bt)
    return exp, bts


def one_set(key):
    index = [s[0] for s in npc.NUCL_PARAM_SETS].index(key)
    _, go, ge, zdrop, mkey = npc.NUCL_PARAM_SETS[index]
    text = npc.serialized(mkey)
    ref = po.RefNucl(gap_open=go, gap_extend=ge, zdrop=zdrop, serialized=text)
    mat, rl = ref.matrix(), ref.reverse_lookup()
    d = {key + "/costs": np.array([go, ge, zdrop], np.int32), key + "/mat": mat, key + "/reverse": rl,
         key + "/serialized": np.frombuffer(text, np.uint8)}
    cases = npc.generate_cases(index, rl)
    exp, bts = record(ref, cases, False)
    n100, n1000 = sum(len(b) > 100 for b in bts), sum(len(b) > 1000 for b in bts)
    print("%-20s %d/%d/%d matrix %s: %d cases, %d alignments longer than 100 letters, %d longer than 1000" %
          (key, go, ge, zdrop, mat.tolist(), len(cases), n100, n1000), flush=True)
    assert len(cases) == 120
    assert n100 >= MIN_LONGER_THAN_100 and n1000 >= MIN_LONGER_THAN_1000, (key, n100, n1000)
    npc.pack_cases(d, key + "/", cases, exp, bts)
    if key in npc.WRAPPED_SETS:
        wcases = npc.generate_wrapped_cases(index, rl)
        wexp, wbts = record(ref, wcases, True)
        npc.pack_cases(d, key + "/w_", wcases, wexp, wbts)
        print("%-20s %d wrapped cases" % (key, len(wcases)), flush=True)
    ref.close()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting")
    ap.add_argument("--out", default=npc.FIXTURE)
    a = ap.parse_args()
    if a.setting:
        save_npz(a.out, one_set(a.setting))
        return 0
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, go, ge, zdrop, mkey in npc.NUCL_PARAM_SETS:
            part = os.path.join(tmp, key + ".npz")
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--setting", key, "--out", part])
            if rc != 0:
                print("setting %s (%d/%d/%d, matrix %s): the recording process ended with status %d" % (key, go, ge, zdrop, mkey, rc))
                return 1
            with np.load(part) as z:
                for name in z.files:
                    d[name] = z[name]
    save_npz(a.out, d)
    size = os.path.getsize(a.out)
    print(os.path.basename(a.out), size, "bytes")
    assert size < MAX_BYTES, size
    return 0


if __name__ == "__main__":
    sys.exit(main())
