"""linclust's k-mer matching stage on the CPU: the serial restatement of tests/kmermatch_cases.py reproduces every list the stock
binary's `kmermatcher --linclust-version 1` recorded in tests/golden/kmermatch.npz; capi.kmermatch_defaults chooses the recorded k and
alphabet; the XXH64 restatement gives the recorded hashes; the C-ABI's new symbols; the refusals that need no device."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import kmermatch_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mmgpu_kmermatch_prepare", "mmgpu_kmermatch_run", "mmgpu_kmermatch_fetch", "mmgpu_kmermatch_fetch_device",
               "mmgpu_kmermatch_last_kernel_ms", "mmgpu_kmermatch_free", "mmgpu_kmermatch_rescore_prepare"]


@functools.lru_cache(maxsize=None)
def golden():
    return kc.Golden()


@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_restatement_equals_the_recorded_lists(k):
    G = golden()
    off, rec = kc.kmermatch(G.seqs, G.params(G.settings[k]))
    want_off, want_rec = G.expected(k)
    assert np.array_equal(off, want_off)
    assert rec.tobytes() == want_rec.tobytes()


def test_the_recorded_settings_cover_what_they_should():
    G = golden()
    names = {s["name"]: s for s in G.settings}
    assert (names["default"]["k"], names["default"]["alph_size"]) == (10, 13)
    assert (names["min_seq_id_09"]["k"], names["min_seq_id_09"]["alph_size"]) == (14, 13)
    assert (names["min_seq_id_099"]["k"], names["min_seq_id_099"]["alph_size"]) == (14, 21)
    assert names["k_12"]["k"] == 12 and names["hash_shift_5"]["hash_shift"] == 5
    assert {5, 40, 300} <= {s["kmers_per_seq"] for s in G.settings} and names["default"]["kmers_per_seq"] == 20
    assert {(1, 0.8), (2, 0.8), (5, 0.8)} <= {(s["cov_mode"], s["cov_thr"]) for s in G.settings}
    assert {0.5, 0.9} <= {s["cov_thr"] for s in G.settings if s["cov_mode"] == 0}
    assert names["only_extendable"]["include_only_extendable"] == 1 and names["kmer_per_seq_scale_01"]["kmers_per_seq_scale"] == 0.1
    lens = {len(s) for s in G.seqs}
    for s in G.settings:      # k - 1, k, k + 1 residues; 63, 64 and 65 windows
        assert {s["k"] - 1, s["k"], s["k"] + 1} <= lens and {62 + s["k"], 63 + s["k"], 64 + s["k"]} <= lens, s["name"]
        assert s["reduce"][20] == s["alph_size"] - 1 and max(s["reduce"]) == s["alph_size"] - 1
    assert len(G.chains) == 6 and {c["rescore_mode"] for c in G.chains} == {0, 2}


def test_the_database_holds_its_engineered_cases():
    G = golden()
    names = {s["name"]: k for k, s in enumerate(G.settings)}
    sp = G.special
    # the surplus in the last bin, under the setting that runs on it
    par = G.params(G.settings[names["kmer_per_seq_300"]])
    assert kc.last_bin_surplus(G.seqs[sp["last_bin"][0]], par) > 0
    # the pair whose two diagonals collect equally many k-mers: the vote takes the larger diagonal
    par = G.params(G.settings[names["min_seq_id_099"]])
    rep, member = sp["tied"]
    assert (rep, member) in kc.tied_diagonal_pairs(G.seqs, par)
    off, rec = G.expected(names["min_seq_id_099"])
    line = [r for r in rec[int(off[rep]):int(off[rep + 1])] if int(r["id"]) == member]
    diags = sorted(d for a, b, d in kc.group(kc.extract(G.seqs, par), par) if (a, b) == (rep, member))
    assert len(line) == 1 and line[0]["diagonal"].astype(np.int16) == max(diags) and len(set(diags)) >= 2
    # exact duplicates meet: the first is the representative of the others; the ones shorter than k through the identity record alone
    off, rec = G.expected(names["default"])
    for group in (sp["duplicates"], sp["short_duplicates"]):
        got = rec[int(off[group[0]]):int(off[group[0] + 1])]["id"].tolist()
        assert got[0] == group[0] and set(group[1:]) <= set(got[1:])
    a, b = sp["short_duplicates"]
    assert rec[int(off[a]):int(off[a + 1])][1].tolist()[:3] == (b, 1, 0)
    # equal lengths: the smaller id represents
    a, b = sp["equal_length"]
    assert len(G.seqs[a]) == len(G.seqs[b]) and b in rec[int(off[a]):int(off[a + 1])]["id"].tolist() and off[b + 1] - off[b] == 1
    # a sequence whose every window holds an X has only its identity record
    s = G.seqs[sp["all_x"][0]]
    assert len(kc.windows(np.asarray(par["reduce"], np.uint8)[s], 10, 21)[0]) == 0 and len(s) > 14


def test_defaults_choose_the_recorded_k_and_alphabet():
    G = golden()
    seen = 0
    for s in G.settings:
        if s["requested_k"]:
            continue
        assert capi.kmermatch_defaults(s["min_seq_id"], s["n_residues"]) == (s["k"], s["alph_size"]), s["name"]
        seen += 1
    assert seen >= 10
    assert capi.kmermatch_defaults(0.0, 10 ** 12)[0] == int(np.log(np.float32(10 ** 12)) / np.log(8.7)) == 12
    assert capi.kmermatch_defaults(0.8995, 1000) == (14, 13) and capi.kmermatch_defaults(0.898, 1000) == (10, 13)


def test_xxh64_restatement_gives_the_recorded_hashes():
    G = golden()
    assert len(G.hash_triples) >= 8
    for value, seed, want in G.hash_triples.tolist():
        assert kc.xxh64_u64(int(value), int(seed)) == int(want)
    for seed in {int(t[1]) for t in G.hash_triples.tolist()}:
        pick = G.hash_triples[G.hash_triples[:, 1] == seed]
        assert np.array_equal(kc.xxh64_u64_array(pick[:, 0], seed), pick[:, 2])
    # the seed enters the hash
    assert kc.xxh64_u64(0, 0) != kc.xxh64_u64(0, 1)


def test_symbols_declared_listed_exported_and_answered_by_the_client():
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmgpu_[a-z0-9_]+)\s*\(", hdr))
    L = capi.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in capi.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert {s for s in declared if s.startswith("mmgpu_kmermatch_")} == set(NEW_SYMBOLS)
    client = ctypes.CDLL(os.path.join(os.path.dirname(capi.library_path()), "libmmgpu_client.so"))
    b = ctypes.c_void_p(1)
    assert client.mmgpu_kmermatch_prepare(None, None, ctypes.byref(b)) == -4 and b.value is None
    assert client.mmgpu_kmermatch_run(None, None) == -4
    assert client.mmgpu_kmermatch_fetch(None, None, None, None, None) == -4
    assert client.mmgpu_kmermatch_fetch_device(None, None, None, None) == -4
    assert client.mmgpu_kmermatch_last_kernel_ms(None, None, None) == -4
    b = ctypes.c_void_p(1)
    assert client.mmgpu_kmermatch_rescore_prepare(None, None, None, ctypes.byref(b)) == -4 and b.value is None
    client.mmgpu_kmermatch_free.restype = None
    client.mmgpu_kmermatch_free(None, None)


def test_mirrors_have_the_c_sizes(tmp_path):
    fields = [("mmgpu_kmermatch_params", f, getattr(capi.KmermatchParams, f).offset) for f, _ in capi.KmermatchParams._fields_]
    fields += [("mmgpu_kmermatch_counts", f, getattr(capi.KmermatchCounts, f).offset) for f, _ in capi.KmermatchCounts._fields_]
    sizes = [("mmgpu_kmermatch_params", ctypes.sizeof(capi.KmermatchParams)), ("mmgpu_kmermatch_counts", ctypes.sizeof(capi.KmermatchCounts)),
             ("mmgpu_pf_hit", kc.HIT_DTYPE.itemsize)]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmgpu.h"\nint main(void) {\n'
           + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in sizes)
           + "".join('    printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, f, _ in fields) + "    return 0;\n}\n")
    c = tmp_path / "sizes.c"
    c.write_text(src)
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines())
    for n, size in sizes:
        assert int(got[n]) == size, n
    for n, f, off in fields:
        assert int(got["%s.%s" % (n, f)]) == off, (n, f)
    assert kc.HIT_DTYPE == capi.PF_HIT_DTYPE


def test_refusals_that_need_no_device():
    """the parameters are judged before the context is looked at"""
    L = capi.load_library()

    def prepare(**change):
        b = ctypes.c_void_p(1)
        rc = L.mmgpu_kmermatch_prepare(None, ctypes.byref(capi.kmermatch_params(dict(kc.identity_params(), **change))), ctypes.byref(b))
        assert b.value is None
        return rc, (L.mmgpu_last_error() or b"").decode()

    rc, msg = prepare(cov_mode=6)
    assert rc == -4 and "cov_mode" in msg
    rc, msg = prepare(cov_mode=-1)
    assert rc == -4 and "cov_mode" in msg
    rc, msg = prepare(k=15)      # 20^15 > 2^63
    assert rc == -4 and "2^63" in msg
    rc, msg = prepare(k=18, alph_size=13, reduce=[min(i, 12) for i in range(21)])      # 12^18 > 2^63, 12^17 < 2^63
    assert rc == -4 and "2^63" in msg
    assert prepare(k=14)[0] == -1 and prepare(k=17, alph_size=13, reduce=[min(i, 12) for i in range(21)])[0] == -1      # fine: only the context is missing
    assert prepare(k=0)[0] == -1 and prepare(k=33)[0] == -1 and prepare(kmers_per_seq=0)[0] == -1 and prepare(alph_size=22)[0] == -1
    assert prepare(alph_size=13)[0] == -1      # reduce holds 20 > 12
    assert L.mmgpu_kmermatch_prepare(None, None, None) == -1
    assert L.mmgpu_kmermatch_run(None, None) == -1 and L.mmgpu_kmermatch_fetch(None, None, None, None, None) == -1
    assert L.mmgpu_kmermatch_rescore_prepare(None, None, None, None) == -1
