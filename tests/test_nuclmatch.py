"""linclust's k-mer matching stage over nucleotides on the CPU: the serial restatement of tests/nuclmatch_cases.py reproduces every
list the stock binary's `kmermatcher --linclust-version 1` recorded in tests/golden/nuclmatch.npz, and none of the recorded settings
holds a strand tie; the reverse complement and the canonical index on small cases written by hand; the engineered cases are in the
database; capi.nuclmatch_defaults chooses the recorded k; the C-ABI's new symbols; the refusals that need no device."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import nuclmatch_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mmgpu_nuclmatch_prepare", "mmgpu_nuclmatch_run", "mmgpu_nuclmatch_fetch", "mmgpu_nuclmatch_fetch_device",
               "mmgpu_nuclmatch_last_kernel_ms", "mmgpu_nuclmatch_free"]
A, C, T, G, N = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def golden():
    return nc.Golden()


def setting(name):
    G_ = golden()
    k = [s["name"] for s in G_.settings].index(name)
    return k, G_.params(G_.settings[k])


@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_restatement_equals_the_recorded_lists(k):
    G_ = golden()
    off, rec = nc.nuclmatch(G_.seqs, G_.params(G_.settings[k]))
    want_off, want_rec = G_.expected(k)
    assert np.array_equal(off, want_off)
    assert rec.tobytes() == want_rec.tobytes()


@pytest.mark.parametrize("k", range(len(golden().settings)), ids=[s["name"] for s in golden().settings])
def test_no_recorded_setting_holds_a_strand_tie(k):
    G_ = golden()
    assert nc.strand_ties(G_.seqs, G_.params(G_.settings[k])) == []


def test_the_recorded_settings_cover_what_they_should():
    G_ = golden()
    names = {s["name"]: s for s in G_.settings}
    assert len(names) == 16 and names["default"]["k"] == 17 and names["default"]["kmers_per_seq"] == 60 and not names["default"]["requested_k"]
    assert {17, 18, 24, 31} == {s["k"] for s in G_.settings} and {5, 60, 300} == {s["kmers_per_seq"] for s in G_.settings}
    assert {0.0, 0.2, 0.5} == {s["kmers_per_seq_scale"] for s in G_.settings} and {0.5, 0.8, 0.9} == {s["cov_thr"] for s in G_.settings}
    assert {0, 2, 5} == {s["cov_mode"] for s in G_.settings} and names["only_extendable"]["include_only_extendable"] == 1
    assert names["hash_shift_5"]["hash_shift"] == 5
    lens = {len(s) for s in G_.seqs}
    assert 20 > min(lens) and max(lens) <= 400 and 200 <= len(G_.seqs) <= 400
    for s in G_.settings:      # k - 1, k, k + 1 residues; 63, 64 and 65 windows
        assert {s["k"] - 1, s["k"], s["k"] + 1} <= lens and {62 + s["k"], 63 + s["k"], 64 + s["k"]} <= lens, s["name"]
    for k in range(len(G_.settings)):      # both orientations are in every recorded result
        score = G_.expected(k)[1]["score"]
        assert (score < 0).sum() >= 10 and (score == 0).sum() > len(G_.seqs)


def test_revcomp_and_canonical_index_on_small_cases():
    assert nc.revcomp([A, A, C, G, N, T]).tolist() == [A, N, C, G, T, T]
    assert nc.revcomp(nc.revcomp([G, A, T, T, A, C, A])).tolist() == [G, A, T, T, A, C, A]
    # ACG = 0b000111 = 7; its reverse complement CGT = 0b011110 = 30: the window is taken as it stands
    assert nc.canonical([A, C, G]) == (7, False)
    assert nc.canonical([C, G, T]) == (7, True)
    # TTT = 0b101010 = 42, AAA = 0: taken as its reverse complement
    assert nc.canonical([T, T, T]) == (0, True)
    # even k: ACGT is its own reverse complement and does not count; AACG is not (CGTT)
    assert nc.canonical([A, C, G, T]) is None and nc.canonical([A, T]) is None and nc.canonical([G, C]) is None
    assert nc.canonical([A, A, C, G]) == (0b00000111, False)
    assert nc.canonical([A, C, N]) is None and nc.canonical([N, N, N]) is None
    # the vectorised walk agrees with it, window by window
    rng = np.random.default_rng(1)
    for k in (1, 2, 4, 7, 16, 17, 24, 31):
        s = nc.random_seq(rng, 90)
        s[40] = N
        s[60:60 + 4] = [A, C, G, T]
        pos, idx, is_rev = nc.windows(s, k)
        want = [(p,) + nc.canonical(s[p:p + k]) for p in range(len(s) - k + 1) if nc.canonical(s[p:p + k]) is not None]
        assert list(zip(pos.tolist(), idx.tolist(), is_rev.tolist())) == want, k
        if k in (2, 4):      # CG at 61 and ACGT at 60 are their own reverse complements
            assert (61 if k == 2 else 60) not in pos.tolist()
    pos, _, _ = nc.windows(np.array([A, C, G, T, A], np.uint8), 4)
    assert pos.tolist() == [1]      # ACGT is dropped, CGTA is not its own reverse complement


def test_stored_strand_bit_and_position():
    """a window taken as its reverse complement stores the position on the other strand and leaves bit 63 clear"""
    s = np.array([T, T, T, T, G], np.uint8)      # TTTT -> AAAA (reverse), TTTG -> CAAA (reverse: 0b01000000 < 0b10101011)
    recs = nc.extract([s], nc.params(k=4, kmers_per_seq=10, scale=0.0))
    assert recs[1:] == [(0, 0, 5 - 0 - 4, 5), (0b01000000, 0, 5 - 1 - 4, 5)]
    recs = nc.extract([nc.revcomp(s)], nc.params(k=4, kmers_per_seq=10, scale=0.0))      # CAAAA: the same k-mers as they stand
    assert recs[1:] == [(0b01000000 | nc.BIT63, 0, 0, 5), (0 | nc.BIT63, 0, 1, 5)]


def test_the_database_holds_its_engineered_cases():
    G_ = golden()
    sp = G_.special
    k_default, par = setting("default")
    off, rec = G_.expected(k_default)

    def line(rep, member):
        hit = [r for r in rec[int(off[rep]):int(off[rep + 1])] if int(r["id"]) == member]
        assert len(hit) == 1, (rep, member)
        return int(hit[0]["score"]), int(hit[0]["diagonal"].astype(np.int16))

    all_runs = {(rep, member): entries for rep, member, entries in nc.runs(nc.group(nc.extract(G_.seqs, par), par))}
    # a run that starts with an as-it-is entry: score 0 and the smallest diagonal, however many entries it has
    rep, rev_first, fwd_first = sp["inversion"]      # (the reverse-complemented second half lies on diagonal -170, the first half on +190)
    entries = all_runs[(rep, fwd_first)]
    assert nc.starts_forward(entries) and any(not e[1] for e in entries) and len(entries) > 5
    assert line(rep, fwd_first) == (0, min(e[0] for e in entries))
    # a run that starts reverse and changes strand: only the leading reverse stretch is voted
    entries = all_runs[(rep, rev_first)]
    assert nc.starts_reverse_and_changes(entries)
    lead = [e for e in entries[:[e[1] for e in entries].index(True)]]
    assert 0 < len(lead) < len(entries) and line(rep, rev_first)[0] == -len(lead)
    # a sequence and its exact reverse complement: the second is the first's member, with a negative score
    a, b = sp["reverse_complement"]
    assert line(a, b)[0] < -10 and line(a, b)[1] == 0
    # a tied vote: the larger diagonal wins
    rep, member = sp["tied"]
    entries = all_runs[(rep, member)]
    assert nc.tied_vote(entries) and not any(e[1] for e in entries)
    cnt = {}
    for d, _ in entries:
        cnt[d] = cnt.get(d, 0) + 1
    assert line(rep, member) == (-len(entries), max(d for d, c in cnt.items() if c == max(cnt.values())))
    # the surplus in the last bin, under the setting that runs on it
    assert nc.last_bin_surplus(G_.seqs[sp["last_bin"][0]], setting("kmer_per_seq_300")[1]) > 0
    # exact duplicates meet, the ones shorter than k through the identity record alone; equal lengths: the smaller id represents
    for group in (sp["duplicates"], sp["short_duplicates"]):
        got = rec[int(off[group[0]]):int(off[group[0] + 1])]["id"].tolist()
        assert got[0] == group[0] and set(group[1:]) <= set(got[1:])
    a, b = sp["short_duplicates"]
    assert len(G_.seqs[a]) < 17 and line(a, b)[1] == 0
    a, b = sp["equal_length"]
    assert len(G_.seqs[a]) == len(G_.seqs[b]) and line(a, b)[0] < 0 and off[b + 1] - off[b] == 1
    # N in every window: only the identity record; a short run of N: a member all the same
    s = G_.seqs[sp["all_n"][0]]
    assert len(nc.windows(s, 17)[0]) == 0 and len(s) > 17
    assert N in G_.seqs[sp["short_run_of_n"][0]].tolist() and len(nc.windows(G_.seqs[sp["short_run_of_n"][0]], 17)[0]) > 100
    # windows that are their own reverse complement, for the even recorded k
    s = G_.seqs[sp["self_complementary"][0]]
    for k in (18, 24):
        assert any(nc.canonical(s[p:p + k]) is None for p in range(len(s) - k + 1))


def test_defaults_choose_the_recorded_k():
    G_ = golden()
    seen = 0
    for s in G_.settings:
        if not s["requested_k"]:
            assert capi.nuclmatch_defaults(s["n_residues"]) == s["k"], s["name"]
            seen += 1
    assert seen >= 10
    assert capi.nuclmatch_defaults(4 ** 18 - 10 ** 7) == 17 and capi.nuclmatch_defaults(1) == 17 and capi.nuclmatch_defaults(4 ** 18) == 18
    for n in (4 ** 19 + 4 ** 18, 10 ** 12, 3 * 10 ** 13):
        assert capi.nuclmatch_defaults(n) == int(float(np.log(np.float32(n))) / float(np.log(4))) > 17
    assert capi.nuclmatch_defaults(10 ** 12) == 19


def test_symbols_declared_listed_exported_and_answered_by_the_client():
    hdr = open(os.path.join(ROOT, "include", "mmgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mmgpu_[a-z0-9_]+)\s*\(", hdr))
    L = capi.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in capi.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert {s for s in declared if s.startswith("mmgpu_nuclmatch_")} == set(NEW_SYMBOLS)
    client = ctypes.CDLL(os.path.join(os.path.dirname(capi.library_path()), "libmmgpu_client.so"))
    b = ctypes.c_void_p(1)
    assert client.mmgpu_nuclmatch_prepare(None, None, ctypes.byref(b)) == -4 and b.value is None
    assert client.mmgpu_nuclmatch_run(None, None) == -4
    assert client.mmgpu_nuclmatch_fetch(None, None, None, None, None) == -4
    assert client.mmgpu_nuclmatch_fetch_device(None, None, None, None) == -4
    assert client.mmgpu_nuclmatch_last_kernel_ms(None, None, None) == -4
    client.mmgpu_nuclmatch_free.restype = None
    client.mmgpu_nuclmatch_free(None, None)


def test_mirror_has_the_c_size_and_offsets(tmp_path):
    fields = [("mmgpu_nuclmatch_params", f, getattr(capi.NuclmatchParams, f).offset) for f, _ in capi.NuclmatchParams._fields_]
    sizes = [("mmgpu_nuclmatch_params", ctypes.sizeof(capi.NuclmatchParams)), ("mmgpu_kmermatch_counts", ctypes.sizeof(capi.KmermatchCounts)),
             ("mmgpu_pf_hit", nc.HIT_DTYPE.itemsize)]
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
    assert len(fields) == 7


def test_refusals_that_need_no_device():
    """the parameters are judged before the context is looked at"""
    L = capi.load_library()

    def prepare(**change):
        b = ctypes.c_void_p(1)
        rc = L.mmgpu_nuclmatch_prepare(None, ctypes.byref(capi.nuclmatch_params(dict(nc.params(), **change))), ctypes.byref(b))
        assert b.value is None
        return rc, (L.mmgpu_last_error() or b"").decode()

    for mode in (1, 6, -1):
        rc, msg = prepare(cov_mode=mode)
        assert rc == -4 and "cov_mode" in msg, mode
    assert "strand" in prepare(cov_mode=1)[1]
    for change in (dict(k=0), dict(k=32), dict(kmers_per_seq=0), dict(kmers_per_seq_scale=-0.1)):
        rc, msg = prepare(**change)
        assert rc == -1 and list(change)[0] in msg, change
    assert prepare(k=1)[0] == -1 and "NULL" in prepare(k=31)[1]      # fine: only the context is missing
    assert L.mmgpu_nuclmatch_prepare(None, None, None) == -1
    b = ctypes.c_void_p(1)
    assert L.mmgpu_nuclmatch_prepare(None, None, ctypes.byref(b)) == -1 and b.value is None
    assert L.mmgpu_nuclmatch_run(None, None) == -1 and L.mmgpu_nuclmatch_fetch(None, None, None, None, None) == -1
    assert L.mmgpu_nuclmatch_fetch_device(None, None, None, None) == -1 and L.mmgpu_nuclmatch_last_kernel_ms(None, None, None) == -1
