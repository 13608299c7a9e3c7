"""Serial restatement of linclust's k-mer matching stage on a nucleotide database (`mmseqs kmermatcher --linclust-version 1` over
`createdb --dbtype 2`) and the generators of its engineered cases.  Written from the stage's description (include/mmgpu.h,
"linclust's k-mer matching stage, nucleotides"), not from the device code: plain loops and `sorted`; what the protein stage shares
comes from tests/kmermatch_cases.py.  Only the indices and hashes of all windows of one sequence are vectorised; `canonical` is the
same on Python integers and the tests hold the two against each other.

Residues are A C T G N = 0 .. 4; the complement of a residue below 4 is `code ^ 2`.  Bit 63 of a stored k-mer is set for a window taken
as it stands and clear for one taken as its reverse complement; bit 63 of an emitted key is set when the representative is aligned as
it stands and clear when it has to be reverse-complemented.

    nuclmatch(seqs, par) -> (offsets uint64[n + 1], records HIT_DTYPE)      the CSR the device returns
    par: dict(k, kmers_per_seq, kmers_per_seq_scale, hash_shift, cov_thr, cov_mode, include_only_extendable)

Ties: Python's `sorted` is stable, so records that compare equal under the reference's comparators (they can differ in the strand bit
only) stay in the order they were born in - id, then window position - which is the device's documented rule.  `strand_ties` lists
them: the reference's own order between them is unspecified."""
import json
import os

import numpy as np

from tests.kmermatch_cases import (HIT_DTYPE, M64, can_be_covered, considered_kmers, pack, select, sequence_hash, split, threshold_of,      # noqa: F401
                                   to_csr, xxh64_u64, xxh64_u64_array)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "nuclmatch.npz")
N = 4
BIT63 = 1 << 63
LETTERS = "ACTGN"


def revcomp(seq):
    s = np.asarray(seq, np.uint8)[::-1]
    return np.where(s < N, s ^ 2, N).astype(np.uint8)


def canonical(window):
    """one window of residues -> (canonical index, taken as reverse complement) or None when it holds an N or is its own reverse
    complement.  Index: 2 bits a residue, the first residue in the highest bits"""
    idx, rev = 0, 0
    for i, r in enumerate(window):
        if int(r) >= N:
            return None
        idx = (idx << 2) | int(r)
        rev |= (int(r) ^ 2) << (2 * i)
    if rev == idx:
        return None
    return (rev, True) if rev < idx else (idx, False)


def windows(seq, k):
    """-> (window positions, canonical indices, taken-as-reverse flags) of the windows that count, in position order"""
    L = len(seq)
    if L < k:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros(0, bool)
    r = np.asarray(seq, np.uint64)
    n = L - k + 1
    idx, rev, has_n = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, bool)
    for i in range(k):
        part = r[i:i + n]
        has_n |= part >= N
        idx |= (part & np.uint64(3)) << np.uint64(2 * (k - 1 - i))
        rev |= ((part & np.uint64(3)) ^ np.uint64(2)) << np.uint64(2 * i)
    pos = np.flatnonzero(~has_n & (idx != rev))
    return pos, np.minimum(idx, rev)[pos], (rev < idx)[pos]


def _scores(seq, par):
    pos, idx, is_rev = windows(seq, int(par["k"]))
    return pos, idx, is_rev, [int(x) & 0xFFFF for x in xxh64_u64_array(idx, int(par["hash_shift"]) & M64)]


def extract(seqs, par):
    """stage 1 -> records (stored k-mer, id, stored position, length) in the order they are born: per sequence the identity record,
    then the selected windows by window position"""
    k, seed = int(par["k"]), int(par["hash_shift"]) & M64
    recs = []
    for sid, s in enumerate(seqs):
        L = len(s)
        pos, idx, is_rev, scores = _scores(s, par)
        considered = considered_kmers(par["kmers_per_seq"], par["kmers_per_seq_scale"], L, len(scores))
        threshold, too_much = threshold_of(scores, considered)
        recs.append((xxh64_u64(sequence_hash(s), seed), sid, 0, L))
        for i in select(scores, considered, threshold, too_much):
            if is_rev[i]:
                recs.append((int(idx[i]), sid, L - int(pos[i]) - k, L))
            else:
                recs.append((int(idx[i]) | BIT63, sid, int(pos[i]), L))
    return recs


def last_bin_surplus(seq, par):
    """tooMuchElemInLastBin of one sequence"""
    _, _, _, scores = _scores(seq, par)
    considered = considered_kmers(par["kmers_per_seq"], par["kmers_per_seq_scale"], len(seq), len(scores))
    return threshold_of(scores, considered)[1] if scores and considered > 0 else 0


def sort1_key(r):
    return (r[0] | BIT63, -r[3], r[1], r[2])


def group(recs, par):
    """sort 1 + assignGroup -> the emitted (representative, representative stays as it is, member, diagonal), in sort-1 order.
    Lengths and positions are below 32 767, so the reference's arithmetic in `short` never wraps"""
    cov_mode = int(par["cov_mode"])
    assert cov_mode != 1, "the target-coverage swap loses the strand: refused on a nucleotide database"
    recs = sorted(recs, key=sort1_key)
    out = []
    a = 0
    while a < len(recs):
        b = a
        while b < len(recs) and recs[b][0] | BIT63 == recs[a][0] | BIT63:
            b += 1
        if b - a > 1:
            rep_kmer, rep, q_pos, q_len = recs[a]
            rep_reverse = not rep_kmer & BIT63
            for kmer, member, t_pos, t_len in recs[a:b]:
                target_reverse = not kmer & BIT63
                if target_reverse:      # both positions counted from the far end
                    diagonal = (q_len - 1 - q_pos) - (t_len - 1 - t_pos)
                else:
                    diagonal = q_pos - t_pos
                as_it_is = rep_reverse == target_reverse
                extendable = diagonal < 0 or diagonal > q_len - t_len
                coverable = can_be_covered(par["cov_thr"], cov_mode, q_len, t_len)
                if (not par["include_only_extendable"] and coverable) or (par["include_only_extendable"] and extendable):
                    out.append((rep, as_it_is, member, diagonal))
        a = b
    return out


def sort2_key(e):
    return (e[0], e[2], e[3])


def runs(pairs):
    """sort 2 -> [(representative, member, [(diagonal, as_it_is), ...])] per (representative, member) run"""
    pairs = sorted(pairs, key=sort2_key)
    out = []
    for rep, as_it_is, member, diagonal in pairs:
        if not out or out[-1][:2] != (rep, member):
            out.append((rep, member, []))
        out[-1][2].append((diagonal, as_it_is))
    return out


def vote_run(entries):
    """writeKmerMatcherResult on one run -> (score, diagonal): a run that starts with an as-it-is entry gets score 0 and that entry's
    diagonal; else the vote runs over the leading reverse entries only"""
    diagonal, prev, best, cnt, walked = entries[0][0], entries[0][0], 0, 0, 0
    for d, as_it_is in entries:
        if as_it_is:
            break
        cnt = cnt + 1 if d == prev else 1
        if cnt >= best:
            diagonal, best = d, cnt
        prev = d
        walked += 1
    return -walked, diagonal


def nuclmatch_lists(seqs, par):
    lists = [[(i, 0, 0)] for i in range(len(seqs))]
    for rep, member, entries in runs(group(extract(seqs, par), par)):
        if member != rep:
            lists[rep].append((member,) + vote_run(entries))
    return lists


def nuclmatch(seqs, par):
    return to_csr(nuclmatch_lists(seqs, par))


def strand_ties(seqs, par):
    """the records of sort 1 and the entries of sort 2 that compare equal to a neighbour under the reference's comparator but differ
    in the strand bit: where the reference's (unstable) sort leaves the order open"""
    recs = sorted(extract(seqs, par), key=sort1_key)
    out = [("sort1", a, b) for a, b in zip(recs, recs[1:]) if sort1_key(a) == sort1_key(b) and a[0] != b[0]]
    pairs = sorted(group(recs, par), key=sort2_key)
    out += [("sort2", a, b) for a, b in zip(pairs, pairs[1:]) if sort2_key(a) == sort2_key(b) and a[1] != b[1]]
    return out


# ---- what a run looks like: the engineered cases are looked for with these ----------------------------------------------------------

def starts_forward(entries):
    return entries[0][1]


def starts_reverse_and_changes(entries):
    return not entries[0][1] and any(e[1] for e in entries)


def tied_vote(entries):
    """the leading reverse stretch collects its largest count on two diagonals"""
    cnt = {}
    for d, as_it_is in entries:
        if as_it_is:
            break
        cnt[d] = cnt.get(d, 0) + 1
    return len(cnt) >= 2 and sorted(cnt.values())[-2] == max(cnt.values())


def runs_where(seqs, par, what):
    return [(rep, member) for rep, member, entries in runs(group(extract(seqs, par), par)) if rep != member and what(entries)]


# ---- generated inputs --------------------------------------------------------------------------------------------------------------

def random_seq(rng, n):
    return rng.integers(0, 4, int(n)).astype(np.uint8)


def mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = rng.integers(0, 4, int(hit.sum()))
    return s


def params(k=17, kmers_per_seq=60, scale=0.2, hash_shift=67, cov_thr=0.8, cov_mode=0, include_only_extendable=0):
    """linclust's nucleotide defaults"""
    return dict(k=k, kmers_per_seq=kmers_per_seq, kmers_per_seq_scale=scale, hash_shift=hash_shift, cov_thr=cov_thr, cov_mode=cov_mode,
                include_only_extendable=include_only_extendable)


def find_last_bin_sequence(par, seed=1, length=400, tries=4000):
    """a random sequence whose last selected bin holds more elements than needed, found by search: an inner repeat makes equal scores"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        s = random_seq(rng, length)
        n = int(rng.integers(int(par["k"]) + 2, int(par["k"]) + 40))
        a, b = int(rng.integers(0, length // 2 - n)), int(rng.integers(length // 2, length - n))
        s[b:b + n] = s[a:a + n]
        if last_bin_surplus(s, par) > 0:
            return s
    raise AssertionError("no sequence with a surplus in its last bin found")


def find_tied_family(par, seed=2, tries=4000):
    """(representative, member): the member is the reverse complement of the representative with three residues inserted in the
    middle, so that the run is voted and its k-mers lie on two diagonals; searched until the two collect equally many"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        rep = random_seq(rng, 260)
        cut = int(rng.integers(100, 160))
        member = revcomp(np.concatenate([rep[:cut], random_seq(rng, 3), rep[cut:-6]]))
        if runs_where([rep, member], par, tied_vote):
            return rep, member
    raise AssertionError("no family with a tied vote found")


def lognormal_database(seed, n=2000):
    """kmermatch_cases.lognormal_database's shape over the four letters and N: log-normal lengths around 150 residues; a third of the
    sequences are mutated, end-truncated copies of earlier ones, half of those reverse-complemented"""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(5.0, 0.6, n), 5, 3000).astype(int)
    seqs = []
    for i in range(n):
        if i > 10 and rng.random() < 0.33:
            src = seqs[int(rng.integers(0, i))]
            s = mutate(rng, src, 0.05)[int(rng.integers(0, 5)):]
            s = revcomp(s) if rng.random() < 0.5 else s
            seqs.append(s if len(s) else random_seq(rng, 5))
        else:
            seqs.append(random_seq(rng, lens[i]))
    for j in range(0, n, 97):
        seqs[j][::23] = N
    for j in range(5, n, 211):      # shorter than k, and around it
        seqs[j] = random_seq(rng, 1 + j % 19)
    return seqs


RECORDED_KS = (17, 18, 24, 31)


def make_database(seed=20261021):
    """the recorded database (tests/golden/make_nuclmatch_golden.py): a few hundred sequences of 20 - 400 residues over A C G T and N"""
    rng = np.random.default_rng(seed)
    seqs = [random_seq(rng, n) for n in rng.integers(20, 400, 120)]
    special = {}
    for f in range(14):      # families of mutated and end-truncated copies, about half of the members reverse-complemented
        base = random_seq(rng, int(rng.integers(150, 400)))
        seqs.append(base)
        for m in range(int(rng.integers(2, 6))):
            s = mutate(rng, base, float(rng.choice([0.01, 0.03, 0.06])))
            a, b = int(rng.integers(0, 12)), int(rng.integers(0, 25))
            s = s[a:len(s) - b]
            seqs.append(revcomp(s) if (f + m) % 2 else s)
    s = random_seq(rng, 300)
    special["reverse_complement"] = [len(seqs), len(seqs) + 1]
    seqs += [s, revcomp(s)]
    dup = random_seq(rng, 140)
    special["duplicates"] = [len(seqs), len(seqs) + 1, len(seqs) + 2]
    seqs += [dup, dup.copy(), dup.copy()]
    short_dup = random_seq(rng, 15)      # shorter than every k: the identity record is all these two have
    special["short_duplicates"] = [len(seqs), len(seqs) + 1]
    seqs += [short_dup, short_dup.copy()]
    base = random_seq(rng, 180)      # two members of equal length: the id decides the representative
    special["equal_length"] = [len(seqs), len(seqs) + 1]
    seqs += [mutate(rng, base, 0.02), revcomp(mutate(rng, base, 0.02))]
    for k in RECORDED_KS:
        for n in (k - 1, k, k + 1):      # twice each so that they can match
            s = random_seq(rng, n)
            seqs += [s, s.copy()]
        for n in (62 + k, 63 + k, 64 + k):      # 63, 64 and 65 windows
            s = random_seq(rng, n)
            seqs += [s, revcomp(mutate(rng, s, 0.02))]
    all_n = random_seq(rng, 90)
    all_n[::16] = N      # every window of 17 residues or more holds an N
    special["all_n"] = [len(seqs)]
    seqs += [all_n, all_n.copy()]
    with_n = mutate(rng, seqs[121], 0.01)
    with_n[40:43] = N
    special["short_run_of_n"] = [len(seqs)]
    seqs.append(with_n)
    own = random_seq(rng, 200)      # for the even k: windows that are their own reverse complement
    half = random_seq(rng, 12)
    own[50:74] = np.concatenate([half, revcomp(half)])
    half = random_seq(rng, 9)
    own[120:138] = np.concatenate([half, revcomp(half)])
    special["self_complementary"] = [len(seqs), len(seqs) + 1]
    seqs += [own, mutate(rng, own, 0.01)[3:]]
    rep = random_seq(rng, 360)      # inversions: one half of the member as it is, the other reverse-complemented
    a, b = rep[:170], rep[170:]
    special["inversion"] = [len(seqs), len(seqs) + 1, len(seqs) + 2]
    seqs += [rep, np.concatenate([a, revcomp(b)])[:-4], np.concatenate([revcomp(a), b])[:-4]]
    rep, member = find_tied_family(params(k=17))
    special["tied"] = [len(seqs), len(seqs) + 1]
    seqs += [rep, member]
    s = find_last_bin_sequence(params(k=17, kmers_per_seq=300))
    special["last_bin"] = [len(seqs), len(seqs) + 1]
    seqs += [s, revcomp(mutate(rng, s, 0.02))]
    return seqs, special


class Golden:
    def __init__(self, path=GOLDEN):
        g = np.load(path)
        self.g = g
        self.seqs = split(g["res"], g["off"])
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.special = json.loads(bytes(g["special"]).decode())

    def params(self, s):
        return {key: s[key] for key in ("k", "kmers_per_seq", "kmers_per_seq_scale", "hash_shift", "cov_thr", "cov_mode", "include_only_extendable")}

    def expected(self, k):
        """-> (offsets, records) of setting k"""
        off = self.g["exp_off_%d" % k].astype(np.uint64)
        rec = np.zeros(int(off[-1]), HIT_DTYPE)
        rec["id"] = self.g["exp_id_%d" % k]
        rec["score"] = self.g["exp_score_%d" % k]
        rec["diagonal"] = self.g["exp_diag_%d" % k].astype(np.int64) & 0xFFFF
        return off, rec
