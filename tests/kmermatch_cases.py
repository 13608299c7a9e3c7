"""Serial restatement of linclust's k-mer matching stage (`mmseqs kmermatcher --linclust-version 1`, amino acids) and the generator
of its engineered cases.  Written from the stage's description, not from the device code: plain loops, a 65 536-bin histogram,
`sorted` with tuple keys.  Only the hashing of all windows of one sequence is vectorised (numpy uint64 arithmetic wraps as the
reference's size_t does); `xxh64_u64` is the same hash on Python integers and the tests hold the two against each other.

    kmermatch(seqs, par) -> (offsets uint64[n + 1], records PF_HIT_DTYPE)      the CSR the device returns
    par: dict(k, alph_size, reduce[21], kmers_per_seq, kmers_per_seq_scale, hash_shift, cov_thr, cov_mode, include_only_extendable)
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kmermatch.npz")

HIT_DTYPE = np.dtype([("id", np.uint32), ("score", np.int32), ("diagonal", np.uint16), ("reserved", np.uint16)])      # mmgpu_pf_hit
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
X21 = 20      # the full alphabet's X


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def xxh64_u64(value, seed):
    """XXH64 of the 8 little-endian bytes of `value` (public xxHash specification, inputs shorter than 32 bytes)"""
    h = (seed + P5 + 8) & M64
    k1 = (_rotl((value * P2) & M64, 31) * P1) & M64
    h ^= k1
    h = (_rotl(h, 27) * P1 + P4) & M64
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    h ^= h >> 32
    return h


def xxh64_u64_array(values, seed):
    """xxh64_u64 over a uint64 array"""
    u = np.uint64
    v = np.asarray(values, np.uint64)

    def rotl(x, r):
        return (x << u(r)) | (x >> u(64 - r))
    with np.errstate(over="ignore"):
        h = np.full(v.shape, (seed + P5 + 8) & M64, np.uint64)
        k1 = rotl(v * u(P2), 31) * u(P1)
        h = h ^ k1
        h = rotl(h, 27) * u(P1) + u(P4)
        h ^= h >> u(33)
        h *= u(P2)
        h ^= h >> u(29)
        h *= u(P3)
        h ^= h >> u(32)
    return h


def sequence_hash(reduced):
    """Util::hash: polynomial, base 31, wrapping uint64"""
    h = 0
    for x in reduced:
        h = (h * 31 + int(x)) & M64
    return h


def windows(reduced, k, alph_size):
    """-> (positions, k-mer indices) of the windows without the reduced X, in position order"""
    L = len(reduced)
    if L < k:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    r = np.asarray(reduced, np.uint64)
    n = L - k + 1
    idx = np.zeros(n, np.uint64)
    has_x = np.zeros(n, bool)
    power = 1
    with np.errstate(over="ignore"):
        for i in range(k):
            idx += r[i:i + n] * np.uint64(power & M64)
            has_x |= r[i:i + n] == alph_size - 1
            power *= alph_size - 1
    pos = np.flatnonzero(~has_x)
    return pos, idx[pos]


def considered_kmers(kmers_per_seq, scale, L, count):
    """min((size_t)(kmersPerSequence - 1 + scale * L), count), the sum in float32"""
    f = np.float32
    return min(int(f(kmers_per_seq - 1) + f(scale) * f(L)), count)


def threshold_of(scores, considered):
    """the two-level walk over the score histogram -> (threshold, tooMuchElemInLastBin)"""
    dist = [0] * 65536
    coarse = [0] * 128
    for s in scores:
        dist[s] += 1
        coarse[s >> 9] += 1
    threshold, in_bins = 0, 0
    if len(scores) > 0:
        h = 0
        while h < 128 and in_bins < considered:
            in_bins += coarse[h]
            h += 1
        h -= 1 if h > 0 else 0
        in_bins -= coarse[h]      # (a size_t that wraps below 0 when nothing is considered: nothing is selected then)
        threshold = h * 512
        while threshold <= 65535 and 0 <= in_bins < considered:
            in_bins += dist[threshold]
            threshold += 1
    return threshold, in_bins - considered


def select(scores, considered, threshold, too_much):
    """the selection loop, in position order -> indices into `scores`"""
    out = []
    for i, s in enumerate(scores):
        if len(out) >= considered:
            break
        if s < threshold:
            if s == threshold - 1 and too_much:
                too_much -= 1
                threshold -= 1 if too_much == 0 else 0
            out.append(i)
    return out


def extract(seqs, par):
    """stage 1 -> records (kmer, id, pos, len) in sequence order: the identity record, then the selected windows by position"""
    reduce = np.asarray(par["reduce"], np.uint8)
    k, alph, seed = int(par["k"]), int(par["alph_size"]), int(par["hash_shift"]) & M64
    recs = []
    for sid, s in enumerate(seqs):
        red = reduce[np.asarray(s, np.int64)]
        L = len(red)
        pos, idx = windows(red, k, alph)
        scores = [int(x) & 0xFFFF for x in xxh64_u64_array(idx, seed)]
        considered = considered_kmers(par["kmers_per_seq"], par["kmers_per_seq_scale"], L, len(scores))
        threshold, too_much = threshold_of(scores, considered)
        recs.append((xxh64_u64(sequence_hash(red), seed), sid, 0, L))
        for i in select(scores, considered, threshold, too_much):
            recs.append((int(idx[i]), sid, int(pos[i]), L))
    return recs


def last_bin_surplus(seq, par):
    """tooMuchElemInLastBin of one sequence"""
    red = np.asarray(par["reduce"], np.uint8)[np.asarray(seq, np.int64)]
    _, idx = windows(red, int(par["k"]), int(par["alph_size"]))
    scores = [int(x) & 0xFFFF for x in xxh64_u64_array(idx, int(par["hash_shift"]) & M64)]
    considered = considered_kmers(par["kmers_per_seq"], par["kmers_per_seq_scale"], len(red), len(scores))
    return threshold_of(scores, considered)[1] if scores and considered > 0 else 0


def can_be_covered(cov_thr, cov_mode, qlen, tlen):
    """Util::canBeCovered in float32"""
    f = np.float32
    q, t, thr = f(qlen), f(tlen), f(cov_thr)
    if cov_mode == 0:
        return bool(q / t >= thr and t / q >= thr)
    if cov_mode == 1:
        return bool(q / t >= thr)
    if cov_mode == 2:
        return bool(t / q >= thr)
    if cov_mode == 3:
        return bool(t / q >= thr and t / q <= f(1.0))
    if cov_mode == 4:
        return bool(q / t >= thr and q / t <= f(1.0))
    if cov_mode == 5:
        return bool(min(q, t) / max(q, t) >= thr)
    return True


def group(recs, par):
    """sort 1 + assignGroup -> the emitted (rep, member, diagonal)"""
    recs = sorted(recs, key=lambda r: (r[0], -r[3], r[1], r[2]))
    out = []
    a = 0
    while a < len(recs):
        b = a
        while b < len(recs) and recs[b][0] == recs[a][0]:
            b += 1
        if b - a > 1:
            _, rep, rep_pos, qlen = recs[a]
            for _, member, pos, tlen in recs[a:b]:
                diagonal = rep_pos - pos
                extendable = diagonal < 0 or diagonal > qlen - tlen
                coverable = can_be_covered(par["cov_thr"], int(par["cov_mode"]), qlen, tlen)
                if (not par["include_only_extendable"] and coverable) or (par["include_only_extendable"] and extendable):
                    if qlen < tlen and int(par["cov_mode"]) == 1:
                        out.append((member, rep, -diagonal))
                    else:
                        out.append((rep, member, diagonal))
        a = b
    return out


def vote(pairs, n):
    """sort 2 + writeKmerMatcherResult -> per sequence its list of (id, score, diagonal)"""
    pairs = sorted(pairs)
    lists = [[(i, 0, 0)] for i in range(n)]
    a = 0
    while a < len(pairs):
        rep, member = pairs[a][0], pairs[a][1]
        b = a
        diagonal, prev, best, cnt = pairs[a][2], pairs[a][2], 0, 0
        while b < len(pairs) and pairs[b][0] == rep and pairs[b][1] == member:
            cnt = cnt + 1 if pairs[b][2] == prev else 1
            if cnt >= best:
                diagonal, best = pairs[b][2], cnt
            prev = pairs[b][2]
            b += 1
        if member != rep:
            lists[rep].append((member, b - a, diagonal))
        a = b
    return lists


def to_csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    rec = np.zeros(int(off[-1]), HIT_DTYPE)
    flat = [x for lines in lists for x in lines]
    rec["id"] = [x[0] for x in flat]
    rec["score"] = [x[1] for x in flat]
    rec["diagonal"] = np.asarray([x[2] for x in flat], np.int64) & 0xFFFF
    return off, rec


def kmermatch_lists(seqs, par):
    return vote(group(extract(seqs, par), par), len(seqs))


def kmermatch(seqs, par):
    return to_csr(kmermatch_lists(seqs, par))


def tied_diagonal_pairs(seqs, par):
    """the (rep, member) pairs whose longest run of equal diagonals is attained by two different diagonals"""
    pairs = sorted(group(extract(seqs, par), par))
    runs = {}
    for rep, member, d in pairs:
        runs.setdefault((rep, member), {}).setdefault(d, 0)
        runs[(rep, member)][d] += 1
    return [key for key, cnt in runs.items() if key[0] != key[1] and sorted(cnt.values())[-2:].count(max(cnt.values())) == 2]


# ---- generated inputs --------------------------------------------------------------------------------------------------------------

def random_seq(rng, n):
    return rng.integers(0, 20, int(n)).astype(np.uint8)


def mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = rng.integers(0, 20, int(hit.sum()))
    return s


def identity_params(k=10, kmers_per_seq=20, scale=0.0, hash_shift=67, cov_thr=0.8, cov_mode=0, include_only_extendable=0):
    """the 21-letter alphabet (identity reduction) with linclust's other defaults"""
    return dict(k=k, alph_size=21, reduce=list(range(21)), kmers_per_seq=kmers_per_seq, kmers_per_seq_scale=scale, hash_shift=hash_shift,
                cov_thr=cov_thr, cov_mode=cov_mode, include_only_extendable=include_only_extendable)


def find_last_bin_sequence(par, seed=1, length=700, tries=4000):
    """a random sequence whose last selected bin holds more elements than needed, found by search: an inner repeat makes equal scores"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        s = random_seq(rng, length)
        a, b, n = rng.integers(0, length // 2 - 40), rng.integers(length // 2, length - 40), rng.integers(int(par["k"]), 40)
        s[b:b + n] = s[a:a + n]
        if last_bin_surplus(s, par) > 0:
            return s
    raise AssertionError("no sequence with a surplus in its last bin found")


def find_tied_family(par, seed=2, tries=4000):
    """(representative, member): the member is the representative with three residues inserted in the middle, so that their shared
    k-mers lie on two diagonals; searched until the two diagonals collect equally many"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        rep = random_seq(rng, 160)
        cut = int(rng.integers(60, 100))
        member = np.concatenate([rep[:cut], random_seq(rng, 3), rep[cut:-6]])
        if tied_diagonal_pairs([rep, member], par):
            return rep, member
    raise AssertionError("no family with tied diagonals found")


def lognormal_database(seed, n=2000):
    """log-normal lengths around 150 residues; a tenth of the sequences are mutated, end-truncated copies of earlier ones"""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(5.0, 0.6, n), 5, 3000).astype(int)
    seqs = []
    for i in range(n):
        if i > 10 and rng.random() < 0.3:
            src = seqs[int(rng.integers(0, i))]
            s = mutate(rng, src, 0.05)[int(rng.integers(0, 5)):]
            seqs.append(s if len(s) else random_seq(rng, 5))
        else:
            seqs.append(random_seq(rng, lens[i]))
    for j in range(0, n, 97):
        seqs[j][::7] = X21
    for j in range(5, n, 211):      # shorter than k, and around it
        seqs[j] = random_seq(rng, 1 + j % 13)
    return seqs


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)), off


def split(res, off):
    return [np.asarray(res[int(off[i]):int(off[i + 1])], np.uint8) for i in range(len(off) - 1)]


def make_database(reduce13):
    """the recorded database (tests/golden/make_kmermatch_golden.py): a few hundred sequences over the 20 amino acids and X.
    reduce13: the reference's 13-letter reduction, which the search for the last-bin sequence needs (--kmer-per-seq 300 runs on it)"""
    rng = np.random.default_rng(20261020)
    seqs = [random_seq(rng, n) for n in rng.integers(30, 260, 150)]
    special = {}
    for f in range(14):      # families of mutated and end-truncated copies
        base = random_seq(rng, int(rng.integers(120, 300)))
        seqs.append(base)
        for m in range(int(rng.integers(2, 6))):
            s = mutate(rng, base, float(rng.choice([0.02, 0.05, 0.1])))
            a, b = int(rng.integers(0, 12)), int(rng.integers(0, 25))
            seqs.append(s[a:len(s) - b])
    dup = random_seq(rng, 140)      # exact duplicates: they meet through the identity record (and here through every k-mer too)
    special["duplicates"] = [len(seqs), len(seqs) + 1, len(seqs) + 2]
    seqs += [dup, dup.copy(), dup.copy()]
    short_dup = random_seq(rng, 9)      # shorter than every k: the identity record is all these two have
    special["short_duplicates"] = [len(seqs), len(seqs) + 1]
    seqs += [short_dup, short_dup.copy()]
    base = random_seq(rng, 180)      # two members of equal length: the id decides the representative
    special["equal_length"] = [len(seqs), len(seqs) + 1]
    seqs += [mutate(rng, base, 0.03), mutate(rng, base, 0.03)]
    for n in range(8, 17):      # k - 1, k, k + 1 for every recorded k, twice each so that they can match
        s = random_seq(rng, n)
        seqs += [s, s.copy()]
    for n in range(70, 80):      # 63, 64 and 65 windows for every recorded k
        s = random_seq(rng, n)
        seqs += [s, mutate(rng, s, 0.03)]
    allx = random_seq(rng, 90)
    allx[::8] = X21      # every window of 9 residues or more holds an X
    special["all_x"] = [len(seqs)]
    seqs += [allx, allx.copy()]
    with_x = mutate(rng, seqs[151], 0.02)
    with_x[40:43] = X21
    seqs.append(with_x)
    tied = identity_params(k=14, kmers_per_seq=20)      # (the --min-seq-id 0.99 setting: 21 letters, no recorded table needed)
    rep, member = find_tied_family(tied)
    special["tied"] = [len(seqs), len(seqs) + 1]
    seqs += [rep, member]
    surplus = dict(identity_params(k=10, kmers_per_seq=300), alph_size=13, reduce=[int(x) for x in reduce13])
    s = find_last_bin_sequence(surplus)
    special["last_bin"] = [len(seqs), len(seqs) + 1]
    seqs += [s, mutate(rng, s, 0.02)]
    return seqs, special


class Golden:
    def __init__(self, path=GOLDEN):
        g = np.load(path)
        self.g = g
        self.seqs = split(g["res"], g["off"])
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.special = json.loads(bytes(g["special"]).decode())
        self.chains = json.loads(bytes(g["chains"]).decode())
        self.hash_triples = g["hash_triples"]      # uint64[n][3]: input, seed, hash

    def params(self, s):
        return dict(k=s["k"], alph_size=s["alph_size"], reduce=s["reduce"], kmers_per_seq=s["kmers_per_seq"],
                    kmers_per_seq_scale=s["kmers_per_seq_scale"], hash_shift=s["hash_shift"], cov_thr=s["cov_thr"], cov_mode=s["cov_mode"],
                    include_only_extendable=s["include_only_extendable"])

    def expected(self, k):
        """-> (offsets, records) of setting k"""
        off = self.g["exp_off_%d" % k].astype(np.uint64)
        rec = np.zeros(int(off[-1]), HIT_DTYPE)
        rec["id"] = self.g["exp_id_%d" % k]
        rec["score"] = self.g["exp_score_%d" % k]
        rec["diagonal"] = self.g["exp_diag_%d" % k].astype(np.int64) & 0xFFFF
        return off, rec

    def chain_expected(self, c):
        """-> per query the lines of the recorded rescorediagonal result of chain c"""
        off = self.g["chain_off_%d" % c]
        key, score = self.g["chain_key_%d" % c], self.g["chain_score_%d" % c]
        out = []
        if self.chains[c]["rescore_mode"] != 2:
            diag = self.g["chain_diag_%d" % c]
            for q in range(len(off) - 1):
                out.append([(int(key[i]), int(score[i]), int(diag[i])) for i in range(int(off[q]), int(off[q + 1]))])
            return out
        seqid, evalue, pos = self.g["chain_seqid_%d" % c], self.g["chain_evalue_%d" % c], self.g["chain_pos_%d" % c]
        for q in range(len(off) - 1):
            out.append([(int(key[i]), int(score[i]), float(seqid[i]), float(evalue[i])) + tuple(int(x) for x in pos[i]) + (None, None)
                        for i in range(int(off[q]), int(off[q + 1]))])      # (laid out as rescore_cases.Golden.expected)
        return out
