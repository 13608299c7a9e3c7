"""The exhaustive ungapped scan for PROFILE queries (include/mmgpu.h "exhaustive ungapped scan", `mmgpu_scan_query::profile`)
restated in plain numpy, the accessors of tests/golden/ungapped_scan_profile.npz and the shapes of the device tests.

    prof    = Sequence::getAlignmentProfile(): int8 [letters][qlen], entry score byte / 4 truncating toward zero
    p(i, x) = prof[x][i] for x < letters, 0 for every other letter (the X state, the pad)
    B       = |min(0, min prof)|          cap = 255 - B          (no matrix, no composition bias)
    S(i, j) = max(0, min(cap, S(i-1, j-1) + p(i, t[j])))                                        score = max S (0: empty target)
The list rule is the sequence queries' (tests/ungapped_scan_cases.select_list)."""
import json
import os

import numpy as np

from tests.ungapped_scan_cases import QUERY_LENGTHS, pack, random_seq, select_list, split  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ungapped_scan_profile.npz")
PROFILE_LETTERS = 20      # Sequence::PROFILE_AA_SIZE
ENTRY_BYTES = 25          # Sequence::PROFILE_READIN_SIZE


def alignment_profile(entry):
    """one profile-database entry [L][25] int8 -> int8 [20][L]: score / 4 in C integer division (Sequence.cpp:332-336)"""
    e = np.asarray(entry).view(np.int8).reshape(-1, ENTRY_BYTES)
    return np.ascontiguousarray(np.trunc(e[:, :PROFILE_LETTERS].astype(np.float64) / 4).astype(np.int8).T)


def bias_of(prof):
    """profile->bias of ssw_init for a profile query: from the profile alone"""
    return abs(min(0, int(np.min(prof)))) if np.size(prof) else 0


def scores_one_query(prof, targets, alphabet=21):
    """scores of one profile query against a list of targets: uint8 [len(targets)].  All targets advance together, a column per step."""
    prof = np.asarray(prof, np.int32)
    letters, qlen = prof.shape
    cap = 255 - bias_of(prof)
    assert cap > 0 and letters <= alphabet
    P = np.vstack([prof, np.zeros((alphabet + 1 - letters, qlen), np.int32)])      # letters without a row, and the pad `alphabet`
    nt = len(targets)
    lens = np.array([len(t) for t in targets], np.int64)
    order = np.argsort(-lens, kind="stable")
    L = int(lens.max()) if nt else 0
    T = np.full((nt, L), alphabet, np.int64)
    for k, o in enumerate(order):
        T[k, :lens[o]] = targets[o]
    S = np.zeros((nt, qlen), np.int32)
    best_sorted = np.zeros(nt, np.int32)
    for j in range(L):
        n = int(np.sum(lens > j))
        add = P[T[:n, j]]
        new = np.empty((n, qlen), np.int32)
        new[:, 0] = add[:, 0]
        new[:, 1:] = S[:n, :-1] + add[:, 1:]
        S[:n] = np.clip(new, 0, cap)
        best_sorted[:n] = np.maximum(best_sorted[:n], S[:n].max(axis=1))
    best = np.zeros(nt, np.int32)
    best[order] = best_sorted
    return best.astype(np.uint8)


def pair_score_cells(prof, t):
    """the same number cell by cell (slow; the cross-check of the vector form)"""
    prof = np.asarray(prof, np.int32)
    letters, qlen = prof.shape
    cap = 255 - bias_of(prof)
    S = [[0] * (len(t) + 1) for _ in range(qlen + 1)]
    best = 0
    for i in range(1, qlen + 1):
        for j in range(1, len(t) + 1):
            x = int(t[j - 1])
            p = int(prof[x, i - 1]) if x < letters else 0
            S[i][j] = max(0, min(cap, S[i - 1][j - 1] + p))
            best = max(best, S[i][j])
    return best


class Golden:
    """tests/golden/ungapped_scan_profile.npz (tests/golden/make_ungapped_scan_profile_golden.py recorded it from the stock binary).
    Groups: "A" profiles the stock binary built (search + result2profile), "B" entries written by hand; each has its own targets."""

    def __init__(self, path=GOLDEN):
        g = self.g = np.load(path)
        self.settings = json.loads(bytes(g["settings"]).decode())
        self.groups = sorted({s["group"] for s in self.settings})
        self._entries = {}
        self._targets = {}
        for grp in self.groups:
            off = g[grp + "_eoff"].astype(np.int64)
            e = g[grp + "_entries"]
            self._entries[grp] = [e[off[i]:off[i + 1]] for i in range(len(off) - 1)]
            self._targets[grp] = split(g[grp + "_tres"], g[grp + "_toff"])

    def entries(self, grp):
        """-> list of int8 [L][25]"""
        return self._entries[grp]

    def targets(self, grp):
        return self._targets[grp]

    def tlens(self, grp):
        return np.array([len(t) for t in self._targets[grp]], np.int64)

    def profiles(self, grp):
        return [alignment_profile(e) for e in self._entries[grp]]

    def expected(self, k):
        """-> per query (ids, scores) of setting k"""
        off = self.g["exp_off_%d" % k].astype(np.int64)
        ids, sc = self.g["exp_ids_%d" % k].astype(np.int64), self.g["exp_scores_%d" % k].astype(np.int64)
        return [(ids[off[i]:off[i + 1]], sc[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def check_recording(G):
    """what the recording must show to be worth committing (asserted by the generator on the reference's output and again by the
    CPU test on the file)"""
    by_name = {(s["group"], s["name"]): k for k, s in enumerate(G.settings)}
    n_sat = n_empty = n_cut = n_cov = 0
    biases = set()
    for grp in G.groups:
        biases |= {bias_of(p) for p in G.profiles(grp)}
    for k, s in enumerate(G.settings):
        profs = G.profiles(s["group"])
        for qi, (ids, sc) in enumerate(G.expected(k)):
            n_empty += int(len(ids) == 0)
            if s["name"] == "base":
                n_sat += int(np.sum(sc == 255 - bias_of(profs[qi])))
    base, small = G.expected(by_name[("A", "base")]), G.expected(by_name[("A", "max_seqs_10")])
    for (bi, bs), (si, ss) in zip(base, small):      # cut inside a class: the element behind the cut scores what the last kept one does
        if len(si) == 10 and len(bi) > 10 and bs[10] == ss[9]:
            n_cut += 1
    for (bi, _), (ci, _) in zip(base, G.expected(by_name[("A", "cov_mode_0")])):
        n_cov += len(set(bi.tolist()) - set(ci.tolist()))
    a, b = by_name[("A", "comp_bias_0")], by_name[("A", "comp_bias_1")]
    for name in ("exp_off_%d", "exp_ids_%d", "exp_scores_%d"):      # the composition bias takes no part
        assert G.g[name % a].tobytes() == G.g[name % b].tobytes(), name
    assert n_sat >= 4, n_sat
    assert n_cut >= 2, n_cut
    assert n_empty >= 1, n_empty
    assert n_cov >= 1, n_cov
    assert len(biases) >= 2, biases
    return dict(saturated=n_sat, cut_in_class=n_cut, empty=n_empty, dropped_by_coverage=n_cov, biases=sorted(biases))


# ---- crafted entries (group B of the recording, and the device tests) ----
def make_entry(rng, mat, L, sharp=1.0):
    """one profile-database entry as tests/test_profile_query.make_entry makes it: [L][25] int8 - 20 scores (x4 scale: the
    substitution row of a random consensus letter, scaled and jittered), query letter, consensus letter, Neff, 2 reserved"""
    cons = rng.integers(0, 20, L).astype(np.uint8)
    e = np.zeros((L, ENTRY_BYTES), np.int8)
    rows = np.asarray(mat)[cons][:, :20].astype(np.int32)
    e[:, :20] = np.clip(np.rint(rows * 4 * sharp + rng.integers(-6, 7, rows.shape)), -120, 120).astype(np.int8)
    e[:, 20] = cons
    e[:, 21] = cons
    e[:, 22] = 40
    return e, cons


def entry_with_one_minus_128(rng, mat, L):
    """a single score byte of -128: B = 32, cap = 223"""
    e, cons = make_entry(rng, mat, L, sharp=1.0)
    pos = L // 2
    e[pos, (int(cons[pos]) + 7) % 20] = -128
    return e, cons


def entry_with_lowest_minus_1(rng, mat, L):
    """every negative score byte in -7 .. -4: the alignment profile's lowest value is -1, B = 1, cap = 254"""
    e, cons = make_entry(rng, mat, L, sharp=1.0)
    sc = e[:, :20]
    neg = sc < 0
    sc[neg] = rng.integers(-7, -3, int(neg.sum())).astype(np.int8)
    return e, cons
