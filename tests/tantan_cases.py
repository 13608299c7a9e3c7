"""Deterministic inputs of the tantan edge tests (fixed seeds, numpy only), shared by the recording script
(tests/golden/make_tantan_edge_golden.py), the CPU tests (tests/test_tantan_edges.py) and the device tests (tests/test_tantan_gpu.py).
Every set is a list of uint8 arrays (amino-acid codes of mmseqs2_amd.workloads: A..Y -> 0..19, X -> 20); pack() makes (residues, offsets).

What each set is for:
  lengths  every length 0 .. 70 (the partial first 50 positions at every max_offset, the rescaling at 15 / 31 / 47 / 63, sequences
           shorter than one group of four states), as background, as a homopolymer and as a period-3 repeat;
  periods  one planted repeat per period 1 .. 52: every word of the 52-letter history, every repeat state, and the two periods
           beyond the 50 states the model has;
  letters  X inside a repeat, a run of X, an all-X sequence, all 20 letters once, a repeat of X (masked letters that already are
           the mask letter);
  probe    at most 400 letters in 8 sequences (one wavefront) whose every probability the two-threshold test pins."""
import numpy as np

from mmseqs2_amd.workloads import BACKGROUND

X = 20
MAX_PERIOD = 52
SET_NAMES = ("lengths", "periods", "letters")


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return res.astype(np.uint8), off


def background(rng, n, alphabet=20):
    if alphabet == 20:
        return rng.choice(20, size=n, p=BACKGROUND).astype(np.uint8)
    return rng.integers(0, alphabet, size=n).astype(np.uint8)


def repeat(rng, period, n, sub=0.05, alphabet=20):
    """a unit of `period` distinct-as-drawn letters repeated to n letters, a fraction `sub` of them substituted"""
    unit = background(rng, period, alphabet)
    rep = np.resize(unit, n)
    mut = rng.random(n) < sub
    rep[mut] = background(rng, int(mut.sum()), alphabet)
    return rep


def lengths_set():
    rng = np.random.default_rng(701)
    out = []
    for n in range(0, 71):
        out.append(background(rng, n))
        out.append(np.full(n, int(rng.integers(0, 20)), np.uint8))
        out.append(np.resize(background(rng, 3), n))
    return out


def period_layout(p):
    """(first letter, length) of the repeat planted for period p"""
    return 60, max(4 * p, 24)


def periods_set(alphabet=20, max_period=MAX_PERIOD, seed=702):
    rng = np.random.default_rng(seed)
    out = []
    for p in range(1, max_period + 1):
        _, n = period_layout(p)
        out.append(np.concatenate([background(rng, 60, alphabet), repeat(rng, p, n, 0.05, alphabet), background(rng, 60, alphabet)]))
    return out


def letters_set():
    rng = np.random.default_rng(703)
    out = []
    t = np.concatenate([background(rng, 40), repeat(rng, 5, 60, 0.0), background(rng, 40)])      # X inside a repeat
    t[[52, 71]] = X
    out.append(t)
    t = np.concatenate([background(rng, 30), np.full(25, X, np.uint8), background(rng, 30)])      # a run of X
    out.append(t)
    out.append(np.full(33, X, np.uint8))                                                           # nothing but X
    out.append(rng.permutation(20).astype(np.uint8))                                               # every letter once
    unit = np.array([X, 9, X], np.uint8)                                                           # a repeat made of the mask letter
    out.append(np.concatenate([background(rng, 20), np.resize(unit, 45), background(rng, 20)]))
    return out


def probe_set():
    """8 sequences, 388 letters: lengths 15, 16, 17, 49, 50, 51 and two longer ones"""
    rng = np.random.default_rng(704)
    out = [
        np.concatenate([background(rng, 10), repeat(rng, 7, 42, 0.05), background(rng, 8)]),       # 60: period 7
        np.concatenate([background(rng, 8), repeat(rng, 37, 111, 0.0), background(rng, 11)]),      # 130: period 37
        np.concatenate([background(rng, 20), np.full(9, 15, np.uint8), background(rng, 22)]),      # 51: a homopolymer run
        background(rng, 50),
        np.concatenate([background(rng, 24), [X], background(rng, 24)]).astype(np.uint8),         # 49: an X
        np.resize(background(rng, 2), 17),
        background(rng, 16),
        np.resize(background(rng, 4), 15),
    ]
    return out


def all_sets():
    return dict(lengths=lengths_set(), periods=periods_set(), letters=letters_set())


def plant(rng, t, start, period, n):
    t[start:start + n] = np.resize(background(rng, period), n)


def long_sequence(n, seed):
    """n background letters with repeats planted near both ends (10 .. 200 and 65 000 .. 65 400)"""
    rng = np.random.default_rng(seed)
    t = background(rng, n)
    plant(rng, t, 10, 3, 60)
    plant(rng, t, 90, 19, 110)
    plant(rng, t, 65000, 1, 40)
    plant(rng, t, 65060, 44, 220)
    plant(rng, t, 65300, 8, 100)
    return t


def mixed_lengths(n_seqs, seed, max_len=300):
    """n_seqs sequences of lengths spread over 0 .. max_len, every third with a planted repeat"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_seqs):
        n = int(rng.integers(0, max_len + 1))
        t = background(rng, n)
        if i % 3 == 0 and n > 12:
            a = int(rng.integers(0, n - 10))
            plant(rng, t, a, int(rng.integers(1, 51)), min(n - a, int(rng.integers(10, 160))))
        out.append(t)
    return out


def nucleotide_table():
    """a positive 5 x 5 likelihood-ratio table (not a reference table): 3.5 for a match, 0.4 for a mismatch, 1 against N"""
    lr = np.full((5, 5), 0.4, np.float64)
    np.fill_diagonal(lr, 3.5)
    lr[4, :] = 1.0
    lr[:, 4] = 1.0
    return lr


def nucleotide_set():
    """planted periods 1 .. 50 over A C G T (0 .. 3), an N (4) here and there, short and empty sequences"""
    rng = np.random.default_rng(705)
    out = periods_set(alphabet=4, max_period=50, seed=706)
    for k in range(0, len(out), 7):
        out[k][int(rng.integers(0, len(out[k])))] = 4
    out += [background(rng, n, 4) for n in (0, 1, 15, 16, 17, 49, 50, 51)]
    out.append(np.full(40, 4, np.uint8))
    return out
