"""The exactness rule of the f16 forward scan (mmseqs2_amd/csrc/sw_body.h, at SW_HALF_LIMIT) on a numpy model: the recurrence
the kernel runs,
    H = max3(Hd + P, E, F);  E' = max3(E - ge, H - go, 0);  F' = max3(F - ge, H - go, 0)
once in integers and once with every operation rounded to np.float16 (one rounding per operation, as v_pk_add_f16 does), on
profiles whose entries reach out to +-127 from the matrix plus +-127 from the composition bias - [-256, 254] - and are -32768 in
the rows past the query end and in the columns past the target end.

Claim: with LIMIT = 2048 - 256, "the final maximum exceeds LIMIT" is the same decision in both, and every column up to and
including the first one whose running maximum exceeds LIMIT is equal cell for cell - so a pair that is not flagged has the int16
kernel's H everywhere (score and end position with it), and a flagged pair is found by the f16 scan without fail.
(The integer model does not saturate at 32767 as the int16 kernel does: that only matters far above the limit, where the model's
columns are no longer compared and the flag is up either way.)

The trials of a batch run side by side (one numpy operation per cell for all of them); a batch takes well under a second."""
import numpy as np
import pytest

LIMIT = 2048 - 256
PAD = -32768
ROWS, COLS, TRIALS = 40, 44, 256


def _scan(P, go, ge, dtype):
    """P [trial, row, column] -> H [trial, column, row] of the kernel's recurrence with every operation in `dtype`"""
    B, n, m = P.shape
    P = P.astype(dtype)
    go, ge, zero = dtype(go), dtype(ge), np.zeros(B, dtype)
    Hprev, E = np.zeros((B, n + 1), dtype), np.zeros((B, n), dtype)
    out = np.zeros((B, m, n), dtype)
    for j in range(m):
        H = np.zeros((B, n + 1), dtype)
        F = zero
        for i in range(n):
            h = np.maximum(np.maximum((Hprev[:, i] + P[:, i, j]).astype(dtype), E[:, i]), F)
            t = (h - go).astype(dtype)
            E[:, i] = np.maximum(np.maximum((E[:, i] - ge).astype(dtype), t), zero)
            F = np.maximum(np.maximum((F - ge).astype(dtype), t), zero)
            H[:, i + 1] = h
        out[:, j, :] = H[:, 1:]
        Hprev = H
    return out


def _profiles(rng):
    """TRIALS profiles: random ones at every scale of diagonal, and engineered ones whose best path is a bare diagonal that
    sums to a chosen value around LIMIT and 2048; ragged query and target ends padded with -32768"""
    P = rng.integers(-256, 40, (TRIALS, ROWS, COLS))
    exact = {}
    targets = [LIMIT - 2, LIMIT - 1, LIMIT, LIMIT + 1, LIMIT + 2, 2046, 2047, 2048, 2049, 2050, LIMIT, LIMIT + 1]
    for b in range(TRIALS):
        qlen, tlen = int(rng.integers(20, ROWS + 1)), int(rng.integers(20, COLS - 1))
        k = min(qlen, tlen)
        if b < len(targets):                       # a bare diagonal of k - 4 steps that sums to targets[b], everything else -256
            steps = k - 4
            d = np.full(steps, targets[b] // steps)
            d[:targets[b] - d.sum()] += 1
            assert d.sum() == targets[b] and d.max() <= 254
            P[b] = -256
            P[b, np.arange(steps), np.arange(steps)] = rng.permutation(d)
            exact[b] = targets[b]
        else:                                      # homolog-like: a positive diagonal band with gaps in it
            top = int(rng.choice([6, 20, 60, 110, 180, 254]))
            shift = int(rng.integers(0, 4))
            for i in range(k - shift):
                if rng.random() < 0.9:
                    P[b, i, i + shift] = rng.integers(top // 3, top + 1)
            if b % 3 == 0:                         # the extremes of the range, side by side
                P[b, rng.integers(0, qlen, 12), rng.integers(0, tlen, 12)] = rng.choice([-256, 254], 12)
        P[b, qlen:, :] = PAD
        P[b, :, tlen:] = PAD
    return P, exact


@pytest.mark.parametrize("go,ge", [(11, 1), (12, 11), (44, 4), (175, 14), (300, 299), (2048, 1), (2048, 2047)])
def test_flag_and_columns_agree(go, ge):
    rng = np.random.default_rng(1000 * go + ge)
    P, exact = _profiles(rng)
    assert P.min() == PAD and P[P > PAD].min() == -256 and P.max() == 254
    Hi = _scan(P, go, ge, np.int64)
    Hh = _scan(P, go, ge, np.float16).astype(np.float64)
    run_i = np.maximum.accumulate(Hi.max(axis=2), axis=1)          # running maximum per column, as the kernel keeps it
    run_h = np.maximum.accumulate(Hh.max(axis=2), axis=1)
    flag_i, flag_h = run_i[:, -1] > LIMIT, run_h[:, -1] > LIMIT
    assert np.array_equal(flag_i, flag_h)
    for b in range(TRIALS):
        first = int(np.argmax(run_i[b] > LIMIT)) if flag_i[b] else COLS - 1
        assert np.array_equal(Hi[b, :first + 1], Hh[b, :first + 1]), (b, first)
        if not flag_i[b]:                          # the result the kernel would write: score, first column, first row
            assert run_h[b, -1] == run_i[b, -1]
    for b, v in exact.items():
        assert run_i[b, -1] == v and flag_i[b] == (v > LIMIT)
    assert flag_i.sum() >= 20 and (~flag_i).sum() >= 20
    # the model does leave the integers above the limit: without the flag the f16 scan would be wrong
    assert any(not np.array_equal(Hi[b], Hh[b]) for b in range(TRIALS) if flag_i[b])
