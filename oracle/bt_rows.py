"""The row-parallel formulation of banded_sw that the wave traceback kernel (mmseqs2_amd/csrc/bt_wave_kernel.hip) computes, in
serial Python - the model tests/test_bt_formulation.py and scripts/bt_formulation_check.py hold against the literal restatement
(oracle/sw_oracle.c banded_backtrace_impl):
 * previous-row H / E by COLUMN with explicit rules instead of the reference's band-frame arrays and their zeroed slots
   (`zero_last`: what row i sees at its last column is 0 when i <= w + 1 or the band is not clipped by the target end);
 * F from H-without-F (Hnf = max(e1, diag)): f[j] = max(Hnf[j-1] - go, f[j-1] - ge), same value and same tie flag;
so that every cell of a row depends on the previous row only, plus a max-plus prefix scan along the row."""


def banded_rows(q, cb, t, mat, go, ge, score, band=None, ties=False):
    """q / cb / t: the aligned sub-rectangle.  -> the backtrace string.
    band: run only the pass of this half-width (the final band the restatement reported) instead of doubling up to it.
    ties=True: -> (string, [(i, j, j - first band column of row i, kind)]) for every cell of the walked path whose consulted
    decision was an exact tie: 'hd' H between the diagonal and a gap, 'ef' H between E and F, 'ee' / 'ff' a gap between being
    opened and being extended."""
    ql, tl = len(q), len(t)
    bw = abs(tl - ql) + 1 if band is None else int(band)
    while True:
        Hprev, Eprev = {}, {}
        dirs = []
        mx = 0
        for i in range(ql):
            beg, end = max(0, i - bw), min(tl - 1, i + bw)
            pbeg, pend = max(0, i - 1 - bw), min(tl - 1, i - 1 + bw)
            zero_last = i <= bw + 1 or i + bw <= tl - 1
            Hc, Ec, row = {}, {}, {}
            f, hnf_left = 0, 0          # virtual predecessor of the first column: H = 0, f = 0
            for j in range(beg, end + 1):
                if i == 0:
                    t1, t2 = -go, -ge
                else:
                    hp = Hprev.get(j, 0) if pbeg <= j <= pend else 0
                    ep = Eprev.get(j, 0) if pbeg <= j <= pend else 0
                    if j == end and zero_last:
                        hp = ep = 0
                    t1, t2 = hp - go, ep - ge
                ev = max(t1, t2)
                de = 3 if t1 > t2 else 2
                tie_e = t1 == t2
                t1, t2 = hnf_left - go, f - ge
                f = max(t1, t2)
                df = 5 if t1 > t2 else 4
                tie_f = t1 == t2
                f1, e1 = max(f, 0), max(ev, 0)
                hd = Hprev.get(j - 1, 0) if (i > 0 and pbeg <= j - 1 <= pend) else 0
                diag = hd + int(mat[q[i], t[j]]) + (int(cb[i]) if cb is not None else 0)
                a = max(e1, f1)
                h = max(a, diag)
                mx = max(mx, h)
                dh = 1 if a <= diag else (de if e1 > f1 else df)
                row[j] = (de, df, dh, tie_e, tie_f, a == diag, a > diag and e1 == f1, e1 > f1) if ties else (de, df, dh)
                Hc[j], Ec[j] = h, ev
                hnf_left = max(e1, diag)      # H without its F term
            Hprev, Eprev = Hc, Ec
            dirs.append(row)
        if mx >= score:
            break
        if band is not None:
            raise ValueError("banded maximum %d below the score %d at the given band %d" % (mx, score, bw))
        bw *= 2
    i, j, state, out, on_path = ql - 1, tl - 1, 2, [], []
    while i > 0 or j > 0:
        c = dirs[i][j]
        d = c[state]
        if ties:
            x = j - max(0, i - bw)
            if state == 0 and c[3]:
                on_path.append((i, j, x, "ee"))
            elif state == 1 and c[4]:
                on_path.append((i, j, x, "ff"))
            elif state == 2:
                if c[5]:
                    on_path.append((i, j, x, "hd"))
                elif c[6]:
                    on_path.append((i, j, x, "ef"))
                if d != 1 and (c[3] if c[7] else c[4]):
                    on_path.append((i, j, x, "ee" if c[7] else "ff"))
        if d == 1: i -= 1; j -= 1; state = 2; out.append("M")
        elif d == 2: i -= 1; state = 0; out.append("I")
        elif d == 3: i -= 1; state = 2; out.append("I")
        elif d == 4: j -= 1; state = 1; out.append("D")
        else: j -= 1; state = 2; out.append("D")
    out.append("M")
    s = "".join(reversed(out))
    return (s, on_path) if ties else s
