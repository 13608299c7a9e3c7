"""GPU parity tests (pytest -m gpu) of mmgpu_sw_traceback - backtrace string and identity count, what the alignment path writes
into result databases under -a - over the parameter table of tests/sw_param_cases.py, every band class and doubling class, both
kernels (the wave kernel bt_wave_kernel.hip and the lane-per-alignment kernel bt_kernel.hip with all its tiers), the fallback
when the wave kernel's direction pool runs out, MMGPU_BT_TOO_LARGE as a required answer, and the contract of the call.
References: the reference's own recorded strings (tests/golden/sw_param_vectors.npz) and the plain-C restatement
(oracle/sw_oracle.c, pinned to those strings by tests/test_sw_params.py); which class a case reached is proven from the
restatement's final band (tests/bt_cases.py).  Bar: bit-exact status, string, ident, bt_len - no tolerances.
MMGPU_BT_FAILED is not constructed (the reference reads unrelated memory there: no defined output); the tests assert that it
never appears where the restatement returns a string."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mmseqs2_amd import workloads as wl
from mmseqs2_amd.capi import SW_BT_DTYPE, _ptr
from tests import bt_cases as bc
from tests import sw_param_cases as pc
from tests.rescore import rescore

pytestmark = pytest.mark.gpu

MMGPU_OK, MMGPU_ERR_ARG, MMGPU_ERR_STATE = 0, -1, -3      # include/mmgpu.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [s[0] for s in pc.SW_PARAM_SETS]


@pytest.fixture(scope="module")
def param_sets():
    return pc.load_param_vectors()


def _case(oracle, v, label, q, t, cb=None):
    return dict(label=label, q=q, cb=cb, t=t, r=oracle.sw_align(q, cb, t, v["mat"], v["go"], v["ge"], need_start=True, need_bt=True))


def _trace_counts(err):
    """the library's MMGPU_TRACE lines of mmgpu_sw_traceback -> (wave jobs, wave declined, pool MB, {tier: [jobs, moved up]})"""
    wave = [(int(a), int(b), float(c)) for a, b, c in re.findall(r"\[sw_traceback\] wave kernel: (\d+) jobs, (\d+) declined, pool ([\d.]+) MB", err)]
    tiers = {}
    for t, n, m in re.findall(r"\[sw_traceback\] tier (\d): (\d+) jobs, (\d+) moved up", err):
        tiers.setdefault(int(t), [0, 0])
        tiers[int(t)][0] += int(n)
        tiers[int(t)][1] += int(m)
    return sum(w[0] for w in wave), sum(w[1] for w in wave), max([w[2] for w in wave], default=0.0), tiers


# ---- a. the reference's own strings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_reference_strings_on_device(gpu, param_sets, key):
    """Every recorded pair of the set at its matrix, gap costs and recorded composition bias: where the reference recorded a
    string the device returns status 0 and that string and identity count, and the string re-scores to the device's own (score,
    q_end, t_end) at the set's costs.  At least 10 compared strings per set contain a gap."""
    v = param_sets[key]
    cases = [dict(label="golden_%d" % i, q=q, cb=cb, t=t) for i, (q, cb, t, exp) in enumerate(v["pairs"])]
    b = bc.run_cases(gpu, v, cases)
    res = b.fetch()
    info, strs = b.traceback(np.arange(len(cases), dtype=np.uint32))
    b.free()
    n = n_gap = 0
    for i, (q, cb, t, exp) in enumerate(v["pairs"]):
        assert [int(res[i][f]) for f in ("score", "q_end", "t_end", "q_start", "t_start", "word")] == [int(x) for x in exp[:6]], (key, i)
        if not v["bt"][i]:
            assert int(info[i]["status"]) == bc.BT_NO_START and strs[i] == "", (key, i, int(info[i]["status"]))
            continue
        assert int(info[i]["status"]) == bc.BT_OK, (key, i, int(info[i]["status"]))
        assert strs[i] == v["bt"][i], (key, i, strs[i][:80], v["bt"][i][:80])
        assert int(info[i]["ident"]) == int(exp[6]) and int(info[i]["bt_len"]) == len(v["bt"][i]), (key, i)
        s, qe, te = rescore(q, cb, t, v["mat"], v["go"], v["ge"], int(res[i]["q_start"]), int(res[i]["t_start"]), strs[i])
        assert (s, qe, te) == (int(res[i]["score"]), int(res[i]["q_end"]), int(res[i]["t_end"])), (key, i)
        n += 1
        n_gap += ("I" in strs[i]) or ("D" in strs[i])
    print("%s: %d reference strings compared, %d with gaps" % (key, n, n_gap))
    assert n_gap >= 10, (key, n, n_gap)


# ---- b. parameter sets x band classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_parameter_sets_across_band_classes(gpu, oracle, param_sets, key):
    """The generator's pairs (bt_cases.band_cases: offsetting indels, one-sided gaps, homologs, periodic, with X), every second
    query with its composition bias from the set's own matrix, queries outside the acceptance rule not sent (at most 20 %).
    Status 0 and the restatement's string / ident for EVERY pair with a start position.  blosum62_11_1 populates every band class
    (the bands 512 and 601 lie beyond the wave kernel: last tier of the lane kernel) and every doubling class; every other set
    at least one doubling, three and more doublings, a band row of several chunks and a band in 257..511."""
    v = param_sets[key]
    full = key == "blosum62_11_1"
    cases, n_refused = bc.band_cases(oracle, v, 500 + sum(map(ord, key)), wide=full)
    b = bc.run_cases(gpu, v, cases)
    tally, bad = bc.check_traceback(b, cases, key)
    b.free()
    print("%s: %s; %d pairs outside the acceptance rule" % (key, tally, n_refused))
    assert not bad, bad[:5]
    assert n_refused <= pc.MAX_REFUSED_SHARE * (len(cases) + n_refused), (key, n_refused)
    assert tally.n == sum(1 for c in cases if c["r"]["bt"]) and tally.n >= 40 and tally.with_bias >= 40
    d, bands = tally.doublings, tally.band
    if full:
        assert all(n > 0 for n in d.values()) and all(bands[c] > 0 for c in bc.BAND_CLASSES), str(tally)
    assert d["1"] + d["2"] + d[">=3"] >= 1 and d[">=3"] >= 1 and tally.multi_chunk >= 1 and tally.wide128 >= 1 and bands["257..511"] >= 1, str(tally)


# ---- c. engineered ties on chunk boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["blosum62_11_1", "blosum62_5_2"])
def test_engineered_ties_on_chunk_boundaries(gpu, oracle, param_sets, key):
    """Ties built into one alignment - H between the diagonal and a gap ('hd', rule: the diagonal), a gap between being opened
    and being extended ('ee' in the query, 'ff' in the target; rule: extended), H between E and F ('ef', rule: F unless E is strictly greater) - with the tie cell
    62, 63, 64, 65, 127 and 128 cells from the row's first band column, in rows of 513 cells: on both sides of the wave kernel's
    chunk boundaries, where its carries (f_carry / hnf_carry / hd_carry) decide.  bt_cases.tie_cases keeps a pair only when the
    walk over the restatement's string consults that tie in that cell; the counts below keep the constructions from decaying.
    'ef' has no construction at 5/2 (|min score| = 4 = 2 gap_extend: mismatches never cost more than two gaps) - skipped there,
    and said so in the output."""
    v = param_sets[key]
    cases, skipped = bc.tie_cases(oracle, v)
    kinds = [k for k in bc.TIE_KINDS if k not in skipped]
    print("%s: tie constructions %s, skipped %s" % (key, kinds, skipped))
    assert kinds == (["hd", "ee", "ff", "ef"] if key == "blosum62_11_1" else ["hd", "ee", "ff"])
    assert sorted((c["kind"], c["x"]) for c in cases) == sorted((k, x) for k in kinds for x in bc.TIE_OFFSETS)
    b = bc.run_cases(gpu, v, cases)
    tally, bad = bc.check_traceback(b, cases, key)
    b.free()
    print("%s: %s" % (key, tally))
    assert not bad, bad[:5]
    assert tally.n == len(cases) and tally.wide128 == len(cases)


# ---- d. the lane kernel alone ----------------------------------------------------------------------------------------------------
def test_lane_kernel_alone(gpu):
    """MMGPU_BT_LANE_KERNEL=1 (the library reads it once per process: a child process, one, with a time limit, not retried): the
    cases of (b) for three sets, the engineered ties of (c) at 11/1 and two profile-query pairs through the lane-per-alignment kernel only, compared with the
    restatement by the child (tests/bt_gpu_check.py).  From the library's trace: no wave kernel ran, tiers 0 (rows in LDS), 2
    and 3 (rows in scratch) each ran jobs, and jobs whose band doubled beyond their tier moved up."""
    env = dict(os.environ, MMGPU_BT_LANE_KERNEL="1", MMGPU_TRACE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bt_gpu_check.py")], env=env, cwd=ROOT, timeout=420,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(p.stdout[-3000:])
    print("\n".join(l for l in p.stderr.splitlines() if "[sw_traceback]" in l and ("tier" in l or "wave" in l)))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    rep = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rep["mismatches"] == 0 and rep["compared"] >= 150 and rep["profile_pairs"] == 2, rep
    n_off = len(bc.TIE_OFFSETS)          # every engineered tie compared equal in the lane kernel: 'ef' is its `hsel` rule
    assert rep["ties"] == dict(hd=n_off, ee=n_off, ff=n_off, ef=n_off), rep["ties"]
    assert "wave kernel:" not in p.stderr
    _, _, _, tiers = _trace_counts(p.stderr)
    print("lane kernel alone: tier -> [jobs, moved up]", tiers)
    assert all(tiers.get(t, [0, 0])[0] > 0 for t in (0, 2, 3)), tiers
    assert sum(m for _, m in tiers.values()) > 0, tiers


# ---- e. the wave kernel's direction pool runs out ----------------------------------------------------------------------------------
def test_direction_pool_exhaustion_falls_back_to_the_lane_kernel(gpu, oracle, param_sets, monkeypatch, capfd):
    """1200 offsetting-indel targets (g = 100) of one 700-residue query in one call.  Depends on these constants of
    mmgpu_sw_traceback (mmgpu_api.hip): the pool is max(sum over the jobs of rows * (2 * min(4 * initial band, 510) + 1) bytes,
    64 MB floor), capped at 8 GB; the wave kernel bumps `dir_cursor` by rows * (2 * final band + 1) and declines a job that passes
    `dir_pool_bytes`.  Here the initial band is 1 and the final band 128: the estimate is ~6 KB a pair (7.5 MB: the 64 MB floor
    holds), a pair needs 700 * 257 B = 180 KB, so about 370 pairs fit and the rest must come back from the lane kernel (tier 0
    -> 1 -> 2: band 128 needs rows in scratch).  Every pair: status 0 and the restatement's string; `declined > 0` from the
    library's trace, so that a larger pool makes this test fail instead of silently testing nothing."""
    v = param_sets["blosum62_11_1"]
    rng = np.random.default_rng(12)
    a, b_, c, ins = (bc._bg(rng, n) for n in (200, 200, 200, 100))
    q = np.concatenate([a, ins, b_, c])
    assert len(q) == 700
    targets = [np.concatenate([bc._subs(rng, a, 0.9), bc._subs(rng, b_, 0.9), bc._bg(rng, 100), bc._subs(rng, c, 0.9)]) for _ in range(1200)]
    tres, toff = wl.seqs_from_list(targets)
    gpu.load_targets(tres, toff, 21)
    batch = gpu.sw_prepare(v["mat"], 11, 1, [dict(q=q, comp_bias=None, targets=np.arange(1200, dtype=np.uint32), min_start_score=0)], mode=1)
    batch.run()
    cases = [_case(oracle, v, "pool_%d" % k, q, t) for k, t in enumerate(targets)]
    assert all(c["r"]["band"] == 128 and c["r"]["q_end"] - c["r"]["q_start"] + 1 >= 650 for c in cases)
    monkeypatch.setenv("MMGPU_TRACE", "1")
    capfd.readouterr()
    tally, bad = bc.check_traceback(batch, cases, "pool")
    err = capfd.readouterr().err
    monkeypatch.delenv("MMGPU_TRACE")
    batch.free()
    jobs, declined, pool_mb, tiers = _trace_counts(err)
    print("pool exhaustion: wave kernel %d jobs, %d declined, pool %.1f MB; lane kernel tier -> [jobs, moved up] %s" % (jobs, declined, pool_mb, tiers))
    print("pool exhaustion: %s" % tally)
    assert not bad, bad[:5]
    assert tally.n == 1200
    assert jobs == 1200 and declined > 0, (jobs, declined, pool_mb)
    assert tiers.get(2, [0, 0])[0] == declined, (declined, tiers)


# ---- f. wide bands -----------------------------------------------------------------------------------------------------------------
def test_wide_bands_and_too_large(gpu, oracle, param_sets):
    """Band 601 (one-sided gap of 600 between 700-residue flanks) is beyond the wave kernel's 511 and must come back with status
    0 through the lane kernel's 8195-word tier.  A band above 4096 (gap of 4200) and a pair whose direction words exceed the last
    tier (band 2001, 5000 rows: 501 words a row) must answer exactly MMGPU_BT_TOO_LARGE with bt_len 0 - the host then runs
    banded_sw itself - without touching their neighbours in the call, and the context serves a normal call afterwards."""
    v = param_sets["blosum62_11_1"]
    rng = np.random.default_rng(21)
    normal = [bc.homolog_pair(rng, 200, 400) for _ in range(3)]
    pairs = [("normal_0",) + normal[0], ("band_601",) + bc.one_sided_pair(rng, 700, 600), ("normal_1",) + normal[1],
             ("band_4201",) + bc.one_sided_pair(rng, 1200, 4200, identity=1.0), ("band_2001_5000_rows",) + bc.one_sided_pair(rng, 2500, 2000, identity=0.85),
             ("normal_2",) + normal[2]]
    cases = [_case(oracle, v, label, q, t) for label, q, t in pairs]
    by = {c["label"]: bc.classify(c["r"]) for c in cases}
    assert all(0 < c["r"]["score"] < 32767 for c in cases), [c["r"]["score"] for c in cases]
    assert by["band_601"]["band"] == 601 and by["band_4201"]["band"] == 4201, by
    assert by["band_2001_5000_rows"]["band"] == 2001 and by["band_2001_5000_rows"]["rows"] >= 5000, by
    want = [bc.required_status(by[c["label"]]["rows"], by[c["label"]]["band"]) for c in cases]
    assert want == [0, 0, 0, 1, 1, 0], want
    b = bc.run_cases(gpu, v, cases)
    info, strs = b.traceback(np.arange(len(cases), dtype=np.uint32))
    for k in (3, 4):
        assert int(info[k]["status"]) == bc.BT_TOO_LARGE and int(info[k]["bt_len"]) == 0 and strs[k] == "", (k, info[k])
    tally, bad = bc.check_traceback(b, cases, "wide")
    b.free()
    print("wide bands: %s; statuses %s" % (tally, info["status"].tolist()))
    assert not bad, bad
    assert tally.n == 4 and tally.band["512..4096"] == 1
    after = [_case(oracle, v, "after_%d" % k, q, t) for k, (q, t) in enumerate(normal)]
    b = bc.run_cases(gpu, v, after)
    tally, bad = bc.check_traceback(b, after, "after too-large")
    b.free()
    assert not bad and tally.n == 3, bad


# ---- g. degenerate rectangles --------------------------------------------------------------------------------------------------------
def test_degenerate_rectangles(gpu, oracle, param_sets):
    """A 1 x 1 alignment (string "M"), alone and inside a long target; a pair aligned end to end (start 0, end the last residue of
    both); a query of two tiles whose alignment crosses the tile boundary; a target containing X.  1 x n and n x 1 rectangles with
    n > 1 do not exist under the rule: a local alignment neither begins nor ends with a gap, so a rectangle of one row has one
    column."""
    v = param_sets["blosum62_11_1"]
    rng = np.random.default_rng(33)
    wi = int(np.argmax(np.diag(v["mat"])[:20]))        # W: the only positive score of its row / column besides W|F, W|Y
    w = np.array([wi], np.uint8)
    long_t = bc._bg(rng, 300)
    long_t[(v["mat"][wi][long_t] > 0) | (v["mat"][:, wi][long_t] > 0)] = 0
    assert int(v["mat"][wi, 0]) < 0
    long_t[150] = wi
    s = bc._bg(rng, 300)
    q2 = bc._bg(rng, 700)
    _, tile_rows, n_tiles = pc.strip_geometry(700)
    assert n_tiles == 2
    cross = wl.mutate(rng, q2[tile_rows - 100:tile_rows + 100], 0.85, max_indels=4, max_indel_len=12)
    tx = wl.mutate(rng, s, 0.9, max_indels=3, max_indel_len=8)
    tx[rng.random(len(tx)) < 0.06] = 20
    cases = [_case(oracle, v, "one_by_one", w, w), _case(oracle, v, "one_row_long_target", w, long_t), _case(oracle, v, "long_query_one_column", long_t, w),
             _case(oracle, v, "end_to_end", s, s.copy()), _case(oracle, v, "across_tiles", q2, cross), _case(oracle, v, "target_with_x", s, tx)]
    r = {c["label"]: c["r"] for c in cases}
    assert r["one_by_one"]["bt"] == "M" and r["one_row_long_target"]["bt"] == "M" and r["long_query_one_column"]["bt"] == "M"
    assert (r["one_row_long_target"]["t_start"], r["long_query_one_column"]["q_start"]) == (150, 150)
    assert (r["end_to_end"]["q_start"], r["end_to_end"]["t_start"], r["end_to_end"]["q_end"], r["end_to_end"]["t_end"]) == (0, 0, 299, 299)
    assert r["end_to_end"]["bt"] == "M" * 300 and r["end_to_end"]["ident"] == 300
    assert r["across_tiles"]["q_start"] < tile_rows - 20 and r["across_tiles"]["q_end"] > tile_rows + 20
    assert 20 in tx[r["target_with_x"]["t_start"]:r["target_with_x"]["t_end"] + 1]
    b = bc.run_cases(gpu, v, cases)
    tally, bad = bc.check_traceback(b, cases, "degenerate")
    b.free()
    assert not bad and tally.n == len(cases), bad


# ---- h. the contract of the call -------------------------------------------------------------------------------------------------------
def _raw(gpu, b, idx, cap=None, with_buffer=True):
    """mmgpu_sw_traceback as the C ABI has it -> (rc, info, buffer, *bt_used)"""
    idx = np.ascontiguousarray(idx, np.uint32)
    info = np.zeros(max(len(idx), 1), SW_BT_DTYPE)
    used = ctypes.c_size_t(0)
    buf = np.zeros(max(cap or 0, 1), np.uint8)
    rc = gpu.L.mmgpu_sw_traceback(gpu.ctx, b.handle, _ptr(idx), len(idx), _ptr(info), _ptr(buf) if with_buffer and cap else None, cap or 0,
                                  ctypes.byref(used))
    return rc, info[:len(idx)], buf, used.value


def _contract_cases(oracle, v, rng):
    cases = [_case(oracle, v, "homolog_%d" % k, *bc.homolog_pair(rng, 150, 400)) for k in range(5)]
    unrelated = bc._bg(rng, 60)
    unrelated[:] = 0                               # A against W: no positive cell
    cases.append(_case(oracle, v, "score_0", unrelated, np.full(50, 17, np.uint8)))
    weak_q = bc._bg(rng, 200)
    weak_t = bc._bg(rng, 200)
    weak_t[90:96] = weak_q[40:46]
    cases.append(_case(oracle, v, "weak", weak_q, weak_t))
    return cases


def test_call_contract(gpu, oracle, param_sets):
    """States and arguments: a mode-0 batch and a batch never run -> MMGPU_ERR_STATE; an index >= pairs -> MMGPU_ERR_ARG; a buffer
    one byte short -> MMGPU_ERR_ARG with *bt_used = the sum of the reservations; n_pairs == 0 is OK; one pair named three times
    gives three equal strings at distinct offsets; bt_off runs back to back in pair_index order with (q_end - q_start + 1) +
    (t_end - t_start + 1) + 1 bytes per pair that has a start position; a score-0 pair and a pair below min_start_score ->
    status 3; a second run() of the batch and a second traceback() give the same answers."""
    v = param_sets["blosum62_11_1"]
    cases = _contract_cases(oracle, v, np.random.default_rng(41))
    assert cases[5]["r"]["score"] == 0 and 0 < cases[6]["r"]["score"] < 70 and all(c["r"]["score"] >= 70 for c in cases[:5])
    tres, toff = wl.seqs_from_list([c["t"] for c in cases])
    gpu.load_targets(tres, toff, 21)
    queries = [dict(q=c["q"], comp_bias=None, targets=np.array([i], np.uint32), min_start_score=70) for i, c in enumerate(cases)]
    b0 = gpu.sw_prepare(v["mat"], 11, 1, queries, mode=0)
    b0.run()
    assert _raw(gpu, b0, [0], cap=4096)[0] == MMGPU_ERR_STATE
    b0.free()
    b = gpu.sw_prepare(v["mat"], 11, 1, queries, mode=1)
    assert _raw(gpu, b, [0], cap=4096)[0] == MMGPU_ERR_STATE          # never run
    b.run()
    res = b.fetch()
    n = len(cases)
    assert _raw(gpu, b, [0, n], cap=1 << 20)[0] == MMGPU_ERR_ARG
    assert _raw(gpu, b, [], cap=16)[0] == MMGPU_OK
    order = np.array([3, 5, 0, 3, 6, 1, 3, 4, 2], np.uint32)
    sizes = [0 if p in (5, 6) else int(res[p]["q_end"] - res[p]["q_start"] + 1) + int(res[p]["t_end"] - res[p]["t_start"] + 1) + 1 for p in order.tolist()]
    total = sum(sizes)
    rc, _, _, used = _raw(gpu, b, order, cap=total - 1)
    assert rc == MMGPU_ERR_ARG and used == total, (rc, used, total)
    rc, _, _, used = _raw(gpu, b, order, cap=0, with_buffer=False)
    assert rc == MMGPU_ERR_ARG and used == total
    rc, info, buf, used = _raw(gpu, b, order, cap=total)
    assert rc == MMGPU_OK and used == total
    assert info["bt_off"].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    strs = [bytes(buf[int(r["bt_off"]):int(r["bt_off"]) + int(r["bt_len"])]).decode() for r in info]
    for k, p in enumerate(order.tolist()):
        r = cases[p]["r"]
        if p in (5, 6):
            assert int(info[k]["status"]) == bc.BT_NO_START and int(info[k]["bt_len"]) == 0, (k, p, info[k])
            assert (int(res[p]["q_start"]), int(res[p]["t_start"])) == (-1, -1)
        else:
            assert int(info[k]["status"]) == bc.BT_OK and strs[k] == r["bt"] and int(info[k]["ident"]) == r["ident"], (k, p)
            assert int(info[k]["bt_len"]) < sizes[k]
    three = [k for k, p in enumerate(order.tolist()) if p == 3]
    assert len(three) == 3 and len({strs[k] for k in three}) == 1 and len({int(info[k]["bt_off"]) for k in three}) == 3
    # a second run of the batch, then the same question
    b.run()
    rc, info2, buf2, _ = _raw(gpu, b, order, cap=total)
    assert rc == MMGPU_OK and np.array_equal(info2, info) and np.array_equal(buf2[:total], buf[:total])
    b.free()


def test_host_copy_follows_reverse_pairs_and_block_starts(gpu, oracle, param_sets):
    """mmgpu_sw_traceback works from a host copy of the batch's records.  In a mode-2 batch the int16-range hits (word == 1) have
    no start position: status 3.  mmgpu_sw_reverse_pairs fills some in - the copy has to follow: status 0 and the restatement's
    string for exactly those, still 3 for the others.  The same for a fresh batch after mmgpu_sw_block_starts: status 0 for every
    int16-range pair; the string is compared for the pairs the block aligner declined (their start is the reverse scan's) and
    for the pairs whose block-aligner start IS the reverse scan's - where the block aligner starts elsewhere the rectangle is
    not banded_sw's and the reference has no string for it.  (No pair of these families is declined by the restatement's block
    aligner - long gaps, saturated hits and 400 homologs were tried - so the declined branch is asserted by count only.)"""
    v = param_sets["blosum62_11_1"]
    rng = np.random.default_rng(43)
    cases = [_case(oracle, v, "word_%d" % k, *bc.homolog_pair(rng, 250, 500)) for k in range(10)]
    cases += [_case(oracle, v, "gap_%d" % k, *bc.one_sided_pair(rng, 180, 400 + 150 * k, identity=0.95)) for k in range(6)]
    cases += [_case(oracle, v, "short_%d" % k, *bc.homolog_pair(rng, 20, 40)) for k in range(4)]
    word = np.array([c["r"]["word"] == 1 for c in cases])
    assert word.sum() >= 10 and (~word).sum() >= 2
    b = bc.run_cases(gpu, v, cases, mode=2)
    everything = np.arange(len(cases), dtype=np.uint32)
    info, strs = b.traceback(everything)
    assert (info["status"][word] == bc.BT_NO_START).all() and (info["status"][~word] == bc.BT_OK).all(), info["status"].tolist()
    pick = np.nonzero(word)[0][::2].astype(np.uint32)
    b.reverse_pairs(pick)
    info, strs = b.traceback(everything)
    filled = ~word
    filled[pick] = True
    assert (info["status"][filled] == bc.BT_OK).all() and (info["status"][~filled] == bc.BT_NO_START).all(), info["status"].tolist()
    _, bad = bc.check_traceback(b, cases, "after reverse_pairs", pick=np.nonzero(filled)[0])
    b.free()
    assert not bad, bad[:5]
    # block_starts: the declined pairs
    b = bc.run_cases(gpu, v, cases, mode=2)
    info, _ = b.traceback(everything)
    assert (info["status"][word] == bc.BT_NO_START).all()
    n_sel, n_declined, n_large = b.block_starts()
    blk = [oracle.block_backtrace(c["q"], None, c["t"], v["mat"], 11, 1, c["r"]["score"], c["r"]["q_end"], c["r"]["t_end"]) if word[k] else None
           for k, c in enumerate(cases)]
    declined = [k for k in np.nonzero(word)[0].tolist() if not blk[k]["ok"]]
    same = [k for k in np.nonzero(word)[0].tolist() if blk[k]["ok"] and (blk[k]["q_start"], blk[k]["t_start"]) == (cases[k]["r"]["q_start"], cases[k]["r"]["t_start"])]
    print("block_starts: selected %d, declined %d (restatement: %d), too large %d; %d accepted pairs start where the reverse scan starts" % (
        n_sel, n_declined, len(declined), n_large, len(same)))
    assert n_sel == int(word.sum()) and n_declined == len(declined) and len(same) + len(declined) >= 8
    res = b.fetch()
    for k in np.nonzero(word)[0].tolist():
        exp = (blk[k]["q_start"], blk[k]["t_start"]) if blk[k]["ok"] else (cases[k]["r"]["q_start"], cases[k]["r"]["t_start"])
        assert (int(res[k]["q_start"]), int(res[k]["t_start"])) == exp, (k, res[k], exp)
    info, _ = b.traceback(everything)
    assert (info["status"] != bc.BT_NO_START).all(), info["status"].tolist()      # every pair has a start now, and the copy knows it
    pick = np.array(declined + same + np.nonzero(~word)[0].tolist(), np.uint32)
    tally, bad = bc.check_traceback(b, cases, "after block_starts", pick=pick)
    b.free()
    assert not bad and tally.n == len(pick), bad[:5]
