"""The f16 forward scan of sw_half_kernel.hip in gfx950 assembly (scripts/sw_isa_audit.py --src sw_half_kernel.hip, no GPU
needed): what the packed f16 arithmetic with the three-way maximum is there for, per forward loop, against the int16 twin of
profiles/sw_isa_audit.txt - `sw_half_kernel<G,true>` against `sw_kernel<G,true>`, the kernels launch_sw can dispatch to (the
forward-only groups stay with the int16 kernels, sw_half_kernel.hip says why).

A row of two cells is 4 adds / subtractions, 3 three-way maxima and half a maximum for the column (two rows fold into one
three-way maximum): 7.5 packed ops against 9, and the running maximum of the column on top - pk <= 7.5 R + 2."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sw_isa_audit  # noqa: E402

pytestmark = pytest.mark.skipif(sw_isa_audit.find_hipcc() is None, reason="hipcc not found")

GROUPS = {0: (1, 12), 1: (13, 24), 2: (25, 28)}      # rows per lane of the single-tile kernel groups


@pytest.fixture(scope="module")
def audits():
    text, bad = sw_isa_audit.run(src="sw_half_kernel.hip", pk_per_row=7.5)
    assert bad == 0, "the audit's own check failed for %d loops" % bad
    twin = open(os.path.join(ROOT, "profiles", "sw_isa_audit.txt")).read()
    return sw_isa_audit.parse_records(twin), sw_isa_audit.parse_records(text)


def test_the_dispatched_kernels_and_all_their_loops_are_there(audits):
    _, (kern, loops) = audits
    assert set(kern) == {"sw_half_kernel<%d,true>" % g for g in GROUPS}
    for g, (lo, hi) in GROUPS.items():
        for R in range(lo, hi + 1):
            for d in ("half", "fwd", "rev"):      # the f16 scan, the int16 re-run of the marked pairs, the reverse scan
                assert ("sw_half_kernel<%d,true>" % g, d, R) in loops, (g, d, R)
    assert len(loops) == 3 * 28


def test_fewer_packed_ops_and_fewer_valu_than_the_int16_twin(audits):
    (_, tloops), (_, loops) = audits
    for g, (lo, hi) in GROUPS.items():
        for R in range(lo, hi + 1):
            rec, twin = loops[("sw_half_kernel<%d,true>" % g, "half", R)], tloops[("sw_kernel<%d,true>" % g, "fwd", R)]
            assert rec["pk"] <= 7.5 * R + 2, "R = %d: %d packed ops per column" % (R, rec["pk"])
            assert rec["valu"] < twin["valu"], "R = %d: %d VALU per column, the int16 twin has %d" % (R, rec["valu"], twin["valu"])


def test_wait_states_do_not_grow_with_the_rows(audits):
    _, (_, loops) = audits
    for g, (lo, hi) in GROUPS.items():
        nops = [loops[("sw_half_kernel<%d,true>" % g, "half", R)]["s_nop"] for R in range(lo, hi + 1)]
        assert max(nops) <= 1, "group %d: s_nop per column %s" % (g, nops)      # a constant, whatever R


def test_the_int16_loops_beside_it_are_the_twins_loops(audits):
    (_, tloops), (_, loops) = audits
    for (kernel, d, R), rec in loops.items():
        if d == "half":
            continue
        twin = tloops[(kernel.replace("sw_half_kernel", "sw_kernel"), d, R)]
        assert rec["pk"] == 9 * R and rec["valu"] <= twin["valu"] and rec["s_nop"] <= twin["s_nop"], (kernel, d, R, rec, twin)


def test_no_scratch_and_the_twins_wavefronts(audits):
    (tkern, _), (kern, _) = audits
    for name, rec in kern.items():
        twin = tkern[name.replace("sw_half_kernel", "sw_kernel")]
        assert rec["scratch"] == 0, "%s uses scratch" % name
        assert rec["occupancy"] >= twin["occupancy"], "%s: %d waves per SIMD, its twin has %d" % (name, rec["occupancy"], twin["occupancy"])
