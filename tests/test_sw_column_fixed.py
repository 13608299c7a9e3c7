"""The part of a Smith-Waterman column that does not depend on R (sw_kernel.hip: hand-off of H / F and of the letters, head
letters, boundary row of the multi-tile bodies), in gfx950 assembly: the built kernel file against the audit of the tree
before that part was cut, profiles/sw_isa_audit_before_fixed_part.txt (scripts/sw_isa_audit.py, one compile per module).

The falls asserted are the ones reached (profiles/sw_isa_audit.txt), so that a compiler that undoes a part
fails here:
  single-tile, R <= 6 forward      -2  VALU per column (zero-fill hand-off; the head letters are selected per column as before)
  single-tile, R <= 6 reverse      -8  (letter blocks, the column shifts the queue)
  single-tile, R >= 7              -9  (letter blocks, indexed); the one body without the row prefetch, sw_kernel<2,false>, -11
  multi-tile forward               -14 (R = 8 .. 10), -16 (R = 11 .. 16), -17 (R >= 17); v_mov -4 / -6 / -7
  multi-tile reverse               -15, but -13 at R = 9 and 10; v_mov -6, -4 at R = 9 and 10
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sw_isa_audit  # noqa: E402

pytestmark = pytest.mark.skipif(sw_isa_audit.find_hipcc() is None, reason="hipcc not found")

MULTI = ("sw_kernel<3,false>", "sw_kernel<3,true>", "sw_rev_multi_kernel")


def reached(kernel, d, R):
    """(fall of valu, fall of v_mov) per column that this body has to show against the audit before."""
    if kernel in MULTI:
        if d == "fwd":
            return (14, 4) if R <= 10 else ((16, 6) if R <= 16 else (17, 7))
        return (13, 4) if R in (9, 10) else (15, 6)
    if kernel == "sw_kernel<2,false>":
        return 11, 4
    if R <= 6:
        return (2, 2) if d == "fwd" else (8, 2)
    return 9, 3


@pytest.fixture(scope="module")
def audits():
    text, bad = sw_isa_audit.run()
    assert bad == 0, "the audit's own check failed: v_pk_* per column is not 9 R for %d loops" % bad
    before = open(os.path.join(ROOT, "profiles", "sw_isa_audit_before_fixed_part.txt")).read()
    return sw_isa_audit.parse_records(before), sw_isa_audit.parse_records(text)


def test_same_bodies(audits):
    (_, bloops), (_, loops) = audits
    assert set(loops) == set(bloops) and len(loops) == 147
    assert all(rec["skipped"] > 0 for rec in loops.values()), "the walk did not leave out the rare block of the new maximum"


def test_single_tile_bodies_lose_the_zero_fill_and_the_letter_work(audits):
    (_, bloops), (_, loops) = audits
    for key, rec in loops.items():
        if key[0] in MULTI:
            continue
        fall = reached(*key)[0]
        assert fall >= 2
        assert rec["valu"] <= bloops[key]["valu"] - fall, "%s: %d VALU per column, %d before, %d fewer expected" % (key, rec["valu"], bloops[key]["valu"], fall)


def test_multi_tile_bodies_lose_valu_and_moves(audits):
    (_, bloops), (_, loops) = audits
    for key, rec in loops.items():
        if key[0] not in MULTI:
            continue
        fall, moves = reached(*key)
        assert fall >= 1 and moves >= 1
        assert rec["valu"] <= bloops[key]["valu"] - fall, "%s: %d VALU per column, %d before, %d fewer expected" % (key, rec["valu"], bloops[key]["valu"], fall)
        assert rec["v_mov"] <= bloops[key]["v_mov"] - moves, "%s: %d v_mov per column, %d before, %d fewer expected" % (key, rec["v_mov"], bloops[key]["v_mov"], moves)


def test_no_wait_state_added(audits):
    (_, bloops), (_, loops) = audits
    for key, rec in loops.items():
        assert rec["s_nop"] <= bloops[key]["s_nop"], "%s: %d s_nop per column, %d before" % (key, rec["s_nop"], bloops[key]["s_nop"])


def test_no_wavefront_lost_and_no_scratch(audits):
    (bkern, _), (kern, _) = audits
    assert set(kern) == set(bkern)
    for name, rec in kern.items():
        assert rec["scratch"] == 0, "%s uses scratch" % name
        assert rec["occupancy"] >= bkern[name]["occupancy"], "%s: %d waves per SIMD, %d before" % (name, rec["occupancy"], bkern[name]["occupancy"])
