"""The Smith-Waterman column loop in gfx950 assembly: conditions on what the compiler makes of sw_kernel.hip.

scripts/sw_isa_audit.py compiles the kernel file device-only (no GPU needed) and counts one column's straight path
per instantiation of sw_body.  The conditions below are what the source is written to achieve (sw_kernel.hip, phase 2
and the prefetch); a compiler that stops honouring the empty asm on the E update, or that puts the wait for the
profile rows back behind their reads, fails them.  The parent's counts are read from profiles/sw_isa_audit_parent.txt.

Bodies for which a condition is relaxed, and why (profiles/sw_isa_audit.txt has the counts):
  * multi-tile bodies with R = 8 .. 16 (`sw_kernel<3,*>`, `sw_rev_multi_kernel`; R < 14 exists only in builds with
    SW_MAX_R < 28): phase 2 has fewer independent ops of phase 1 left to put behind `t = h - go`, and the compiler
    leaves a wait state there in most rows (1 - 14 per column; the parent has 24 - 60).  Rows contribute none from R = 17 on, so
    the R-independence is checked between R = 17 and 28, and R = 8 .. 16 must stay at or below R - with the
    anchors that pair is the only dependent one left in a row, so one wait state per row is the most the rows can cost
    (R - 2 does not hold: 7 at R = 8, two of them in the fixed part) - and below the parent.
  * multi-tile forward bodies: one v_mov more per column than the parent (the zero the column maximum starts from is
    materialised for the anchor on cmax); allowed as + 1.
  * no prefetch in the multi-tile bodies and in `sw_kernel<2,false>` (sw_passes says why): condition 4 does not
    apply to them.
The double buffer of the prefetch needed no extra VALU instruction in any body: condition 2 holds without allowance.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sw_isa_audit  # noqa: E402

pytestmark = pytest.mark.skipif(sw_isa_audit.find_hipcc() is None, reason="hipcc not found")

SINGLE = {"sw_kernel<0,false>": (2, 12), "sw_kernel<0,true>": (2, 12), "sw_kernel<1,false>": (13, 24), "sw_kernel<1,true>": (13, 24),
          "sw_kernel<2,false>": (25, 28), "sw_kernel<2,true>": (25, 28)}
MULTI = ("sw_kernel<3,false>", "sw_kernel<3,true>", "sw_rev_multi_kernel")
NO_PREFETCH = MULTI + ("sw_kernel<2,false>",)


@pytest.fixture(scope="module")
def audits():
    text, bad = sw_isa_audit.run()
    assert bad == 0, "the audit's own check failed: v_pk_* per column is not 9 R for %d loops" % bad
    parent = open(os.path.join(ROOT, "profiles", "sw_isa_audit_parent.txt")).read()
    return sw_isa_audit.parse_records(parent), sw_isa_audit.parse_records(text)


def test_every_body_found(audits):
    (_, ploops), (_, loops) = audits
    assert set(loops) == set(ploops) and len(loops) == 147
    assert all(rec["pk_ok"] == 1 for rec in loops.values())


def test_rows_contribute_no_wait_states(audits):
    (_, ploops), (_, loops) = audits
    for kernel, (lo, hi) in SINGLE.items():
        for d in ("fwd", "rev"):
            if (kernel, d, lo) not in loops:
                assert d == "rev" and kernel.endswith("false>")      # forward-only kernels have no reverse body
                continue
            a, b = loops[(kernel, d, lo)]["s_nop"], loops[(kernel, d, hi)]["s_nop"]
            assert abs(a - b) <= 2, "%s %s: %d s_nop at R = %d, %d at R = %d" % (kernel, d, a, lo, b, hi)
    for kernel in MULTI:
        d = "rev" if kernel == "sw_rev_multi_kernel" else "fwd"
        a, b = loops[(kernel, d, 17)]["s_nop"], loops[(kernel, d, 28)]["s_nop"]
        assert abs(a - b) <= 2, "%s %s: %d s_nop at R = 17, %d at R = 28" % (kernel, d, a, b)
        for R in range(8, 17):      # relaxed (see the docstring): the one dependent pair a row can still hold, t -> f', R times at most
            n, p = loops[(kernel, d, R)]["s_nop"], ploops[(kernel, d, R)]["s_nop"]
            assert n <= R and n < p, "%s %s R = %d: %d s_nop (bound R), the parent has %d" % (kernel, d, R, n, p)


def test_no_more_valu_than_the_parent(audits):
    (_, ploops), (_, loops) = audits
    for key, rec in loops.items():
        allow = 1 if key[0] in ("sw_kernel<3,false>", "sw_kernel<3,true>") else 0
        assert rec["valu"] <= ploops[key]["valu"] + allow, "%s: %d VALU per column, the parent has %d" % (key, rec["valu"], ploops[key]["valu"])


def test_no_scratch_and_no_wavefront_lost(audits):
    (pkern, _), (kern, _) = audits
    assert set(kern) == set(pkern)
    for name, rec in kern.items():
        assert rec["scratch"] == 0, "%s uses scratch" % name
        assert rec["occupancy"] >= pkern[name]["occupancy"], "%s: %d waves per SIMD, the parent has %d" % (name, rec["occupancy"], pkern[name]["occupancy"])


def test_no_lds_wait_behind_the_prefetch(audits):
    _, (_, loops) = audits
    for key, rec in loops.items():
        if key[0] in NO_PREFETCH:
            continue
        assert rec["lgkm_wait_within2"] == 0, "%s: s_waitcnt lgkmcnt within two instructions of the last ds_read" % (key,)
