"""The wide Smith-Waterman bodies (32-lane groups, sw_body.h) in gfx950 assembly, against the 16-lane bodies of the same R in the
same kernels: one compile per kernel file (scripts/sw_isa_audit.py, no GPU needed), audited once for each kind.

A wide body is the 16-lane single-tile body of its R with one more move per hand-off - `v_mov_b32_dpp ... wave_shr:1` behind each of
the three `row_shr:1` of a column - and nothing else: three VALU instructions more per column, the same packed ops, no wait state
more than one, no LDS read more, no scratch, and the kernels keep their wavefronts (profiles/sw_wide_isa_audit.txt)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sw_isa_audit  # noqa: E402

pytestmark = pytest.mark.skipif(sw_isa_audit.find_hipcc() is None, reason="hipcc not found")

WIDE_R = range(15, 29)          # ceil(449 / 32) .. ceil(896 / 32)


def _group(R):
    return 1 if R <= 24 else 2


@pytest.fixture(scope="module", params=["sw_kernel.hip", "sw_half_kernel.hip"])
def audits(request, tmp_path_factory):
    src = request.param
    asm = str(tmp_path_factory.mktemp("asm") / (src + ".s"))
    sw_isa_audit.compile_asm(asm, src=src)
    pk = 7.5 if src == "sw_half_kernel.hip" else 9.0
    narrow, bad_n = sw_isa_audit.run(asm=asm, src=src, pk_per_row=pk)
    wide, bad_w = sw_isa_audit.run(asm=asm, src=src, pk_per_row=pk, wide=True)
    assert bad_n == 0 and bad_w == 0
    committed = open(os.path.join(ROOT, "profiles", "sw_isa_audit.txt" if src == "sw_kernel.hip" else "sw_half_isa_audit.txt")).read()
    return src, sw_isa_audit.parse_records(narrow), sw_isa_audit.parse_records(wide), sw_isa_audit.parse_records(committed)


def _expected_keys(src):
    keys = set()
    for R in WIDE_R:
        if src == "sw_kernel.hip":
            keys |= {("sw_kernel<%d,false>" % _group(R), "fwd", R), ("sw_kernel<%d,true>" % _group(R), "fwd", R), ("sw_kernel<%d,true>" % _group(R), "rev", R)}
        else:
            keys |= {("sw_half_kernel<%d,true>" % _group(R), d, R) for d in ("half", "fwd", "rev")}
    return keys


def test_every_wide_body_is_there_and_no_other(audits):
    src, _, (_, wide), _ = audits
    assert set(wide) == _expected_keys(src)
    assert all(rec["pk_ok"] == 1 and rec["skipped"] > 0 for rec in wide.values())


def test_a_wide_column_is_the_16_lane_column_plus_three_moves(audits):
    _, (_, narrow), (_, wide), _ = audits
    for key, rec in wide.items():
        twin = narrow[key]
        # the forward-only body without the row prefetch (sw_kernel<2,false>, sw_passes says why) gets a register copy beside the
        # three moves: four; it has no wait state left in exchange
        more = 4 if key[0] == "sw_kernel<2,false>" else 3
        assert rec["valu"] == twin["valu"] + more and rec["v_mov"] == twin["v_mov"] + more, (key, rec, twin)
        assert rec["pk"] == twin["pk"] and rec["perm"] == twin["perm"] and rec["ds_read"] == twin["ds_read"], (key, rec, twin)
        assert rec["s_nop"] <= max(twin["s_nop"], 1) and rec["lgkm_wait_within2"] <= twin["lgkm_wait_within2"], (key, rec, twin)


def test_the_16_lane_bodies_are_the_committed_ones(audits):
    _, (_, narrow), _, (_, committed) = audits
    assert set(narrow) == set(committed)
    for key, rec in narrow.items():
        for f in ("instr", "valu", "pk", "perm", "ds_read", "s_nop", "v_mov", "s_waitcnt", "lgkm_wait_within2"):
            assert rec[f] == committed[key][f], (key, f, rec[f], committed[key][f])


def test_no_scratch_and_the_groups_wavefronts(audits):
    _, (kern, _), _, (ckern, _) = audits
    assert set(kern) == set(ckern)
    for name, rec in kern.items():
        assert rec["scratch"] == 0, "%s uses scratch" % name
        assert rec["occupancy"] == ckern[name]["occupancy"], "%s: %d waves per SIMD, %d before the wide bodies" % (name, rec["occupancy"], ckern[name]["occupancy"])
