#!/usr/bin/env python3
"""Static audit of the Smith-Waterman column loop (mmseqs2_amd/csrc/sw_kernel.hip) in gfx950 assembly.

Compiles sw_kernel.hip device-only to assembly with the Makefile's flags (no GPU needed, about 40 s), finds the
innermost loops that hold the three `row_shr:1` hand-off moves - one per instantiation of sw_body - and counts
what one column costs a wavefront: instructions, VALU, packed ops, LDS reads, wait states (`s_nop`), moves and
waits.  Per kernel it prints the register count, the occupancy the compiler states and scratch use.

What is counted is the straight path of a column: conditional branches fall through (the boundary-row load and
store of the multi-tile bodies are on the path), and the block under the `s_and_saveexec` / `s_cbranch_execz` of
the rarely taken `nm != vmax` branch (running maximum, snapshot / row search) is skipped.

    python scripts/sw_isa_audit.py                 # compile and print the audit
    python scripts/sw_isa_audit.py -o FILE         # ... into a file (profiles/sw_isa_audit.txt)
    python scripts/sw_isa_audit.py --asm FILE.s    # audit an assembly file made earlier
    python scripts/sw_isa_audit.py -D MMGPU_SW_WAVES_G1B=3
    python scripts/sw_isa_audit.py --src sw_half_kernel.hip --pk-per-row 7.5 -o profiles/sw_half_isa_audit.txt
    python scripts/sw_isa_audit.py --wide [--src ...]   # the bodies of 32-lane groups instead of the 16-lane ones

The wide bodies (a group of 32 lanes, sw_body.h) follow each `row_shr:1` move with a `wave_shr:1` move that carries the value
across the DPP row boundary: a loop that holds three of those is a wide body.  They sit in the same kernels under the same
R as the 16-lane bodies, so an audit lists one kind or the other: the 16-lane bodies by default (the committed audits and
the tests that compare against them), the wide ones with --wide.

--src names another file of mmseqs2_amd/csrc that instantiates sw_body (sw_half_kernel.hip: the f16 forward scan).  Its f16
loops - the ones that hold v_pk_maximum3_f16 - are listed as dir=half, and the tool's own check on them is
pk <= PK_PER_ROW * R + 2 (--pk-per-row); the int16 loops are always held to pk = 9 R.

The `LOOP` and `KERNEL` lines are `key=value` records: tests/test_sw_isa_audit.py reads them (parse_records).
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmseqs2_amd", "csrc")


def find_hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M)
    if not m:
        raise RuntimeError("no FLAGS line in mmseqs2_amd/csrc/Makefile")
    return m.group(1).split()


def compile_asm(out_path, defines=(), src="sw_kernel.hip"):
    hipcc = find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    cmd = [hipcc] + makefile_flags() + ["-D" + d for d in defines] + [
        "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out_path]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed (exit %d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-4000:]))


def kernel_name(sym):
    if "sw_rev_multi_kernel" in sym:
        return "sw_rev_multi_kernel"
    m = re.search(r"(sw_kernel|sw_half_kernel)ILi(\d+)ELb([01])E", sym)
    if m:
        return "%s<%s,%s>" % (m.group(1), m.group(2), "true" if m.group(3) == "1" else "false")
    if "sw_from_pf_kernel" in sym:
        return "sw_from_pf_kernel"
    return sym


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")


def split_functions(lines):
    """[(symbol, first line, last line)] of every function of the assembly file."""
    out, start, sym = [], None, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            sym, start = m.group(1), i
        elif l.startswith(".Lfunc_end") and sym:
            out.append((sym, start, i))
            sym = None
    return out


def is_instr(l):
    s = l.strip()
    return bool(s) and l[0] in " \t" and not s.startswith((";", "."))


def mnemonic(l):
    return l.split()[0]


def walk_column(lines, labels, head):
    """Instructions of the straight path of one trip through the loop whose header label is at line `head`.

    Conditional branches fall through, unconditional ones are followed (the compiler may rotate the loop, so that
    the header sits in the middle of its blocks); the trip ends where control is back at the header."""
    name = LABEL.match(lines[head]).group(1)
    path, skipped, i, seen = [], 0, head + 1, set()
    while i < len(lines) and i not in seen:
        seen.add(i)
        l = lines[i]
        if i == head:
            return path, skipped, True
        if l.startswith(".Lfunc_end"):
            break
        if not is_instr(l):
            i += 1
            continue
        path.append(l.strip())
        b = BRANCH.match(l)
        if b:
            kind, target = b.group(1), b.group(2)
            if target == name:
                return path, skipped, True
            tl = labels.get(target, -1)
            if kind == "s_branch" and tl >= 0:
                i = tl
                continue
            if kind == "s_cbranch_execz" and tl >= 0 and len(path) >= 3 and path[-2].startswith("s_and_saveexec"):
                # the rare maximum branch: exec mask straight from the compare of the new maximum with the old
                prev = [p for p in path[-5:-2] if not p.startswith("s_nop")]
                mask = prev[-1].split()[1].rstrip(",") if prev and prev[-1].startswith("v_cmp_ne_u32") else None
                if mask and path[-2].split()[-1] == mask:      # (vcc, or the SGPR pair the compare wrote)
                    k = i + 1   # size of the skipped block: up to the join label or the branch that leaves it
                    while k < len(lines) and k != tl and not lines[k].startswith(".Lfunc_end"):
                        if is_instr(lines[k]):
                            skipped += 1
                            if lines[k].split()[0] == "s_branch":
                                break
                        k += 1
                    i = tl
                    continue
        i += 1
    return path, skipped, False


def audit_loop(path):
    c = collections.Counter()
    c["instr"] = len(path)
    for p in path:
        m = mnemonic(p)
        if m.startswith("v_"):
            c["valu"] += 1
        if m.startswith("v_pk_"):
            c["pk"] += 1
        if m == "v_perm_b32":
            c["perm"] += 1
        if m == "v_pk_maximum3_f16":
            c["max3_f16"] += 1
        if m.startswith("ds_read"):
            c["ds_read"] += 1
        if m == "s_nop":
            c["s_nop"] += 1
        if m.startswith("v_mov"):
            c["v_mov"] += 1
        if m == "s_waitcnt":
            c["s_waitcnt"] += 1
        if m == "v_bitop3_b32" and "0xca" in p:
            c["select"] += 1
    reads = [k for k, p in enumerate(path) if mnemonic(p).startswith("ds_read")]
    c["lgkm_wait_within2"] = 0
    if reads:
        after = path[reads[-1] + 1:reads[-1] + 3]
        c["lgkm_wait_within2"] = int(any(a.startswith("s_waitcnt") and "lgkmcnt" in a for a in after))
    pairs = collections.Counter()
    for k, p in enumerate(path):
        if mnemonic(p) == "s_nop":
            before = next((mnemonic(q) for q in reversed(path[:k]) if mnemonic(q) != "s_nop"), "-")
            after = next((mnemonic(q) for q in path[k + 1:] if mnemonic(q) != "s_nop"), "-")
            pairs[(before, after)] += 1
    return c, pairs


def audit(asm_path):
    lines = open(asm_path).read().split("\n")
    kernels, loops = [], []
    for sym, a, b in split_functions(lines):
        name = kernel_name(sym)
        if not name.startswith(("sw_kernel", "sw_half_kernel")) and name != "sw_rev_multi_kernel":
            continue
        labels = {}
        for i in range(a, b):
            m = LABEL.match(lines[i])
            if m:
                labels[m.group(1)] = i
        # kernel facts: the .amdhsa block and the comment block behind the function
        info = {"kernel": name, "vgpr": None, "occupancy": None, "scratch": None}
        for i in range(b, min(b + 60, len(lines))):
            m = re.search(r"; ScratchSize:\s*(\d+)", lines[i])
            if m:
                info["scratch"] = int(m.group(1))
            m = re.search(r"; Occupancy:\s*(\d+)", lines[i])
            if m:
                info["occupancy"] = int(m.group(1))
                break
        for i in range(b, a, -1):
            m = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", lines[i])
            if m:
                info["vgpr"] = int(m.group(1))
                break
        kernels.append(info)
        for lab, i in sorted(labels.items(), key=lambda kv: kv[1]):
            head = "".join(lines[i:i + 4])
            if "Inner Loop Header" not in head:
                continue
            path, skipped, closed = walk_column(lines, labels, i)
            if not closed or sum("row_shr:1" in p for p in path) != 3:
                continue
            wide = sum("wave_shr:1" in p for p in path)
            if wide not in (0, 3):
                continue
            c, pairs = audit_loop(path)
            R = c["perm"]
            direction = "rev" if c["select"] >= R and R > 0 else ("half" if c["max3_f16"] else "fwd")
            loops.append(dict(kernel=name, label=lab, dir=direction, R=R, wide=wide == 3,
                              counts=c, pairs=pairs, skipped=skipped))
    return kernels, loops


FIELDS = ["instr", "valu", "pk", "perm", "ds_read", "s_nop", "v_mov", "s_waitcnt", "lgkm_wait_within2"]


def report(kernels, loops, out, src="sw_kernel.hip", pk_per_row=9.0, wide=False):
    w = out.write
    loops = [lp for lp in loops if lp["wide"] == wide]
    if wide:
        w("# The bodies of 32-lane groups (three wave_shr:1 moves per column beside the three row_shr:1).\n")
    w("# SW column loop audit (scripts/sw_isa_audit.py): gfx950 assembly of mmseqs2_amd/csrc/%s, Makefile flags\n" % src)
    w("# Per loop: one column's straight path.  Skipped: the block under s_and_saveexec / s_cbranch_execz of the rare\n")
    w("# `nm != vmax` branch (its instruction count is given as skipped=).  R is the v_perm_b32 count of the loop.\n")
    w("# pk must be 9 R (the tool's own check): pk_ok=1.\n")
    if any(lp["dir"] == "half" for lp in loops):
        w("# dir=half: the f16 forward loops (they hold v_pk_maximum3_f16); their check is pk <= %g R + 2.\n" % pk_per_row)
    w("\n")
    for k in kernels:
        w("KERNEL kernel=%s vgpr=%s occupancy=%s scratch=%s\n" % (k["kernel"], k["vgpr"], k["occupancy"], k["scratch"]))
    w("\n")
    bad = 0
    for lp in sorted(loops, key=lambda d: (d["kernel"], d["dir"], d["R"])):
        c = lp["counts"]
        ok = int(c["pk"] <= pk_per_row * lp["R"] + 2 if lp["dir"] == "half" else c["pk"] == 9 * lp["R"])
        bad += 1 - ok
        w("LOOP kernel=%s dir=%s R=%d %s skipped=%d pk_ok=%d label=%s\n" % (
            lp["kernel"], lp["dir"], lp["R"], " ".join("%s=%d" % (f, c[f]) for f in FIELDS), lp["skipped"], ok, lp["label"]))
    w("\n# what stands before -> after the s_nop's of each loop (count x before -> after)\n")
    for lp in sorted(loops, key=lambda d: (d["kernel"], d["dir"], d["R"])):
        w("NOPS kernel=%s dir=%s R=%d:" % (lp["kernel"], lp["dir"], lp["R"]))
        if not lp["pairs"]:
            w(" none")
        for (b, a), n in sorted(lp["pairs"].items(), key=lambda kv: -kv[1]):
            w(" %dx %s->%s;" % (n, b, a))
        w("\n")
    return bad


def parse_records(text):
    """The KERNEL and LOOP records of an audit file: ({kernel: {...}}, {(kernel, dir, R): {...}})."""
    kernels, loops = {}, {}
    for line in text.split("\n"):
        if not line.startswith(("KERNEL ", "LOOP ")):
            continue
        rec = {}
        for tok in line.split()[1:]:
            k, _, v = tok.partition("=")
            rec[k] = int(v) if re.fullmatch(r"-?\d+", v) else v
        if line.startswith("KERNEL "):
            kernels[rec["kernel"]] = rec
        else:
            loops[(rec["kernel"], rec["dir"], rec["R"])] = rec
    return kernels, loops


def run(defines=(), asm=None, src="sw_kernel.hip", pk_per_row=9.0, wide=False):
    """Audit text of the tree (or of an assembly file made earlier)."""
    import io
    if asm is None:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sw_kernel.s")
            compile_asm(path, defines, src)
            kernels, loops = audit(path)
    else:
        kernels, loops = audit(asm)
    buf = io.StringIO()
    bad = report(kernels, loops, buf, src, pk_per_row, wide)
    return buf.getvalue(), bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="audit this assembly file instead of compiling")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra -D for the compile")
    ap.add_argument("-o", dest="out", help="write the audit here instead of stdout")
    ap.add_argument("--src", default="sw_kernel.hip", help="file of mmseqs2_amd/csrc to audit (default sw_kernel.hip)")
    ap.add_argument("--pk-per-row", type=float, default=9.0, help="v_pk_* per row the f16 loops may hold (dir=half); default 9")
    ap.add_argument("--wide", action="store_true", help="list the bodies of 32-lane groups instead of the 16-lane ones")
    a = ap.parse_args()
    text, bad = run(a.defines, a.asm, a.src, a.pk_per_row, a.wide)
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    if bad:
        sys.stderr.write("sw_isa_audit: %d loops whose v_pk_* count is not what is expected - the loop walk is wrong for them\n" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
