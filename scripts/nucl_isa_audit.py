"""Static audit of the two nucleotide alignment kernels (nucl_wave_kernel.hip, nucl_kernel.hip) in gfx950 assembly, no GPU:
registers, scratch, occupancy, LDS and the instruction count per kernel, and the instruction count of every innermost loop
that holds a marker instruction - `wave_ror:1` (the neighbour exchange of ksw_extz2_wave: its anti-diagonal loops) in the wave
kernel, `ds_write_b8` (the state of ksw_extz2 in LDS) in the 16-lane kernel.

    python scripts/nucl_isa_audit.py [--root TREE] [-o FILE]      TREE: a checkout to audit instead of this one

Instructions are the lines of the .s file that are not comments, directives or labels."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = (("nucl_wave_kernel.hip", "wave_ror:1"), ("nucl_kernel.hip", "ds_write_b32"))


def compile_s(root, src, out):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(root, "mmseqs2_amd", "csrc", src), "-o", out]
    return subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr


def instructions(path):
    """(text, is_label) of every label and instruction line, metadata left out"""
    rows, meta = [], False
    for line in open(path):
        s = line.split(";")[0].strip()
        if s.startswith(".amdgpu_metadata"):
            meta = True
        if meta or not s or s.startswith("//"):
            meta = meta and not s.startswith(".end_amdgpu_metadata")
            continue
        if s.endswith(":"):
            rows.append((s[:-1], True))
        elif not s.startswith("."):
            rows.append((s, False))
    return rows


def marked_loops(rows, marker):
    """instruction counts of the innermost loops (label ... backward branch to it) that hold `marker`, in source order"""
    at = {t: i for i, (t, lab) in enumerate(rows) if lab}
    loops = []
    for i, (t, lab) in enumerate(rows):
        m = None if lab else re.match(r"s_c?branch\S*\s+(\S+)$", t)
        if m and m.group(1) in at and at[m.group(1)] < i:
            loops.append((at[m.group(1)], i))
    out = []
    for i, (t, lab) in enumerate(rows):
        if not lab and marker in t:
            inner = min(((b - a, a, b) for a, b in loops if a < i <= b), default=None)
            if inner and inner[1:] not in out:
                out.append(inner[1:])
    return [sum(1 for t, lab in rows[a:b + 1] if not lab) for a, b in out]


def audit(root):
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for src, marker in KERNELS:
            s = os.path.join(tmp, src + ".s")
            rem = compile_s(root, src, s)
            get = lambda key: re.search(re.escape(key) + r":\s*(\d+)", rem).group(1)
            name = re.search(r"Function Name: (\S+)", rem).group(1)
            rows = instructions(s)
            lines.append("%s  (%s)" % (src, name))
            lines.append("  VGPRs %s  SGPRs %s  scratch %s  waves/SIMD %s  LDS %s B  instructions %d" % (
                get("VGPRs"), get("SGPRs"), get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"),
                get("LDS Size [bytes/block]"), sum(1 for t, lab in rows if not lab)))
            lines.append("  innermost loops with %s, instructions per body: %s" % (marker, marked_loops(rows, marker)))
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("-o", default=None)
    a = ap.parse_args()
    text = "\n".join(audit(a.root)) + "\n"
    sys.stdout.write(text)
    if a.o:
        open(a.o, "w").write(text)
