"""mmseqs2_amd/csrc/block_plan.h - which path a pair takes through the block aligner's launches: head size, pool groups, pairs
handed on, tier slots - with limits a few dozen jobs cross (tests/block_plan_check.cpp).  Plain g++, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_plan_properties(tmp_path):
    exe = str(tmp_path / "block_plan_check")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # with the address and undefined-behaviour sanitizers where a trivial program links with their runtimes
    if subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + san, stderr=subprocess.DEVNULL).returncode != 0:
        san = []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "mmseqs2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "block_plan_check.cpp"), "-o", exe] + san)
    for seed in (1, 2, 3):
        out = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout
