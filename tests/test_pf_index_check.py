"""The argument checks of mmgpu_pf_load_index / mmgpu_pf_build_index / mmgpu_db_load (pf_index_check, mmseqs2_amd/csrc/pf_index.h)
need no device: tests/pf_index_check.cpp calls them as a stand-alone program.  Rows that are not sorted, short row strides, a NULL
table, a bad k, offsets and entries that do not fit are refused with the entry point's name at the head of the message - and within a
modest address space: unsorted rows once sized the cumulative table from (first column - last column) before they were looked at."""
import os
import resource
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_argument_checks_on_the_host(tmp_path):
    lib = os.path.join(ROOT, "mmseqs2_amd", "lib")
    exe = str(tmp_path / "pf_index_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17",
                           "-I" + os.path.join(ROOT, "mmseqs2_amd", "csrc"), os.path.join(ROOT, "tests", "pf_index_check.cpp"), "-o", exe,
                           "-L" + lib, "-lmmgpu", "-Wl,-rpath," + lib])

    def limit():
        resource.setrlimit(resource.RLIMIT_AS, (8 << 30, 8 << 30))
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, preexec_fn=limit)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout
