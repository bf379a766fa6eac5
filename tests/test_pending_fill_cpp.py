"""The pending-zero-fill table of the HIP library (iterative-solver_amd/csrc/pending_fill.h) alone, on
the CPU: tests/cpp/pending_fill_test.cpp is compiled with g++ into a stand-alone program, the way
tests/test_host_layer_cpp.py builds its programs (with its sanitizer flags when ITSOLV_SAN_FLAGS is
set), and run.  The header includes nothing of HIP; the stores the table asks for are only recorded.
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.environ.get("ITSOLV_SAN_FLAGS", "").split()  # tools/asan_cpu.sh: the sanitizer build
INC = ["-I" + os.path.join(ROOT, "iterative-solver_amd", "csrc")]

CASES = ("exact_match", "overlap_queries", "partial_overlap_left_and_right_is_flushed", "full_cover_is_dropped",
         "erase_inside_freed_block", "overflow_at_65_inserts", "drain_order", "entries_stay_disjoint")


def test_pending_fill_table():
    exe = os.path.join(tempfile.mkdtemp(), "t")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *SAN, *INC,
                        os.path.join(HERE, "cpp", "pending_fill_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK 0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    for name in CASES:
        assert "PASS " + name in r.stdout
    assert r.stdout.count("PASS ") == len(CASES)
