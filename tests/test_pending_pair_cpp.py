"""The pair of pending gemm_outer records of the HIP library (OuterPair in
iterative-solver_amd/csrc/pending_outer.h) alone, on the CPU: tests/cpp/pending_pair_test.cpp is compiled
with g++ into a stand-alone program, the way tests/test_pending_outer_cpp.py builds its program (with its
sanitizer flags when ITSOLV_SAN_FLAGS is set), and run.  The header includes nothing of HIP; the launches
the records ask for are only recorded.
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.environ.get("ITSOLV_SAN_FLAGS", "").split()  # tools/asan_cpu.sh: the sanitizer build
INC = ["-I" + os.path.join(ROOT, "iterative-solver_amd", "csrc")]

CASES = ("pair_and_flush", "pairing_conditions", "register_term_or_not", "unpair_is_the_single_record_state",
         "unpair_without_terms", "touches", "discard")


def test_pending_pair():
    exe = os.path.join(tempfile.mkdtemp(), "t")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *SAN, *INC,
                        os.path.join(HERE, "cpp", "pending_pair_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK 0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    for name in CASES:
        assert "PASS " + name in r.stdout
    assert r.stdout.count("PASS ") == len(CASES)
