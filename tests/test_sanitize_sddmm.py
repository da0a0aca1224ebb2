"""ASan + UBSan run of pg_sddmm_dot_cpu: tests/sanitize_sddmm/san_sddmm.cpp, a stand-alone
program built with csrc/graph.cpp and csrc/cpu_backend.cpp, builds hub graphs through the
C-ABI's host calls and runs the three forms and both record kinds against a double-precision
loop; any sanitizer report fails the process. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sanitize_sddmm")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sddmm_cpu_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               OMP_NUM_THREADS="4")
    r = subprocess.run([os.path.join(HERE, "build", "san_sddmm")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sanitize sddmm ok" in r.stdout
