"""ASan + UBSan run of the multi-head attention host entry points: tests/sanitize_gat/san_gat.cpp,
a stand-alone program built with csrc/graph.cpp and csrc/cpu_backend.cpp, builds hub graphs
through the C-ABI's host calls and runs pg_edge_softmax_fwd_cpu / _bwd_cpu, pg_spmm_sum_heads_cpu
(both CSR directions) and pg_sddmm_dot_heads_cpu for H in {1, 3, 8} against double-precision
loops; any sanitizer report fails the process. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sanitize_gat")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gat_cpu_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               OMP_NUM_THREADS="4")
    r = subprocess.run([os.path.join(HERE, "build", "san_gat")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sanitize gat ok" in r.stdout
