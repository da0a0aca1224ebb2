"""ASan + UBSan run of the link-prediction host entry points: tests/sanitize_linkpred/
san_linkpred.cpp, a stand-alone program built with csrc/graph.cpp and csrc/cpu_backend.cpp, drives
pg_edge_bits_update_cpu, pg_sample_count_excl_cpu / pg_sample_fill_excl_cpu, pg_edge_lookup_cpu
and pg_negative_sample_cpu on the sampler's edge-case graph with exactly-sized buffers; any
sanitizer report fails the process. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sanitize_linkpred")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_linkpred_cpu_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               OMP_NUM_THREADS="4")
    r = subprocess.run([os.path.join(HERE, "build", "san_linkpred")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sanitize linkpred ok" in r.stdout
