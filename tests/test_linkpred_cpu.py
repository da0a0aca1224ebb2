"""Link-prediction mini-batches on the CPU device (pg_edge_bits_update_cpu, pg_sample_*_excl_cpu,
pg_edge_lookup_cpu, pg_negative_sample_cpu and the dgl shim on them): the checks of
tests/linkpred_common.py. No GPU needed."""
import os
import shutil
import subprocess

import pytest

import linkpred_common as lc
from conftest import PKG

DEV = "cpu"


def test_exports():
    lc.check_exports()


@pytest.mark.parametrize("fanout", lc.FANOUTS)
def test_exclusion_equals_deletion(fanout):
    lc.check_exclusion(DEV, fanout)


def test_exclusion_empty_inputs():
    lc.check_exclusion_empty(DEV)


def test_edge_bits():
    lc.check_bits(DEV)


def test_edge_lookup():
    lc.check_lookup(DEV)


def test_negative_sample():
    lc.check_negatives(DEV)


def test_negative_sample_uniformity():
    lc.check_negative_uniformity()


def test_shim_edge_queries():
    lc.check_shim_queries(DEV)


def test_shim_sampling():
    lc.check_shim_sampling(DEV)


def test_negative_samplers():
    lc.check_negative_samplers(DEV)


def test_edge_loader():
    lc.check_edge_loader(DEV)


def test_link_prediction_end_to_end():
    lc.check_end_to_end(DEV)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_linkpred_hip_compiles_without_warnings(tmp_path):
    """csrc/linkpred.hip under the Makefile's flags with -Wall -Werror, and its place in HIP_SRCS."""
    mk = open(os.path.join(PKG, "Makefile")).read()
    hip_srcs = [ln for ln in mk.splitlines() if ln.startswith("HIP_SRCS")][0]
    assert "csrc/linkpred.hip" in hip_srcs
    flags = [ln for ln in mk.splitlines() if ln.startswith("HIPFLAGS :=")][0].split(":=")[1].split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc] + flags + ["-Werror", "-c", os.path.join(PKG, "csrc", "linkpred.hip"), "-o",
                                          str(tmp_path / "linkpred.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
