"""Neighbour sampling, block compaction, rectangular graphs and the dgl shim's blocks on the CPU
device (pg_sample_*_cpu, pg_block_compact_cpu and the *_cpu aggregation twins): the checks of
tests/block_common.py. No GPU needed."""
import os
import shutil
import subprocess

import pytest

import block_common as bc
from conftest import PKG

DEV = "cpu"
SHAPES = [(37, 11), (11, 37)]


def test_exports():
    bc.check_exports()


@pytest.mark.parametrize("fanout", bc.FANOUTS)
def test_sampler_properties_and_repeatability(fanout):
    bc.check_sampler(DEV, fanout)


def test_sampler_empty_inputs():
    bc.check_sampler_empty(DEV)


def test_sampler_many_seeds():
    bc.check_sampler_many_seeds(DEV)


def test_sampler_uniformity():
    bc.check_uniformity()


def test_block_compact():
    bc.check_compact(DEV)


@pytest.mark.parametrize("ns,nd", SHAPES)
def test_from_in_csr(ns, nd):
    bc.check_from_in_csr(ns, nd)


@pytest.mark.parametrize("ns,nd", SHAPES)
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("op", ["add", "sub", "mul", "div", "copy_lhs", "copy_rhs"])
def test_rect_gspmm(op, reduce, ns, nd):
    for family in ("grid", "gauss"):
        bc.check_rect_gspmm(DEV, ns, nd, op, reduce, family)


@pytest.mark.parametrize("ns,nd", SHAPES)
@pytest.mark.parametrize("op,reduce", [("mul", "sum"), ("add", "max"), ("copy_rhs", "min"), ("copy_lhs", "mean")])
def test_rect_gspmm_transposed(op, reduce, ns, nd):
    for family in ("grid", "gauss"):
        bc.check_rect_gspmm(DEV, ns, nd, op, reduce, family, transpose=True)


@pytest.mark.parametrize("ns,nd", SHAPES)
@pytest.mark.parametrize("lt,rt", [("u", "v"), ("v", "u"), ("u", "e"), ("e", "u"), ("v", "e"), ("e", "v")])
def test_rect_gsddmm(lt, rt, ns, nd):
    for family, op in (("grid", "div"), ("gauss", "mul"), ("gauss", "sub")):
        bc.check_rect_gsddmm(DEV, ns, nd, lt, rt, family, op=op)


@pytest.mark.parametrize("ns,nd", SHAPES)
def test_rect_heads_softmax_sddmm(ns, nd):
    bc.check_rect_heads(DEV, ns, nd)


@pytest.mark.parametrize("ns,nd", SHAPES)
def test_rect_aggregates_and_gatv2_score(ns, nd):
    bc.check_rect_aggregates(DEV, ns, nd)


def test_block_surface():
    bc.check_block_surface(DEV)


@pytest.mark.parametrize("ns,nd", SHAPES)
def test_block_update_all_apply_edges(ns, nd):
    bc.check_block_update_all(DEV, ns, nd)


def test_to_block():
    bc.check_to_block(DEV)


def test_sample_neighbors_shim():
    bc.check_sample_neighbors_shim(DEV)


def test_loader():
    bc.check_loader(DEV)


def test_full_neighbour_aggregations_bitwise():
    bc.check_full_aggregations_bitwise(DEV)


@pytest.mark.parametrize("pair", [False, True], ids=["tensor", "pair"])
@pytest.mark.parametrize("kind", bc.LAYERS)
def test_layers_match_full_graph(kind, pair):
    bc.check_layer_equivalence(DEV, kind, pair)


def test_block_layer_forms():
    bc.check_graphconv_both(DEV)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_sample_hip_compiles_without_warnings(tmp_path):
    """csrc/sample.hip under the Makefile's flags with -Wall -Werror, and its place in HIP_SRCS."""
    mk = open(os.path.join(PKG, "Makefile")).read()
    hip_srcs = [ln for ln in mk.splitlines() if ln.startswith("HIP_SRCS")][0]
    assert "csrc/sample.hip" in hip_srcs
    flags = [ln for ln in mk.splitlines() if ln.startswith("HIPFLAGS :=")][0].split(":=")[1].split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc] + flags + ["-Werror", "-c", os.path.join(PKG, "csrc", "sample.hip"), "-o",
                                          str(tmp_path / "sample.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
