"""Neighbour sampling (pg_sample_count / pg_sample_fill), block compaction (pg_block_compact),
rectangular graphs in the HIP aggregation kernels, and the dgl shim's blocks, samplers, loader
and bipartite layers on the GPU: the checks of tests/block_common.py with DEV = cuda. The
sampler and the compaction must equal their CPU twins bit for bit."""
import pytest

import block_common as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(37, 11), (11, 37)]


@pytest.mark.parametrize("fanout", bc.FANOUTS)
def test_sampler_equals_cpu_twin(fanout):
    bc.check_sampler(DEV, fanout)


def test_sampler_empty_inputs():
    bc.check_sampler_empty(DEV)


def test_sampler_many_seeds():
    bc.check_sampler_many_seeds(DEV)


def test_block_compact_equals_cpu_twin():
    bc.check_compact(DEV)


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
