"""pg_sddmm_dot_cpu and the edge-weight gradients it serves, on the CPU device: the kernel
against a float64 reference within the summation-order bar, and every autograd path that
used to raise (ops.SumAggregate / ops.MaxAggregate) or return None (ops.SagePool) for a
weight that requires grad against a float64 torch composition on the edge list
(tests/sddmm_common.py holds the references and the bars)."""
import numpy as np
import pytest
import torch

import sddmm_common as sc
from conftest import hub_graph, random_graph

DEV = "cpu"


def _graph(name):
    import plagnn

    if name == "random":
        src, dst = random_graph(300, 2000)
        return plagnn.CSRGraph(src, dst, 300)
    src, dst = hub_graph(200, 700)
    return plagnn.CSRGraph(src, dst, 200, chunk=4)


@pytest.fixture(scope="module", params=["random", "hub_chunk4"])
def graph(request):
    return _graph(request.param)


@pytest.mark.parametrize("form", ["plain", "mean", "max"])
@pytest.mark.parametrize("F", [1, 3, 40])
def test_sddmm_dot_cpu_within_bar(graph, F, form):
    from plagnn import ops

    g, dg = graph, graph.on(DEV)
    rng = np.random.default_rng(F)
    D = rng.standard_normal((g.num_nodes, F)).astype(np.float32)
    X = rng.standard_normal((g.num_nodes, F)).astype(np.float32)
    Dt, Xt = torch.from_numpy(D), torch.from_numpy(X)
    argpos = ops.spmm_max(dg, Xt)[1] if form == "max" else None
    de = ops.sddmm_dot(dg, Dt, Xt, mean=form == "mean", argpos=argpos)
    assert de.shape == (g.num_edges,) and de.dtype == torch.float32
    ref, bar = sc.sddmm_ref(g, D, X, mean=form == "mean", argpos=argpos)
    sc.assert_within(de, ref, bar, f"{form} F={F}")
    if form == "max":  # every (row, feature) has exactly one winner: nothing lost, nothing doubled
        terms = D.astype(np.float64) * ops.spmm_max(dg, Xt)[0].numpy()
        assert abs(de.double().sum().item() - terms.sum()) <= 1e-5 * np.abs(terms).sum()


@pytest.mark.parametrize("kind", ["sum", "mean", "max"])
def test_aggregate_ops_edge_weight_grad(kind, monkeypatch):
    sc.check_aggregate_ops(DEV, kind, monkeypatch)


@pytest.mark.parametrize("reduce_op", ["sum", "mean", "max"])
def test_update_all_u_mul_e_edge_weight_grad(reduce_op, monkeypatch):
    sc.check_update_all(DEV, reduce_op, monkeypatch)


@pytest.mark.parametrize("zero_w", [False, True], ids=["positive_w", "zero_w"])
def test_sage_pool_edge_weight_grad(zero_w, monkeypatch):
    sc.check_sage_pool(DEV, 10, 6, monkeypatch, zero_w=zero_w)


@pytest.mark.parametrize("fin,fout", [(12, 5), (5, 12)], ids=["lin_before_mp", "lin_after_mp"])
def test_sage_mean_edge_weight_grad(fin, fout):
    sc.check_sage_mean(DEV, fin, fout)


@pytest.mark.parametrize("fin,fout", [(12, 5), (5, 12)], ids=["w_first", "aggregate_first"])
def test_graphconv_edge_weight_grad(fin, fout):
    sc.check_graphconv(DEV, fin, fout)


def test_apply_edges_u_dot_v():
    sc.check_u_dot_v(DEV)


def test_apply_edges_rejects_other_functions():
    import dgl
    import dgl.function as fn

    g = dgl.graph((torch.tensor([0, 1]), torch.tensor([1, 2])), num_nodes=3)
    g.ndata["h"] = torch.ones(3, 2)
    with pytest.raises(NotImplementedError):
        g.apply_edges(lambda edges: {"s": edges.src["h"]})
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.copy_u("h", "m"))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.u_dot_v("h", "h", "m"), fn.sum("m", "o"))


def test_version_stays_13():
    from plagnn import _lib

    assert _lib.lib().pg_version() == 13


def test_error_returns():
    from plagnn import _lib
    from plagnn._lib import ptr

    g = _graph("random")
    s = g.on(DEV).fwd.struct(None)
    n, F = g.num_nodes, 8
    D, X = torch.zeros(n, F), torch.zeros(n, F)
    de = torch.zeros(g.num_edges)
    with pytest.raises(_lib.PlagnnError, match="norm_mode"):
        _lib.call("pg_sddmm_dot_cpu", s, ptr(D), F, ptr(X), F, F, 2, None, 0, _lib.PG_ARG_U16, ptr(de))
    with pytest.raises(_lib.PlagnnError, match="leading"):
        _lib.call("pg_sddmm_dot_cpu", s, ptr(D), F, ptr(X), F - 1, F, 0, None, 0, _lib.PG_ARG_U16, ptr(de))
    a = torch.zeros(n, F, dtype=torch.int16)
    with pytest.raises(_lib.PlagnnError, match="arg_kind"):
        _lib.call("pg_sddmm_dot_cpu", s, ptr(D), F, ptr(X), F, F, 0, ptr(a), F, 7, ptr(de))
    # empty shapes are fine
    _lib.call("pg_sddmm_dot_cpu", s, ptr(D), F, ptr(X), F, 0, 0, None, 0, _lib.PG_ARG_U16, ptr(de))
