"""pg_sddmm_dot on the GPU (the per-edge dot products behind the edge-weight gradients of
u_mul_e aggregations and apply_edges(u_dot_v)): every kernel path against a float64
reference within the summation-order bar of tests/sddmm_common.py, determinism, agreement
with the CPU entry point, HIP-graph capture, and the autograd / shim checks of
test_sddmm_cpu.py on the device."""
import numpy as np
import pytest
import torch

import sddmm_common as sc
from conftest import hub_graph, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hub():
    """hub_graph(500, 700): with the default chunk of 256 the hub row splits into three items."""
    import plagnn

    src, dst = hub_graph(500, 700)
    g = plagnn.CSRGraph(src, dst, 500)
    assert g.fwd.n_items >= g.num_nodes + 2
    return g


def _operands(g, F, seed=0, relu=False):
    rng = np.random.default_rng(1000 * seed + F)
    D = rng.standard_normal((g.num_nodes, F)).astype(np.float32)
    X = rng.standard_normal((g.num_nodes, F)).astype(np.float32)
    if relu:
        X = np.maximum(X, 0)
    return D, X


def _run(g, D, X, name, mean=False, argpos=None, Dt=None, Xt=None):
    from plagnn import ops

    dg = g.on(DEV)
    Dt = sc.to_dev(D, DEV) if Dt is None else Dt
    Xt = sc.to_dev(X, DEV) if Xt is None else Xt
    de = ops.sddmm_dot(dg, Dt, Xt, mean=mean, argpos=argpos)
    assert de.shape == (g.num_edges,) and de.dtype == torch.float32
    ref, bar = sc.sddmm_ref(g, D, X, mean=mean, argpos=argpos)
    sc.assert_within(de, ref, bar, name)
    return de, ref, bar


# one lane, the scalar tail, the vector path, a partial last lane, exactly one tile, one tile
# plus 4, two tiles plus 4
@pytest.mark.parametrize("F", [1, 3, 4, 40, 64, 67, 256, 260, 516])
def test_width_sweep(hub, F):
    D, X = _operands(hub, F)
    _run(hub, D, X, f"plain F={F}")


@pytest.mark.parametrize("F", [40, 260])
def test_unaligned_operands_take_the_scalar_path(hub, F):
    n = hub.num_nodes
    D, X = _operands(hub, F, seed=1)
    # a row stride of F + 1
    Db = torch.zeros(n, F + 1, device=DEV)
    Xb = torch.zeros(n, F + 1, device=DEV)
    Db[:, :F], Xb[:, :F] = sc.to_dev(D, DEV), sc.to_dev(X, DEV)
    _run(hub, D, X, f"stride F+1, F={F}", Dt=Db[:, :F], Xt=Xb[:, :F])
    # a base pointer offset by 4 bytes
    Df = torch.zeros(n * F + 1, device=DEV)
    Xf = torch.zeros(n * F + 1, device=DEV)
    Dv, Xv = Df[1:].view(n, F), Xf[1:].view(n, F)
    Dv.copy_(sc.to_dev(D, DEV))
    Xv.copy_(sc.to_dev(X, DEV))
    assert Dv.data_ptr() % 16 == 4
    _run(hub, D, X, f"base + 4 B, F={F}", Dt=Dv, Xt=Xv)


@pytest.mark.parametrize("F", [3, 40, 260])
def test_tiny_items(F):
    """CSRGraph(chunk=4): many items are shorter than the U = 8 edges gathered at once."""
    import plagnn
    from plagnn import ops

    src, dst = hub_graph(500, 700)
    g = plagnn.CSRGraph(src, dst, 500, chunk=4)
    D, X = _operands(g, F, seed=2)
    _run(g, D, X, f"chunk 4 plain F={F}")
    _run(g, D, X, f"chunk 4 mean F={F}", mean=True)
    argpos = ops.spmm_max(g.on(DEV), sc.to_dev(X, DEV))[1]
    _run(g, D, X, f"chunk 4 max F={F}", argpos=argpos)


@pytest.mark.parametrize("F", [3, 40])
def test_zero_in_degree_rows(F):
    import plagnn
    from plagnn import ops

    src, dst = random_graph(300, 900, self_loop=False)
    g = plagnn.CSRGraph(src, dst, 300)
    assert (g.in_degrees() == 0).any()
    D, X = _operands(g, F, seed=3)
    _run(g, D, X, f"zero in-degree plain F={F}")
    _run(g, D, X, f"zero in-degree mean F={F}", mean=True)
    argpos = ops.spmm_max(g.on(DEV), sc.to_dev(X, DEV))[1]
    _run(g, D, X, f"zero in-degree max F={F}", argpos=argpos)


def test_empty_shapes(hub):
    import plagnn
    from plagnn import ops

    g0 = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    de = ops.sddmm_dot(g0.on(DEV), torch.ones(5, 8, device=DEV), torch.ones(5, 8, device=DEV))
    assert de.shape == (0,)
    n = hub.num_nodes
    de = ops.sddmm_dot(hub.on(DEV), torch.ones(n, 0, device=DEV), torch.ones(n, 0, device=DEV))
    torch.cuda.synchronize()
    assert de.shape == (hub.num_edges,) and not de.any()  # an empty sum


@pytest.mark.parametrize("F", [40, 260])
def test_mean_form(hub, F):
    D, X = _operands(hub, F, seed=4)
    _run(hub, D, X, f"mean F={F}", mean=True)


@pytest.mark.parametrize("weighted", [False, True], ids=["copy_u", "u_mul_e"])
@pytest.mark.parametrize("F", [3, 40, 260])
def test_max_form_u16(hub, F, weighted):
    from plagnn import ops

    dg = hub.on(DEV)
    assert dg.arg_dtype == torch.int16
    D, X = _operands(hub, F, seed=5)
    w = None
    if weighted:
        w = sc.to_dev(np.random.default_rng(F).uniform(-1.0, 1.0, hub.num_edges).astype(np.float32), DEV)
    out, argpos = ops.spmm_max(dg, sc.to_dev(X, DEV), w)
    de, _, _ = _run(hub, D, X, f"max u16 F={F} weighted={weighted}", argpos=argpos)
    if not weighted:  # every (row, feature) has exactly one winner: nothing lost, nothing doubled
        terms = D.astype(np.float64) * out.cpu().numpy()
        assert abs(de.double().sum().item() - terms.sum()) <= 1e-5 * np.abs(terms).sum()


def test_max_form_i32():
    """64 nodes, node 0 with 70,000 in-edges: positions do not fit u16 records."""
    import plagnn
    from plagnn import _lib, ops

    n, F = 64, 8
    rng = np.random.default_rng(6)
    src = np.concatenate([rng.integers(0, n, 70000), np.arange(n)])
    dst = np.concatenate([np.zeros(70000, np.int64), np.arange(n)])
    g = plagnn.CSRGraph(src, dst, n)
    assert g.arg_kind == _lib.PG_ARG_I32
    D, X = _operands(g, F, seed=6)
    argpos = ops.spmm_max(g.on(DEV), sc.to_dev(X, DEV))[1]
    assert argpos.dtype == torch.int32
    _run(g, D, X, "max i32", argpos=argpos)
    _run(g, D, X, "plain, 70,000-entry row")


@pytest.mark.parametrize("F", [40, 260])
def test_max_form_dead_none_records(hub, F):
    """Dead-none records (no winner where the maximum is 0) are accepted. Without weights and
    with X >= 0 the dropped entries have X[u,f] = 0, so the result equals the plain records'
    everywhere; with weights (some of them 0) it follows the records it was given."""
    from plagnn import ops

    dg = hub.on(DEV)
    D, X = _operands(hub, F, seed=7, relu=True)
    Xt = sc.to_dev(X, DEV)
    plain = ops.spmm_max(dg, Xt)[1]
    out, dead = ops.spmm_max(dg, Xt, dead_none=True)
    assert (sc.argpos_np(dead) < 0).any() and not (sc.argpos_np(plain) < 0).any()
    de_dead, _, _ = _run(hub, D, X, f"dead-none F={F}", argpos=dead)
    de_plain, _, _ = _run(hub, D, X, f"plain records F={F}", argpos=plain)
    assert bool((de_dead == de_plain).all())
    w = np.random.default_rng(F).uniform(0.1, 1.0, hub.num_edges).astype(np.float32)
    w[::3] = 0.0
    dead_w = ops.spmm_max(dg, Xt, sc.to_dev(w, DEV), dead_none=True)[1]
    _run(hub, D, X, f"dead-none weighted F={F}", argpos=dead_w)


@pytest.mark.parametrize("form", ["plain", "mean", "max"])
def test_deterministic_and_matches_cpu_entry_point(hub, form):
    from plagnn import ops

    F = 260
    D, X = _operands(hub, F, seed=8)
    Dt, Xt = sc.to_dev(D, DEV), sc.to_dev(X, DEV)
    dg = hub.on(DEV)
    argpos = ops.spmm_max(dg, Xt)[1] if form == "max" else None
    a = ops.sddmm_dot(dg, Dt, Xt, mean=form == "mean", argpos=argpos)
    b = ops.sddmm_dot(dg, Dt, Xt, mean=form == "mean", argpos=argpos)
    assert torch.equal(a, b), "two calls on the same inputs differ"
    cpu = ops.sddmm_dot(hub.on("cpu"), torch.from_numpy(D), torch.from_numpy(X), mean=form == "mean",
                        argpos=None if argpos is None else argpos.cpu())
    _, bar = sc.sddmm_ref(hub, D, X, mean=form == "mean", argpos=argpos)
    sc.assert_within(a, cpu.double().numpy(), bar, f"GPU vs CPU entry point, {form}", factor=2.0)


def test_graph_capture(hub):
    """pg_sddmm_dot allocates nothing and does not synchronise: captured in a HIP graph, its
    replays equal the eager result bitwise."""
    from plagnn import ops

    F = 64
    D, X = _operands(hub, F, seed=9)
    Dt, Xt = sc.to_dev(D, DEV), sc.to_dev(X, DEV)
    dg = hub.on(DEV)
    argpos = ops.spmm_max(dg, Xt)[1]
    eager = ops.sddmm_dot(dg, Dt, Xt), ops.sddmm_dot(dg, Dt, Xt, argpos=argpos)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.sddmm_dot(dg, Dt, Xt), ops.sddmm_dot(dg, Dt, Xt, argpos=argpos)
    for _ in range(2):
        for c in cap:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1])


def test_error_returns(hub):
    from plagnn import _lib
    from plagnn._lib import ptr

    s = hub.on(DEV).fwd.struct(None)
    n, F = hub.num_nodes, 8
    D, X = torch.zeros(n, F, device=DEV), torch.zeros(n, F, device=DEV)
    de = torch.zeros(hub.num_edges, device=DEV)
    with pytest.raises(_lib.PlagnnError, match="norm_mode"):
        _lib.call("pg_sddmm_dot", s, ptr(D), F, ptr(X), F, F, 2, None, 0, _lib.PG_ARG_U16, ptr(de), None)
    with pytest.raises(_lib.PlagnnError, match="leading"):
        _lib.call("pg_sddmm_dot", s, ptr(D), F - 1, ptr(X), F, F, 0, None, 0, _lib.PG_ARG_U16, ptr(de), None)
    a = torch.zeros(n, F, dtype=torch.int16, device=DEV)
    with pytest.raises(_lib.PlagnnError, match="arg_kind"):
        _lib.call("pg_sddmm_dot", s, ptr(D), F, ptr(X), F, F, 0, ptr(a), F, 7, ptr(de), None)


# ------------------------------------------------------------------ autograd and the shim
@pytest.mark.parametrize("kind", ["sum", "mean", "max"])
def test_aggregate_ops_edge_weight_grad(kind, monkeypatch):
    sc.check_aggregate_ops(DEV, kind, monkeypatch, n=500, hub=700, F=40)


@pytest.mark.parametrize("reduce_op", ["sum", "mean", "max"])
def test_update_all_u_mul_e_edge_weight_grad(reduce_op, monkeypatch):
    sc.check_update_all(DEV, reduce_op, monkeypatch, n=500, hub=700, F=40)


# in_feats 40: the two-piece product path (no padding); 37: the padded path
@pytest.mark.parametrize("zero_w", [False, True], ids=["positive_w", "zero_w"])
@pytest.mark.parametrize("fin,fout", [(40, 16), (37, 16), (16, 40)])
def test_sage_pool_edge_weight_grad(fin, fout, zero_w, monkeypatch):
    sc.check_sage_pool(DEV, fin, fout, monkeypatch, n=500, hub=700, zero_w=zero_w)


@pytest.mark.parametrize("fin", [40, 37])
def test_sage_pool_frozen_weight_keeps_dead_none_records(fin, monkeypatch):
    sc.check_sage_pool_frozen_weight_unchanged(DEV, fin, monkeypatch, n=500, hub=700)


@pytest.mark.parametrize("fin,fout", [(40, 16), (16, 40)], ids=["lin_before_mp", "lin_after_mp"])
def test_sage_mean_edge_weight_grad(fin, fout):
    sc.check_sage_mean(DEV, fin, fout, n=500, hub=700)


@pytest.mark.parametrize("fin,fout", [(40, 16), (16, 40)], ids=["w_first", "aggregate_first"])
def test_graphconv_edge_weight_grad(fin, fout):
    sc.check_graphconv(DEV, fin, fout, n=500, hub=700)


def test_apply_edges_u_dot_v():
    sc.check_u_dot_v(DEV)
