"""Multi-head attention on the GPU: the kernels behind pg_edge_softmax_fwd / _bwd,
pg_spmm_sum_heads and pg_sddmm_dot_heads against the float64 references and derived bars of
tests/gat_common.py (every path: power-of-two and generic H, vector and scalar feature paths,
a head that straddles the 256-column tile, whole rows and split rows, both CSR directions),
agreement with the _cpu entry points within twice the bars, bitwise-equal repeated calls, and
the shim checks of test_gat_cpu.py on the device."""
import pytest
import torch

import gat_common as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = [1, 2, 3, 4, 8]


@pytest.mark.parametrize("sigma", [1.0, 10.0])
@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_edge_softmax_forward(gname, H, sigma):
    gc.check_softmax_fwd(DEV, gname, H, sigma)


@pytest.mark.parametrize("H", [3, 4])
def test_edge_softmax_forward_shifted_scores(H):
    gc.check_softmax_shift(DEV, "hub", H)


@pytest.mark.parametrize("H", [3, 4])
def test_edge_softmax_forward_neg_inf_scores(H):
    gc.check_softmax_neg_inf(DEV, H)


def test_edge_softmax_64_heads():
    """H = 64: one lane per head, no cross-lane step; rows longer than the register path."""
    gc.check_softmax_fwd(DEV, "hub", 64, 1.0)
    gc.check_softmax_bwd(DEV, "hub", 64)


@pytest.mark.parametrize("H", [3, 4])
def test_edge_softmax_long_row_on_one_wave(H):
    """CSRGraph(chunk=1024): the 300-entry hub row is not split, so one wave takes it and
    re-reads its scores between the passes (more than 4 values per lane for either H)."""
    gc.check_softmax_fwd(DEV, "hub_whole", H, 1.0)
    gc.check_softmax_bwd(DEV, "hub_whole", H)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_edge_softmax_backward(gname, H):
    gc.check_softmax_bwd(DEV, gname, H)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "transposed"])
@pytest.mark.parametrize("H,Fh", gc.SHAPES)
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_spmm_sum_heads(gname, H, Fh, transpose):
    gc.check_sum_heads(DEV, gname, H, Fh, transpose)


@pytest.mark.parametrize("H,Fh", gc.SHAPES + [(2, 256), (16, 4), (2, 512)])
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_sddmm_dot_heads(gname, H, Fh):
    gc.check_sddmm_heads(DEV, gname, H, Fh)


def test_padded_edge_tensors():
    """Edge tensors with a leading dimension of H + 3."""
    gc.check_softmax_fwd(DEV, "hub", 4, 1.0, pad=3)
    gc.check_softmax_bwd(DEV, "hub", 4, pad=3)
    gc.check_sum_heads(DEV, "hub", 4, 64, False, pad=3)
    gc.check_sum_heads(DEV, "hub", 4, 64, True, pad=3)
    gc.check_sddmm_heads(DEV, "hub", 4, 64, pad=3)


@pytest.mark.parametrize("H,Fh", [(4, 64), (3, 5), (4, 96)])
@pytest.mark.parametrize("gname", ["hub", "hub64"])
def test_matches_cpu_entry_points_and_repeats_bitwise(gname, H, Fh):
    """GPU vs _cpu within twice the bars; two calls on the same inputs are torch.equal."""
    g = gc.graph(gname)
    s = gc.scores(g, H, 1.0)
    a, _, bar = gc.run_softmax_fwd(DEV, g, s, "softmax fwd")
    a2, _, _ = gc.run_softmax_fwd(DEV, g, s, "softmax fwd")
    assert torch.equal(a, a2), "edge softmax: two calls differ"
    a_cpu, _, _ = gc.run_softmax_fwd("cpu", g, s, "softmax fwd (cpu)")
    gc.within(a, a_cpu.double().numpy(), bar, "softmax fwd GPU vs CPU", factor=2.0)

    av, da = gc.softmax_bwd_case(g, H)
    d1, _, bar = gc.run_softmax_bwd(DEV, g, av, da, "softmax bwd")
    d2, _, _ = gc.run_softmax_bwd(DEV, g, av, da, "softmax bwd")
    assert torch.equal(d1, d2), "edge softmax backward: two calls differ"
    d_cpu, _, _ = gc.run_softmax_bwd("cpu", g, av, da, "softmax bwd (cpu)")
    gc.within(d1, d_cpu.double().numpy(), bar, "softmax bwd GPU vs CPU", factor=2.0)

    A, X, D = gc.heads_case(g, H, Fh)
    for tr in (False, True):
        o1, _, bar = gc.run_sum_heads(DEV, g, A, X, H, tr, f"sum_heads T={tr}")
        o2, _, _ = gc.run_sum_heads(DEV, g, A, X, H, tr, f"sum_heads T={tr}")
        assert torch.equal(o1, o2), "spmm_sum_heads: two calls differ"
        o_cpu, _, _ = gc.run_sum_heads("cpu", g, A, X, H, tr, f"sum_heads T={tr} (cpu)")
        gc.within(o1, o_cpu.double().numpy(), bar, "sum_heads GPU vs CPU", factor=2.0)

    e1, _, bar = gc.run_sddmm_heads(DEV, g, D, X, H, "sddmm_heads")
    e2, _, _ = gc.run_sddmm_heads(DEV, g, D, X, H, "sddmm_heads")
    assert torch.equal(e1, e2), "sddmm_dot_heads: two calls differ"
    e_cpu, _, _ = gc.run_sddmm_heads("cpu", g, D, X, H, "sddmm_heads (cpu)")
    gc.within(e1, e_cpu.double().numpy(), bar, "sddmm_heads GPU vs CPU", factor=2.0)


def test_graph_capture():
    """The four entry points allocate nothing and do not synchronise: captured in a HIP graph,
    their replays equal the eager results bitwise."""
    from plagnn import ops
    import sddmm_common as sc

    g = gc.graph("hub")
    dg = g.on(DEV)
    H, Fh = 4, 64
    A, X, D = (sc.to_dev(t, DEV) for t in gc.heads_case(g, H, Fh))
    s = sc.to_dev(gc.scores(g, H, 1.0), DEV)

    def run():
        a = ops.edge_softmax(dg, s)
        return (a, ops.edge_softmax_backward(dg, a, A), ops.spmm_sum_heads(dg, a, X, H),
                ops.spmm_sum_heads(dg, a, X, H, transpose=True), ops.sddmm_dot_heads(dg, D, X, H))

    eager = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    for _ in range(2):
        for c in cap:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for c, e in zip(cap, eager):
            assert torch.equal(c, e)


def test_empty_shapes():
    gc.check_empty_shapes(DEV)
    torch.cuda.synchronize()


def test_rejections():
    gc.check_rejections(DEV)


# ------------------------------------------------------------------ autograd and the shim
def test_shim_edge_softmax():
    gc.check_shim_edge_softmax(DEV)


@pytest.mark.parametrize("H,Fh", [(4, 8), (3, 5), (4, 64)])
def test_shim_update_all_multi_head(H, Fh):
    gc.check_shim_update_all_heads(DEV, H, Fh)


@pytest.mark.parametrize("shape", [(4, 1), (3,), (70,)], ids=["heads", "flat", "wide"])
def test_shim_apply_edges_u_add_v(shape):
    """Values, both gradients, and the gradients of two runs are bitwise equal."""
    gc.check_shim_u_add_v(DEV, shape, twice=True)


def test_shim_apply_edges_u_dot_v_multi_head():
    gc.check_shim_u_dot_v_heads(DEV)


@pytest.mark.parametrize("fin,fout,H,residual", [(20, 8, 4, False), (12, 16, 1, True)])
def test_gatconv(fin, fout, H, residual):
    gc.check_gatconv(DEV, fin, fout, H, residual)


def test_gatconv_identity_residual():
    gc.check_gatconv(DEV, 16, 8, 2, True)


def test_gatconv_zero_in_degree():
    gc.check_gatconv_zero_in_degree(DEV)
    gc.check_gatconv(DEV, 20, 8, 4, False, self_loop=False)


def test_shim_rejections():
    gc.check_shim_rejections(DEV)


def test_one_weight_per_edge_still_issues_spmm_sum(monkeypatch):
    gc.check_one_weight_per_edge_unchanged(DEV, monkeypatch)
