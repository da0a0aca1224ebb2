"""pg_spmm_sum on the GPU (sum / mean / edge-weighted aggregation and its transposed mean
form, behind GraphConv, SAGEConv('mean' | 'gcn'), update_all(copy_u | u_mul_e, sum | mean) and
their backwards): every width path, split rows, strides and guards within the float64 bar of
tests/sum_common.py and bitwise against the schedule's own float32 order
(sum_piecewise32 with split=True), repeatability, HIP-graph capture, the C-ABI's error
returns and agreement with the CPU entry point on unsplit rows."""
import numpy as np
import pytest
import torch

import sddmm_common as sc
import sum_common as su
from conftest import hub_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_width_list_straddles_the_tile_boundaries():
    su.check_width_list()


@pytest.mark.parametrize("F,form", su.WIDTH_CASES)
def test_width_sweep(F, form):
    su.check_width(DEV, F, form)


@pytest.mark.parametrize("chunk_bwd", [4, None], ids=["chunk4", "default_chunk"])
@pytest.mark.parametrize("weighted", [False, True], ids=["copy_u", "u_mul_e"])
@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("F", su.TRANSPOSED_WIDTHS)
def test_transposed_forms(F, mean, weighted, chunk_bwd):
    su.check_transposed(DEV, F, mean, weighted, chunk_bwd)


@pytest.mark.parametrize("chunk", [4, 64])
@pytest.mark.parametrize("F", [3, 40, 260])
def test_tiny_and_exact_items(F, chunk):
    su.check_item_lengths(DEV, chunk, F)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("F", [40, 260, 1100])
def test_unaligned_operands_give_the_same_bits(F, transpose):
    su.check_unaligned(DEV, F, transpose)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("off", [4, 1])
@pytest.mark.parametrize("F", [5, 64, 260])
def test_strided_views_with_guards(F, off, transpose):
    su.check_strided_guards(DEV, F, off, transpose)


@pytest.mark.parametrize("F", [3, 260])
def test_rectangular_graph(F):
    su.check_rect(DEV, F)


def test_empty_shapes():
    su.check_empty_shapes(DEV)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("F", [64, 65])
def test_nonfinite_inputs(F, transpose):
    su.check_nonfinite(DEV, F, transpose)


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("F", [260, 503])
def test_autograd_at_width(F, mean):
    su.check_autograd(DEV, F, mean)


def test_error_returns():
    su.check_error_returns(DEV)


def test_graph_capture():
    """pg_spmm_sum allocates nothing and does not synchronise: a forward call and a transposed
    mean call on a graph with split rows, captured one after the other on one stream, replay
    to the eager results bitwise."""
    from plagnn import ops

    F = 260
    g = su.ladder_graph()
    assert g.fwd.n_merges > 0 and g.bwd.n_merges > 0
    dg = g.on(DEV)
    X, w = su.operands(g.fwd, F, seed=8)
    Xt, wt = sc.to_dev(X, DEV), sc.to_dev(w, DEV)

    def both():
        return (ops.spmm_sum(dg, Xt, mean=True, ew_slots=wt),
                ops.spmm_sum(dg, Xt, mean=True, ew_slots=wt, transpose=True))

    eager = both()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = both()
    for _ in range(2):
        for c in cap:
            c.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        su.assert_bits(cap[0], eager[0], "replayed forward")
        su.assert_bits(cap[1], eager[1], "replayed transposed mean")


@pytest.mark.parametrize("form", ["plain", "weighted_mean"])
def test_unsplit_rows_match_the_cpu_entry_point(form):
    """On rows the schedule does not split the kernel's order is pg_spmm_sum_cpu's: the same
    bits, in both directions."""
    import plagnn
    from plagnn import ops

    F = 260
    mean, weighted = su.FORMS[form]
    src, dst = hub_graph(500, 700)
    g = plagnn.CSRGraph(src, dst, 500)
    for transpose in (False, True):
        csr = g.bwd if transpose else g.fwd
        split = np.zeros(csr.n_rows, bool)
        split[csr.merges.reshape(-1, 4)[:csr.n_merges, 0]] = True
        assert split.any() and not split.all()
        X, w = su.operands(csr, F, seed=9)
        w = w if weighted else None
        res = []
        for dev in (DEV, "cpu"):
            wt = None if w is None else sc.to_dev(w, dev)
            res.append(ops.spmm_sum(g.on(dev), sc.to_dev(X, dev), mean=mean, ew_slots=wt, transpose=transpose).cpu())
        su.assert_bits(res[0][~split], res[1][~split], f"{form} transpose={transpose}: unsplit rows, GPU vs CPU")
        ref, bar = su.sum_ref64(csr, X, w, (2 if transpose else 1) if mean else 0, g.fwd.ptr)
        sc.assert_within(res[0], ref, bar, f"{form} transpose={transpose}: all rows")
