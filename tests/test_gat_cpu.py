"""Multi-head attention on the CPU device: the four _cpu entry points (pg_edge_softmax_fwd /
_bwd, pg_spmm_sum_heads, pg_sddmm_dot_heads) against float64 references within the derived
bars of tests/gat_common.py, and the shim built on them (edge_softmax, apply_edges(u_add_v),
multi-head u_dot_v and u_mul_e, GATConv) against float64 torch compositions on the edge
list."""
import pytest

import gat_common as gc

DEV = "cpu"
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


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_edge_softmax_backward(gname, H):
    gc.check_softmax_bwd(DEV, gname, H)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "transposed"])
@pytest.mark.parametrize("H,Fh", gc.SHAPES)
@pytest.mark.parametrize("gname", gc.GRAPHS)
def test_spmm_sum_heads(gname, H, Fh, transpose):
    gc.check_sum_heads(DEV, gname, H, Fh, transpose)


@pytest.mark.parametrize("H,Fh", gc.SHAPES)
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


def test_empty_shapes():
    gc.check_empty_shapes(DEV)


def test_rejections():
    gc.check_rejections(DEV)


# ------------------------------------------------------------------ autograd and the shim
def test_shim_edge_softmax():
    gc.check_shim_edge_softmax(DEV)


@pytest.mark.parametrize("H,Fh", [(4, 8), (3, 5)])
def test_shim_update_all_multi_head(H, Fh):
    gc.check_shim_update_all_heads(DEV, H, Fh)


@pytest.mark.parametrize("shape", [(4, 1), (3,), (70,)], ids=["heads", "flat", "wide"])
def test_shim_apply_edges_u_add_v(shape):
    gc.check_shim_u_add_v(DEV, shape)


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


def test_gatconv_is_exported():
    import dgl.nn
    import dgl.nn.pytorch as dnp

    assert "GATConv" in dnp.__all__ and dgl.nn.GATConv is dnp.GATConv
