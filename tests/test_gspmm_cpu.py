"""pg_gspmm_cpu / pg_gsddmm_cpu (vector edge features on the CPU device) against the float64
references of tests/gspmm_common.py, and the shim built on them: dgl.function's binary
builtins, copy_e and min in update_all / apply_edges, dgl.ops.gspmm / gsddmm and EdgeConv,
with their gradients. No GPU needed."""
import pytest

import gspmm_common as gs

DEV = "cpu"


@pytest.mark.parametrize("reduce", gs.REDUCERS + ["mean"])
@pytest.mark.parametrize("op", gs.OPS)
def test_gspmm_every_op_and_reducer(op, reduce):
    gs.check_gspmm(DEV, "hub", op, reduce, 12, "grid")
    gs.check_gspmm(DEV, "hub", op, reduce, 12, "gauss")


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "transposed"])
@pytest.mark.parametrize("F", gs.WIDTHS)
@pytest.mark.parametrize("op,reduce", gs.TRIO)
@pytest.mark.parametrize("gname", gs.GRAPHS)
def test_gspmm_graphs_and_widths(gname, op, reduce, F, transpose):
    gs.check_gspmm(DEV, gname, op, reduce, F, "grid", transpose=transpose)
    gs.check_gspmm(DEV, gname, op, reduce, F, "gauss", transpose=transpose)


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("op,reduce", gs.TRIO)
def test_gspmm_leading_dimensions(op, reduce, pad):
    gs.check_gspmm(DEV, "hub64", op, reduce, 8, "grid", pad=pad)
    gs.check_gspmm(DEV, "hub", op, reduce, 300, "gauss", pad=pad)


@pytest.mark.parametrize("eidx", [None, "perm"], ids=["slot_order", "permutation"])
@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "transposed"])
def test_gspmm_edge_index(transpose, eidx):
    for op, reduce in gs.TRIO:
        gs.check_gspmm(DEV, "hub64", op, reduce, 8, "grid", transpose=transpose, eidx=eidx)


def test_gspmm_i32_records():
    _, rec = gs.check_gspmm(DEV, "hub", "add", "max", 8, "grid", kind=32)
    assert rec is not None
    gs.check_gspmm(DEV, "hub", "copy_rhs", "min", 5, "grid", kind=32, pad=3)


def test_gspmm_inf_is_stored_as_zero():
    gs.check_inf_edge(DEV)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("lt,rt", gs.TARGET_PAIRS)
@pytest.mark.parametrize("op", gs.OPS)
def test_gsddmm_every_op_and_target_pair(op, lt, rt, masked):
    gs.check_gsddmm(DEV, "hub", op, lt, rt, 12, "grid", masked=masked)
    gs.check_gsddmm(DEV, "hub", op, lt, rt, 12, "gauss", masked=masked)


@pytest.mark.parametrize("F", gs.WIDTHS)
@pytest.mark.parametrize("gname", gs.GRAPHS)
def test_gsddmm_graphs_and_widths(gname, F):
    gs.check_gsddmm(DEV, gname, "sub", "u", "v", F, "grid")
    gs.check_gsddmm(DEV, gname, "copy_lhs", "v", "e", F, "grid", masked=True)
    gs.check_gsddmm(DEV, gname, "mul", "e", "u", F, "gauss")


@pytest.mark.parametrize("pad", [3, 4])
def test_gsddmm_leading_dimensions_and_edge_index(pad):
    gs.check_gsddmm(DEV, "hub64", "div", "v", "e", 8, "grid", pad=pad, eidx="perm")
    gs.check_gsddmm(DEV, "hub", "copy_lhs", "v", "e", 300, "grid", masked=True, pad=pad, kind=32)
    gs.check_gsddmm(DEV, "hub", "mul", "u", "v", 8, "gauss", masked=True, pad=pad, eidx=None)


def test_empty_shapes():
    gs.check_empty_shapes(DEV)


def test_abi_rejections():
    gs.check_abi_rejections(DEV)


def test_version_and_exports():
    gs.check_exports()


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("op", gs.BINARY)
def test_update_all_u_op_e(op, reduce):
    gs.check_update_all(DEV, f"u_{op}_e", reduce)


@pytest.mark.parametrize("msg,reduce", [("e_sub_u", "sum"), ("e_sub_u", "max"), ("e_div_u", "sum"), ("e_div_u", "min"),
                                        ("copy_e", "sum"), ("copy_e", "max"), ("copy_e", "min"), ("copy_u", "min")])
def test_update_all_other_messages(msg, reduce):
    gs.check_update_all(DEV, msg, reduce, shape=(2, 4))


@pytest.mark.parametrize("msg", ["u_sub_v", "v_sub_u", "u_mul_v", "u_div_v", "e_add_v", "u_dot_e"])
def test_apply_edges(msg):
    gs.check_apply_edges(DEV, msg)


def test_dgl_ops():
    gs.check_dgl_ops(DEV)


@pytest.mark.parametrize("batch_norm", [False, True])
def test_edgeconv(batch_norm):
    gs.check_edgeconv(DEV, batch_norm)


def test_tie_gradient_goes_to_the_first_winner():
    gs.check_tie_gradient(DEV)


def test_shim_rejections():
    gs.check_shim_rejections(DEV)


def test_scalar_forms_keep_their_entry_points(monkeypatch):
    gs.check_scalar_forms_unchanged(DEV, monkeypatch)
