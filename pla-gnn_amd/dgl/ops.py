"""dgl.ops: edge_softmax (DGL 0.8.2's ``dgl.ops.edge_softmax`` /
``dgl.nn.functional.edge_softmax``) on the engine's pg_edge_softmax_fwd / _bwd, and DGL's two
message-passing primitives gspmm / gsddmm with the names DGL generates on top of them
(u_mul_e_sum, copy_e_max, u_sub_v, ...) on pg_gspmm / pg_gsddmm."""
from __future__ import annotations

import torch

ALL = "__ALL__"  # dgl.base.ALL


def _is_all(eids) -> bool:
    return isinstance(eids, str) and eids == ALL


def edge_softmax(graph, logits, eids=ALL, norm_by="dst"):
    """Softmax of ``logits`` ((E, *) in edge-id order) over the in-edges of each destination
    node, independently for every trailing index (at most 64 of them per edge). The result
    has the shape and dtype of ``logits`` and is differentiable. ``norm_by='src'`` and a
    subset of ``eids`` are not supported."""
    import dgl
    from plagnn import ops

    if not isinstance(graph, dgl.DGLGraph):
        raise TypeError("expected a dgl.DGLGraph built by this package")
    if norm_by != "dst":
        raise NotImplementedError("edge_softmax: only norm_by='dst' is supported")
    if not _is_all(eids):
        raise NotImplementedError("edge_softmax on a subset of the edges is not supported")
    E = graph.num_edges()
    if logits.dim() < 1 or logits.shape[0] != E:
        raise ValueError(f"edge_softmax: logits {tuple(logits.shape)} on a graph of {E} edges")
    dg = graph._device_graph(logits.device)
    s = logits.reshape(E, -1).float().index_select(0, dg.eid)  # edge-id order -> slot order
    a = ops.EdgeSoftmax.apply(s, dg)
    # slot order -> edge-id order: eid is a permutation, so every element is written once
    out = torch.empty_like(a).index_copy(0, dg.eid, a)
    return out.to(logits.dtype).reshape(logits.shape)


_BINARY = ("add", "sub", "mul", "div")


def _graph_and_ops(graph):
    import dgl
    from plagnn import ops

    if not isinstance(graph, dgl.DGLGraph):
        raise TypeError("expected a dgl.DGLGraph built by this package")
    return ops


def _flat(t):
    return None if t is None else t.reshape(t.shape[0], -1).float()


def _pair(name, op, lhs_data, rhs_data):
    """The operands `op` reads, of equal trailing shapes (broadcasting is not supported)."""
    if op == "copy_lhs":
        rhs_data = None
    if op == "copy_rhs":
        lhs_data = None
    if (lhs_data is None and op != "copy_rhs") or (rhs_data is None and op != "copy_lhs"):
        raise ValueError(f"{name}: operator {op!r} needs both operands")
    if lhs_data is not None and rhs_data is not None and lhs_data.shape[1:] != rhs_data.shape[1:]:
        raise NotImplementedError(f"{name}: operands of equal trailing shapes are supported, not "
                                  f"{tuple(lhs_data.shape[1:])} with {tuple(rhs_data.shape[1:])}")
    return lhs_data, rhs_data


def gspmm(g, op, reduce_op, lhs_data, rhs_data):
    """dgl.ops.gspmm: out[v] = reduce_op over the in-edges e = (u -> v) of op(lhs_data[u],
    rhs_data[e]); op in 'add', 'sub', 'mul', 'div', 'copy_lhs', 'copy_rhs', reduce_op in 'sum',
    'mean', 'max', 'min'; lhs_data are node features (N, *), rhs_data edge features (E, *) in
    edge-id order, of equal trailing shapes (pg_gspmm; differentiable in both). 'div' is a true
    division: DGL multiplies by the reciprocal of rhs_data, which rounds twice. Nodes without
    in-edges get 0."""
    ops = _graph_and_ops(g)
    if op not in _BINARY + ("copy_lhs", "copy_rhs") or reduce_op not in ("sum", "mean", "max", "min"):
        raise ValueError(f"gspmm: unknown operator {op!r} or reducer {reduce_op!r}")
    lhs_data, rhs_data = _pair("gspmm", op, lhs_data, rhs_data)
    ref = lhs_data if lhs_data is not None else rhs_data
    out = ops.GSpMM.apply(g._device_graph(ref.device), op, reduce_op, _flat(lhs_data), _flat(rhs_data), "u", "e")
    return out.to(ref.dtype).reshape((g.num_nodes(),) + tuple(ref.shape[1:]))


def gsddmm(g, op, lhs_data, rhs_data, lhs_target="u", rhs_target="v"):
    """dgl.ops.gsddmm: out[e] = op(lhs_data[t_l(e)], rhs_data[t_r(e)]) for every edge, in edge-id
    order; targets 'u' (source), 'v' (destination), 'e' (edge), two different ones; op in 'add',
    'sub', 'mul', 'div', 'dot', 'copy_lhs', 'copy_rhs' on operands of equal trailing shapes
    (pg_gsddmm; differentiable in both). 'dot' sums the product over the last dimension
    (keepdim); 'div' is a true division where DGL multiplies by a reciprocal."""
    ops = _graph_and_ops(g)
    if op not in _BINARY + ("dot", "copy_lhs", "copy_rhs"):
        raise ValueError(f"gsddmm: unknown operator {op!r}")
    for t in (lhs_target, rhs_target):
        if t not in ("u", "v", "e"):
            raise ValueError(f"gsddmm: unknown target {t!r}")
    kop = "mul" if op == "dot" else op
    lhs_data, rhs_data = _pair("gsddmm", kop, lhs_data, rhs_data)
    ref = lhs_data if lhs_data is not None else rhs_data
    out = ops.GSDDMM.apply(g._device_graph(ref.device), kop, _flat(lhs_data), _flat(rhs_data), lhs_target,
                           rhs_target)
    out = out.to(ref.dtype).reshape((g.num_edges(),) + tuple(ref.shape[1:]))
    return out.sum(-1, keepdim=True) if op == "dot" and out.dim() > 1 else out


def _gen_spmm(lhs, op, rhs, reduce_op):
    name = f"{lhs}_{op}_{rhs}_{reduce_op}"

    def fn(g, x, y):
        # e_<op>_u: the edge operand comes first; the kernel takes (node, edge) targets either way
        ops = _graph_and_ops(g)
        x, y = _pair(name, op, x, y)
        node = x if lhs == "u" else y
        out = ops.GSpMM.apply(g._device_graph(node.device), op, reduce_op, _flat(x), _flat(y), lhs, rhs)
        return out.to(node.dtype).reshape((g.num_nodes(),) + tuple(node.shape[1:]))

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"out[v] = {reduce_op} over the in-edges of {op}(x at '{lhs}', y at '{rhs}') (dgl.ops.{name})."
    return fn


def _gen_copy_spmm(target, reduce_op):
    name = f"copy_{target}_{reduce_op}"

    def fn(g, x):
        return gspmm(g, "copy_lhs", reduce_op, x, None) if target == "u" else gspmm(g, "copy_rhs", reduce_op, None, x)

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"out[v] = {reduce_op} over the in-edges of x at '{target}' (dgl.ops.{name})."
    return fn


def _gen_sddmm(lhs, op, rhs):
    name = f"{lhs}_{op}_{rhs}"

    def fn(g, x, y):
        return gsddmm(g, op, x, y, lhs, rhs)

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"out[e] = {op}(x at '{lhs}', y at '{rhs}') per edge (dgl.ops.{name})."
    return fn


__all__ = ["edge_softmax", "gspmm", "gsddmm"]
for _r in ("sum", "mean", "max", "min"):
    for _o in _BINARY:
        for _l, _t in (("u", "e"), ("e", "u")):
            globals()[f"{_l}_{_o}_{_t}_{_r}"] = _gen_spmm(_l, _o, _t, _r)
            __all__.append(f"{_l}_{_o}_{_t}_{_r}")
    for _t in ("u", "e"):
        globals()[f"copy_{_t}_{_r}"] = _gen_copy_spmm(_t, _r)
        __all__.append(f"copy_{_t}_{_r}")
for _l in "uve":
    for _t in "uve":
        if _l != _t:
            for _o in _BINARY + ("dot",):
                globals()[f"{_l}_{_o}_{_t}"] = _gen_sddmm(_l, _o, _t)
                __all__.append(f"{_l}_{_o}_{_t}")
del _r, _o, _l, _t
