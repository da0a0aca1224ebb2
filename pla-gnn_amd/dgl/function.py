"""dgl.function builtins understood by DGLGraph.update_all (the forms SAGEConv uses:
copy_u('h', 'm') / u_mul_e('h', '_edge_weight', 'm') with sum / mean / max) and by
DGLGraph.apply_edges (u_dot_v('a', 'b', 'out'), DGL's SDDMM, and u_add_v('a', 'b', 'out'),
GATConv's attention logits). With vector edge features (pg_gspmm / pg_gsddmm): every binary
builtin {u,v,e}_{add,sub,mul,div,dot}_{u,v,e} with two different targets, copy_e and the min
reducer."""
from __future__ import annotations


class _Message:
    def __init__(self, op: str, lhs: str, rhs, out: str):
        self.op, self.lhs, self.rhs, self.out = op, lhs, rhs, out


class _Reduce:
    def __init__(self, op: str, msg: str, out: str):
        self.op, self.msg, self.out = op, msg, out


def copy_u(u: str, out: str) -> _Message:
    return _Message("copy_u", u, None, out)


copy_src = copy_u  # DGL < 0.8 name


def u_mul_e(lhs_field: str, rhs_field: str, out: str) -> _Message:
    return _Message("u_mul_e", lhs_field, rhs_field, out)


def u_dot_v(lhs_field: str, rhs_field: str, out: str) -> _Message:
    """out[e] = <ndata[lhs][src_e], ndata[rhs][dst_e]>, shape (E, 1) (apply_edges only)."""
    return _Message("u_dot_v", lhs_field, rhs_field, out)


def u_add_v(lhs_field: str, rhs_field: str, out: str) -> _Message:
    """out[e] = ndata[lhs][src_e] + ndata[rhs][dst_e], any trailing shape (apply_edges only)."""
    return _Message("u_add_v", lhs_field, rhs_field, out)


def copy_e(e: str, out: str) -> _Message:
    """out[e] = edata[e] (update_all: the message is the edge feature itself)."""
    return _Message("copy_e", e, None, out)


copy_edge = copy_e  # DGL < 0.8 name


def _binary(name: str):
    def fn(lhs_field: str, rhs_field: str, out: str) -> _Message:
        return _Message(name, lhs_field, rhs_field, out)

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = (f"out = {name.split('_')[1]}(lhs at '{name[0]}', rhs at '{name[-1]}') per edge, as DGL "
                  "generates it: u = source node, v = destination node, e = edge.")
    return fn


# every {u,v,e}_{add,sub,mul,div,dot}_{u,v,e} with two different targets; the four documented
# above keep their definitions
for _l in "uve":
    for _r in "uve":
        for _o in ("add", "sub", "mul", "div", "dot"):
            _n = f"{_l}_{_o}_{_r}"
            if _l != _r and _n not in globals():
                globals()[_n] = _binary(_n)
del _l, _r, _o, _n


def sum(msg: str, out: str) -> _Reduce:  # noqa: A001  (DGL's name)
    return _Reduce("sum", msg, out)


def mean(msg: str, out: str) -> _Reduce:
    return _Reduce("mean", msg, out)


def max(msg: str, out: str) -> _Reduce:  # noqa: A001  (DGL's name)
    return _Reduce("max", msg, out)


def min(msg: str, out: str) -> _Reduce:  # noqa: A001  (DGL's name)
    return _Reduce("min", msg, out)
