"""Drop-in subset of the DGL 0.8.2 Python API that quinlanW/PLA-GNN uses, backed by the
MI355X message-passing engine (``plagnn``).

The reference touches exactly this surface:
  import dgl                                         code/utils.py:4, main_normal.py:9-15
  dgl.graph((start, end), num_nodes=N)               code/utils.py:44
  dgl.add_self_loop(g)                               code/utils.py:45
  g.nodes[list(range(N))].data[key] = tensor         code/utils.py:46, 49
  g.ndata['feat'], g.ndata['loc']                    code/train.py:145-146, 179
  g.to(device)                                       code/main_normal.py:66
  dgl.seed(seed)                                     code/main_normal.py:15
  from dgl.nn.pytorch import SAGEConv                code/model.py:7
  SAGEConv(in, out, 'pool')(g, h)                    code/model.py:13-15, 20-24
plus ``update_all`` with ``dgl.function`` builtins (copy_u / u_mul_e with sum / mean /
max), which SAGEConv itself is defined by, and ``apply_edges`` with ``u_dot_v`` (DGL's
SDDMM). Edge weights may require grad: every weighted aggregation is differentiable with
respect to them, as DGL's GSpMM.backward is. Multi-head attention (reference-unpinned):
``apply_edges(u_add_v)``, ``dgl.ops.edge_softmax`` / ``dgl.nn.functional.edge_softmax``,
``u_dot_v`` and ``update_all(u_mul_e, sum)`` on (N, H, Fh) features with (E, H, 1) edge
features, ``dgl.nn.pytorch.GATConv`` built on them, and ``dgl.nn.pytorch.GATv2Conv`` on a
fused score kernel of its own (pg_gatv2_score). Vector edge features
(reference-unpinned): every binary builtin ``{u,v,e}_{add,sub,mul,div,dot}_{u,v,e}``, ``copy_e``
and the ``min`` reducer on node and edge features of equal trailing shapes, ``dgl.ops.gspmm`` /
``gsddmm`` and ``dgl.nn.pytorch.EdgeConv`` (pg_gspmm, pg_gsddmm).
Mini-batch training (reference-unpinned): ``DGLBlock`` with separate ``srcdata`` / ``dstdata``,
``dgl.create_block``, ``dgl.to_block`` (pg_block_compact), ``dgl.sampling.sample_neighbors``
(pg_sample_count, pg_sample_fill), ``dgl.dataloading``'s neighbour samplers and DataLoader, and
blocks or (feat_src, feat_dst) pairs in the layers of ``dgl.nn.pytorch``.
Link prediction (reference-unpinned): ``g.find_edges`` / ``has_edges_between`` / ``edge_ids``
(pg_edge_lookup), ``exclude_edges`` / ``exclude_eids`` in the samplers (pg_edge_bits_update,
pg_sample_count_excl, pg_sample_fill_excl), ``dgl.dataloading.negative_sampler`` and
``dgl.sampling.global_uniform_negative_sampling`` (pg_negative_sample),
``dgl.dataloading.as_edge_prediction_sampler`` and ``EdgeDataLoader``.

Message passing on a CUDA (HIP) device always runs in libplagnn.so; a missing library is
an error, never a silent fallback.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import numpy as np
import torch

from . import function  # noqa: F401  (dgl.function)
from . import ops  # noqa: F401  (dgl.ops)
from . import nn  # noqa: F401  (dgl.nn)

__version__ = "0.8.2+plagnn"

_SEED: Optional[int] = None
_SAMPLE_CALLS = 0
_BINARY_OPS = ("add", "sub", "mul", "div")
NID = "_ID"  # dgl.NID: parent node ids of a block's / subgraph's nodes
EID = "_ID"  # dgl.EID: parent edge ids of its edges


class DGLError(Exception):
    """dgl.DGLError (dgl.base.DGLError): what DGL raises for a bad argument of a graph query."""


def seed(val: int) -> None:
    """dgl.seed: DGL seeds its own C RNG, the one its samplers draw from. Here it starts the
    sampler's counter: every dgl.sampling.sample_neighbors call (one per layer of a
    NeighborSampler) takes the next 64-bit value of a sequence fixed by `val`, so the same
    seed gives the same blocks. Nothing on the full-graph training path draws from it."""
    global _SEED, _SAMPLE_CALLS
    _SEED = int(val)
    _SAMPLE_CALLS = 0


def _next_sample_seed() -> int:
    """The 64-bit seed of the next sampling call: a counter advanced per call, offset by
    dgl.seed's value (the kernel's key function mixes it, so consecutive values are fine)."""
    global _SAMPLE_CALLS
    _SAMPLE_CALLS += 1
    return ((_SEED or 0) * 0x9E3779B97F4A7C15 + _SAMPLE_CALLS) & 0xFFFFFFFFFFFFFFFF


def _engine():
    import plagnn  # deferred: keeps `import dgl` cheap and the load order torch -> lib

    return plagnn


class _Frame(dict):
    """ndata / edata: name -> tensor whose first dimension is the node/edge count."""

    def __init__(self, n: int, kind: str):
        super().__init__()
        self._n = n
        self._kind = kind

    def __setitem__(self, key, value):
        if not isinstance(value, torch.Tensor):
            value = torch.as_tensor(value)
        if value.shape[0] != self._n:
            raise ValueError(f"{self._kind} data '{key}' has {value.shape[0]} rows, expected {self._n}")
        super().__setitem__(key, value)


class _NodeDataView:
    def __init__(self, g: "DGLGraph", ids):
        self._g = g
        self._ids = ids

    def __getitem__(self, key):
        t = self._g.ndata[key]
        return t if self._ids is None else t[self._index(t.device)]

    def __setitem__(self, key, value):
        if not isinstance(value, torch.Tensor):
            value = torch.as_tensor(value)
        n = self._g.num_nodes()
        idx = self._ids
        if idx is not None:
            ids = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
            if ids.numel() == n and bool((ids == torch.arange(n)).all()):
                idx = None  # full, in order (code/utils.py:46, 49 pass list(range(N)))
        if idx is None:
            self._g.ndata[key] = value
            return
        if key in self._g.ndata:
            self._g.ndata[key][self._index(self._g.ndata[key].device)] = value.to(self._g.ndata[key].device)
        else:
            buf = torch.zeros((n,) + tuple(value.shape[1:]), dtype=value.dtype, device=value.device)
            buf[self._index(value.device)] = value
            self._g.ndata[key] = buf

    def _index(self, device):
        return torch.as_tensor(self._ids, dtype=torch.int64, device=device)

    def keys(self):
        return self._g.ndata.keys()


class _NodeSpace:
    def __init__(self, g: "DGLGraph", ids):
        self.data = _NodeDataView(g, ids)


class _NodeView:
    def __init__(self, g: "DGLGraph"):
        self._g = g

    def __getitem__(self, ids):
        if isinstance(ids, slice) and ids == slice(None):
            ids = None
        return _NodeSpace(self._g, ids)

    def __call__(self):
        return torch.arange(self._g.num_nodes(), device=self._g.device)

    def __len__(self):
        return self._g.num_nodes()


class DGLGraph:
    """Homogeneous graph: COO edge list (edge id = position), node/edge frames, and the
    engine's CSR (built on first message passing, shared by every ``.to()`` copy)."""

    def __init__(self, src: torch.Tensor, dst: torch.Tensor, num_nodes: int, device=None,
                 _csr_cache=None):
        self._src = src.to(torch.int64)
        self._dst = dst.to(torch.int64)
        self._n = int(num_nodes)
        self._device = torch.device(device) if device is not None else self._src.device
        self._init_frames()
        self.edata = _Frame(int(self._src.numel()), "edge")
        self._csr_cache = _csr_cache if _csr_cache is not None else {}

    is_block = False

    def _init_frames(self):
        self.ndata = _Frame(self._n, "node")

    # --- structure -------------------------------------------------------------------
    def num_nodes(self, ntype=None) -> int:
        return self._n

    number_of_nodes = num_nodes

    def num_src_nodes(self, ntype=None) -> int:
        return self._n

    def num_dst_nodes(self, ntype=None) -> int:
        return self._n

    number_of_src_nodes = num_src_nodes
    number_of_dst_nodes = num_dst_nodes

    def num_edges(self, etype=None) -> int:
        return int(self._src.numel())

    number_of_edges = num_edges

    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def idtype(self):
        return torch.int64

    @property
    def nodes(self) -> _NodeView:
        return _NodeView(self)

    @property
    def srcdata(self):
        return self.ndata

    @property
    def dstdata(self):
        return self.ndata

    def edges(self, form: str = "uv", order: str = "eid"):
        if form != "uv":
            raise NotImplementedError("edges(form != 'uv')")
        return self._src.to(self._device), self._dst.to(self._device)

    def in_degrees(self, v=None):
        d = torch.bincount(self._dst.cpu(), minlength=self._n).to(self._device)
        return d if v is None else d[torch.as_tensor(v, device=self._device)]

    def out_degrees(self, u=None):
        d = torch.bincount(self._src.cpu(), minlength=self._n).to(self._device)
        return d if u is None else d[torch.as_tensor(u, device=self._device)]

    def is_homogeneous(self) -> bool:
        return True

    # --- edge queries ----------------------------------------------------------------
    def find_edges(self, eid, etype=None):
        """(src, dst) of the edges with ids `eid`, on the graph's device."""
        eid = _as_ids(eid).to(self._device)
        if eid.numel() and (int(eid.min()) < 0 or int(eid.max()) >= self.num_edges()):
            raise DGLError(f"find_edges: edge ids outside [0, {self.num_edges()})")
        src, dst = self._uv(self._device)
        return src[eid], dst[eid]

    def _lookup(self, u, v) -> torch.Tensor:
        """int32 edge id (the smallest) of every pair u[i] -> v[i], -1: no such edge
        (pg_edge_lookup on the graph's device). Node ids must lie inside the graph."""
        u, v = _as_ids(u).to(self._device), _as_ids(v).to(self._device)
        if u.numel() != v.numel():
            if u.numel() == 1:
                u = u.expand(v.numel())
            elif v.numel() == 1:
                v = v.expand(u.numel())
            else:
                raise DGLError("the lengths of u and v differ")
        for t, n in ((u, self.num_src_nodes()), (v, self.num_dst_nodes())):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
                raise DGLError(f"node ids outside [0, {n})")
        return _engine().ops.edge_lookup(self._device_graph(self._device), u.contiguous(), v.contiguous())

    def has_edges_between(self, u, v, etype=None) -> torch.Tensor:
        """bool per pair: whether the graph holds an edge u[i] -> v[i]."""
        return self._lookup(u, v) >= 0

    def edge_ids(self, u, v, return_uv: bool = False, etype=None) -> torch.Tensor:
        """The id of the edge u[i] -> v[i] per pair; where the graph holds it more than once, the
        smallest id. A pair that is not an edge raises DGLError, as DGL does. return_uv=True
        (every id of a multi-edge) is not supported."""
        if return_uv:
            raise NotImplementedError("edge_ids(return_uv=True) is not supported")
        eid = self._lookup(u, v).to(torch.int64)
        if eid.numel() and int(eid.min()) < 0:
            i = int((eid < 0).nonzero()[0])
            raise DGLError(f"edge_ids: no edge between the nodes of pair {i}")
        return eid

    # --- placement -------------------------------------------------------------------
    def to(self, device, **kwargs) -> "DGLGraph":
        device = torch.device(device)
        g = DGLGraph(self._src, self._dst, self._n, device=device, _csr_cache=self._csr_cache)
        for k, v in self.ndata.items():
            g.ndata[k] = v.to(device)
        for k, v in self.edata.items():
            g.edata[k] = v.to(device)
        if device.type == "cuda":
            self._engine_graph().on(device)  # upload the CSR once, eagerly (main_normal.py:66)
        return g

    def cpu(self) -> "DGLGraph":
        return self.to("cpu")

    def cuda(self, device=None) -> "DGLGraph":
        return self.to(torch.device("cuda") if device is None else device)

    # --- engine bridge ------------------------------------------------------------------
    def _engine_graph(self):
        if "host" not in self._csr_cache:
            self._csr_cache["host"] = _engine().CSRGraph(
                self._src.cpu().numpy(), self._dst.cpu().numpy(), self._n)
        return self._csr_cache["host"]

    def _device_graph(self, device=None):
        return self._engine_graph().on(device if device is not None else self._device)

    # --- message passing ----------------------------------------------------------------
    @contextlib.contextmanager
    def local_scope(self):
        frames = self._frames()
        saved = [dict(f) for f in frames]
        try:
            yield
        finally:
            for f, old in zip(frames, saved):
                dict.clear(f)
                dict.update(f, old)

    def _frames(self):
        return [self.ndata, self.edata]

    def update_all(self, message_func, reduce_func, apply_node_func=None, etype=None):
        from .function import _Message, _Reduce

        if not isinstance(message_func, _Message) or not isinstance(reduce_func, _Reduce):
            raise NotImplementedError("update_all supports dgl.function builtins only")
        parts = message_func.op.split("_")
        binary = len(parts) == 3 and parts[1] in _BINARY_OPS and {parts[0], parts[2]} == {"u", "e"}
        if message_func.op not in ("copy_u", "copy_e") and not binary:
            raise NotImplementedError(f"update_all: message function {message_func.op} is not supported")
        if reduce_func.msg != message_func.out:
            raise ValueError("reduce function reads a message the message function does not write")
        if not self._scalar_edge_form(message_func, reduce_func):
            self._update_all_gspmm(message_func, reduce_func)
            if apply_node_func is not None:
                self.dstdata.update(apply_node_func(_NodeBatch(self)))
            return
        X = self.srcdata[message_func.lhs]
        ew = None
        if message_func.op == "u_mul_e":
            ew = self.edata[message_func.rhs]
            if ew.dim() > 1:
                if ew.numel() != ew.shape[0]:
                    self._update_all_heads(X, ew, reduce_func)
                    if apply_node_func is not None:
                        self.dstdata.update(apply_node_func(_NodeBatch(self)))
                    return
                ew = ew.reshape(-1)
        shape = X.shape
        X2 = X.reshape(shape[0], -1)
        dg = self._device_graph(X.device)
        ews = dg.edge_weight_slots(ew)
        eng = _engine()
        if reduce_func.op == "max":
            out = eng.ops.MaxAggregate.apply(X2.float(), dg, ews)
        else:
            out = eng.ops.SumAggregate.apply(X2.float(), dg, ews, reduce_func.op == "mean")
        out = out.to(X.dtype).reshape((self.num_dst_nodes(),) + tuple(shape[1:]))
        self.dstdata[reduce_func.out] = out
        if apply_node_func is not None:
            self.dstdata.update(apply_node_func(_NodeBatch(self)))

    def _scalar_edge_form(self, message_func, reduce_func) -> bool:
        """True for the forms with at most one scalar per edge (or per head) that SAGEConv,
        GraphConv and GATConv use: copy_u, and u_mul_e whose edge feature is not a vector of
        the node feature's trailing shape, with sum / mean / max. They keep their entry points
        (pg_spmm_sum, pg_spmm_max_fwd, pg_spmm_sum_heads); everything else is pg_gspmm."""
        if reduce_func.op == "min" or message_func.op not in ("copy_u", "u_mul_e"):
            return False
        if message_func.op == "copy_u":
            return True
        X, ew = self.srcdata[message_func.lhs], self.edata[message_func.rhs]
        vector = ew.dim() >= 2 and ew.numel() != ew.shape[0] and X.shape[1:] == ew.shape[1:]
        return not vector

    def _field(self, target: str, name: str):
        return self.edata[name] if target == "e" else (self.srcdata if target == "u" else self.dstdata)[name]

    def _update_all_gspmm(self, message_func, reduce_func):
        """update_all on pg_gspmm: copy_e, copy_u with min, and u_<op>_e / e_<op>_u with node and
        edge features of equal trailing shapes (flattened to F), with sum / mean / max / min."""
        op = message_func.op
        if op == "copy_u":
            kop, lt, rt, lhs, rhs = "copy_lhs", "u", "e", self.srcdata[message_func.lhs], None
        elif op == "copy_e":
            kop, lt, rt, lhs, rhs = "copy_rhs", "u", "e", None, self.edata[message_func.lhs]
        else:
            lt, kop, rt = op.split("_")
            lhs, rhs = self._field(lt, message_func.lhs), self._field(rt, message_func.rhs)
            if lhs.shape[1:] != rhs.shape[1:]:
                raise NotImplementedError(f"{op}: node and edge features of equal trailing shapes are supported, "
                                          f"not {tuple(lhs.shape[1:])} with {tuple(rhs.shape[1:])}")
        ref = lhs if lhs is not None else rhs
        dg = self._device_graph(ref.device)

        def flat(t):
            return None if t is None else t.reshape(t.shape[0], -1).float()

        out = _engine().ops.GSpMM.apply(dg, kop, reduce_func.op, flat(lhs), flat(rhs), lt, rt)
        self.dstdata[reduce_func.out] = out.to(ref.dtype).reshape((self.num_dst_nodes(),) + tuple(ref.shape[1:]))

    def _update_all_heads(self, X, ew, reduce_func):
        """update_all(u_mul_e, sum) with (N, H, Fh) features and (E, H, 1) weights, H > 1:
        GATConv's aggregation, the engine's pg_spmm_sum_heads."""
        if X.dim() != 3 or ew.dim() != 3 or ew.shape[2] != 1:
            raise NotImplementedError("u_mul_e with multi-dimensional edge features: (N, H, Fh) node "
                                      "features with (E, H, 1) edge features are supported")
        if ew.shape[1] != X.shape[1]:
            raise ValueError(f"u_mul_e: {X.shape[1]} heads of node features, {ew.shape[1]} of edge features")
        if reduce_func.op != "sum":
            raise NotImplementedError(f"u_mul_e with multi-head edge features supports sum, not {reduce_func.op}")
        n, H, Fh = X.shape
        dg = self._device_graph(X.device)
        A = dg.edge_weight_slots(ew)
        out = _engine().ops.SumAggregateHeads.apply(X.reshape(n, H * Fh).float(), dg, A, H)
        self.dstdata[reduce_func.out] = out.to(X.dtype).reshape(self.num_dst_nodes(), H, Fh)

    def _uv(self, device):
        """(src, dst) per edge id on `device`, uploaded once per device."""
        key = ("uv", str(device))
        if key not in self._csr_cache:
            self._csr_cache[key] = (self._src.to(device), self._dst.to(device))
        return self._csr_cache[key]

    def apply_edges(self, func, edges=None, etype=None):
        """apply_edges(dgl.function.u_dot_v(lhs, rhs, out)): edata[out][e] = the dot product of
        ndata[lhs][src_e] and ndata[rhs][dst_e] in edge-id order (DGL's SDDMM): shape (E, 1)
        for 2-D operands (pg_sddmm_dot), (E, H, 1) for (N, H, Fh) operands (pg_sddmm_dot_heads).
        apply_edges(dgl.function.u_add_v(lhs, rhs, out)): edata[out][e] = ndata[lhs][src_e] +
        ndata[rhs][dst_e], any trailing shape. Every other binary builtin (two different
        targets of u, v, e; add, sub, mul, div, dot): _apply_edges_gsddmm."""
        from .function import _Message

        parts = func.op.split("_") if isinstance(func, _Message) else ()
        if len(parts) != 3 or parts[1] not in _BINARY_OPS + ("dot",) or parts[0] == parts[2] or edges is not None:
            raise NotImplementedError("apply_edges supports the binary dgl.function builtins on all edges only")
        if func.op not in ("u_dot_v", "v_dot_u", "u_add_v"):
            self._apply_edges_gsddmm(func, *parts)
            return
        if func.op == "v_dot_u":  # the same dot product with the operands named the other way
            func = _Message("u_dot_v", func.rhs, func.lhs, func.out)
        lhs, rhs = self.srcdata[func.lhs], self.dstdata[func.rhs]
        if lhs.shape[1:] != rhs.shape[1:]:
            raise ValueError(f"{func.op}: operand shapes {tuple(lhs.shape)} and {tuple(rhs.shape)} differ")
        dg = self._device_graph(lhs.device)
        n, nr = lhs.shape[0], rhs.shape[0]
        ops = _engine().ops
        if func.op == "u_add_v":
            src, dst = self._uv(lhs.device)
            out = ops.EdgeAdd.apply(lhs.reshape(n, -1).float(), rhs.reshape(nr, -1).float(), dg, src, dst)
            self.edata[func.out] = out.to(lhs.dtype).reshape((-1,) + tuple(lhs.shape[1:]))
            return
        if lhs.dim() == 3 and lhs.shape[1] > 1:
            H = lhs.shape[1]
            de = ops.EdgeDotHeads.apply(lhs.reshape(n, -1).float(), rhs.reshape(nr, -1).float(), dg, H)
        else:
            de = ops.EdgeDot.apply(lhs.reshape(n, -1).float(), rhs.reshape(nr, -1).float(), dg)
        # slot order -> edge-id order: eid is a permutation, so every element is written once
        out = torch.empty_like(de).index_copy(0, dg.eid, de)
        shape = (-1, lhs.shape[1], 1) if lhs.dim() == 3 else (-1, 1)
        self.edata[func.out] = out.to(lhs.dtype).reshape(shape)

    def _apply_edges_gsddmm(self, func, lt: str, op: str, rt: str):
        """apply_edges on pg_gsddmm: edata[out][e] = op(lhs at lt, rhs at rt) for operands of
        equal trailing shapes, in edge-id order; `dot` is the product summed over the last
        dimension (keepdim)."""
        lhs, rhs = self._field(lt, func.lhs), self._field(rt, func.rhs)
        if lhs.shape[1:] != rhs.shape[1:]:
            raise NotImplementedError(f"{func.op}: operands of equal trailing shapes are supported, "
                                      f"not {tuple(lhs.shape[1:])} with {tuple(rhs.shape[1:])}")
        dg = self._device_graph(lhs.device)
        out = _engine().ops.GSDDMM.apply(dg, "mul" if op == "dot" else op, lhs.reshape(lhs.shape[0], -1).float(),
                                         rhs.reshape(rhs.shape[0], -1).float(), lt, rt)
        out = out.to(lhs.dtype).reshape((-1,) + tuple(lhs.shape[1:]))
        if op == "dot":
            out = out.sum(-1, keepdim=True) if out.dim() > 1 else out
        self.edata[func.out] = out

    def __repr__(self):
        return (f"Graph(num_nodes={self._n}, num_edges={self.num_edges()},\n"
                f"      ndata_schemes={ {k: (tuple(v.shape[1:]), v.dtype) for k, v in self.ndata.items()} }\n"
                f"      edata_schemes={ {k: (tuple(v.shape[1:]), v.dtype) for k, v in self.edata.items()} })")


class _NodeBatch:
    def __init__(self, g: DGLGraph):
        self.data = g.dstdata


def _as_ids(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(torch.int64).reshape(-1)
    return torch.as_tensor(np.asarray(x, dtype=np.int64)).reshape(-1)


def graph(data, num_nodes: Optional[int] = None, idtype=None, device=None, **kwargs) -> DGLGraph:
    """dgl.graph((U, V), num_nodes=N): edge i goes U[i] -> V[i] (code/utils.py:44)."""
    if isinstance(data, tuple) and len(data) == 2:
        src, dst = _as_ids(data[0]), _as_ids(data[1])
    else:
        raise NotImplementedError("dgl.graph: only the (src, dst) form is supported")
    if src.numel() != dst.numel():
        raise ValueError("dgl.graph: src and dst lengths differ")
    n = int(num_nodes) if num_nodes is not None else (
        int(max(src.max().item(), dst.max().item())) + 1 if src.numel() else 0)
    if src.numel() and (int(src.min()) < 0 or int(dst.min()) < 0 or
                        int(src.max()) >= n or int(dst.max()) >= n):
        raise ValueError("dgl.graph: node id out of range")
    g = DGLGraph(src.cpu(), dst.cpu(), n)
    return g.to(device) if device is not None else g


def add_self_loop(g: DGLGraph, etype=None) -> DGLGraph:
    """dgl.add_self_loop (code/utils.py:45): one loop per node appended, so the new
    edges get ids E..E+N-1 (existing loops are kept; duplicates allowed). Edge features
    of the new loops are zero-filled, as DGL does."""
    n = g.num_nodes()
    loops = torch.arange(n, dtype=torch.int64)
    ng = DGLGraph(torch.cat([g._src.cpu(), loops]), torch.cat([g._dst.cpu(), loops]), n,
                  device=g.device)
    for k, v in g.ndata.items():
        ng.ndata[k] = v
    for k, v in g.edata.items():
        pad = torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
        ng.edata[k] = torch.cat([v, pad])
    return ng


def remove_self_loop(g: DGLGraph, etype=None) -> DGLGraph:
    keep = g._src != g._dst
    ng = DGLGraph(g._src[keep], g._dst[keep], g.num_nodes(), device=g.device)
    for k, v in g.ndata.items():
        ng.ndata[k] = v
    for k, v in g.edata.items():
        ng.edata[k] = v[keep.to(v.device)]
    return ng


class _NoFrame:
    """DGLBlock.ndata: a block has two node sets, as DGL says when ndata is touched."""

    def __init__(self, what: str):
        self._what = what

    def _fail(self, *a, **k):
        raise ValueError(f"{self._what} is ambiguous on a block (source and destination nodes are separate "
                         "sets): use srcdata or dstdata")

    __getitem__ = __setitem__ = __contains__ = __iter__ = __len__ = keys = items = values = update = pop = _fail


class DGLBlock(DGLGraph):
    """A bipartite message-flow graph ("block"): num_src source nodes, num_dst destination
    nodes, edges src -> dst in local ids (edge id = position), separate srcdata / dstdata
    frames. With include_dst_in_src (the only form built here) the first num_dst source nodes
    are the destination nodes. The engine graph is rectangular (CSRGraph.from_coo_rect, or the
    sampler's finished in-CSR through DeviceGraph.from_in_csr on a HIP device, CSRGraph.from_in_csr
    on the host)."""

    is_block = True

    def __init__(self, src: torch.Tensor, dst: torch.Tensor, num_src: int, num_dst: int, device=None,
                 _csr_cache=None):
        self._n_src, self._n_dst = int(num_src), int(num_dst)
        super().__init__(src, dst, self._n_src + self._n_dst, device=device, _csr_cache=_csr_cache)

    def _init_frames(self):
        self._srcdata = _Frame(self._n_src, "source node")
        self._dstdata = _Frame(self._n_dst, "destination node")

    @property
    def ndata(self):
        return _NoFrame("ndata")

    @property
    def nodes(self):
        raise ValueError("nodes is ambiguous on a block: use srcnodes / dstnodes")

    @property
    def srcdata(self):
        return self._srcdata

    @property
    def dstdata(self):
        return self._dstdata

    def srcnodes(self):
        return torch.arange(self._n_src, device=self._device)

    def dstnodes(self):
        return torch.arange(self._n_dst, device=self._device)

    def num_src_nodes(self, ntype=None) -> int:
        return self._n_src

    def num_dst_nodes(self, ntype=None) -> int:
        return self._n_dst

    number_of_src_nodes = num_src_nodes
    number_of_dst_nodes = num_dst_nodes

    def in_degrees(self, v=None):
        d = torch.bincount(self._dst.cpu(), minlength=self._n_dst).to(self._device)
        return d if v is None else d[torch.as_tensor(v, device=self._device)]

    def out_degrees(self, u=None):
        d = torch.bincount(self._src.cpu(), minlength=self._n_src).to(self._device)
        return d if u is None else d[torch.as_tensor(u, device=self._device)]

    def is_homogeneous(self) -> bool:
        return False

    def _frames(self):
        return [self._srcdata, self._dstdata, self.edata]

    def to(self, device, **kwargs) -> "DGLBlock":
        device = torch.device(device)
        g = DGLBlock(self._src, self._dst, self._n_src, self._n_dst, device=device, _csr_cache=self._csr_cache)
        for new, old in zip(g._frames(), self._frames()):
            for k, v in old.items():
                new[k] = v.to(device)
        if device.type == "cuda":
            self._engine_graph().on(device)
        return g

    def _engine_graph(self):
        if "host" not in self._csr_cache:
            self._csr_cache["host"] = _engine().CSRGraph.from_coo_rect(
                self._src.cpu().numpy(), self._dst.cpu().numpy(), self._n_src, self._n_dst)
        return self._csr_cache["host"]

    def __repr__(self):
        return (f"Block(num_src_nodes={self._n_src}, num_dst_nodes={self._n_dst}, "
                f"num_edges={self.num_edges()})")


def create_block(data, num_src_nodes: Optional[int] = None, num_dst_nodes: Optional[int] = None, idtype=None,
                 device=None) -> DGLBlock:
    """dgl.create_block((u, v), num_src_nodes, num_dst_nodes): edge i goes from source node u[i]
    to destination node v[i]."""
    if not (isinstance(data, tuple) and len(data) == 2):
        raise NotImplementedError("dgl.create_block: only the (src, dst) form is supported")
    src, dst = _as_ids(data[0]), _as_ids(data[1])
    if src.numel() != dst.numel():
        raise ValueError("dgl.create_block: src and dst lengths differ")
    ns = int(num_src_nodes) if num_src_nodes is not None else (int(src.max()) + 1 if src.numel() else 0)
    nd = int(num_dst_nodes) if num_dst_nodes is not None else (int(dst.max()) + 1 if dst.numel() else 0)
    if src.numel() and (int(src.min()) < 0 or int(dst.min()) < 0 or int(src.max()) >= ns or int(dst.max()) >= nd):
        raise ValueError("dgl.create_block: node id out of range")
    b = DGLBlock(src.cpu(), dst.cpu(), ns, nd)
    return b.to(device) if device is not None else b


def _block_from_in_csr(ptr, col_local, num_src: int, device) -> DGLBlock:
    """A block from a finished in-CSR on the host (numpy int32; edge id = slot): its engine graph
    is built by CSRGraph.from_in_csr with no COO sort."""
    import numpy as _np

    num_dst = len(ptr) - 1
    dst = _np.repeat(_np.arange(num_dst, dtype=_np.int64), _np.diff(ptr))
    cache = {"host": _engine().CSRGraph.from_in_csr(ptr, col_local, num_src)}
    return DGLBlock(torch.from_numpy(col_local.astype(_np.int64)), torch.from_numpy(dst), num_src, num_dst,
                    device=device, _csr_cache=cache)


def _block_from_device_csr(ptr, col_local, num_src: int) -> DGLBlock:
    """A block from a finished in-CSR on a HIP device (int32 tensors; edge id = slot): its engine
    graph is built there (plagnn.graph.DeviceBuiltGraph), and so are the block's COO arrays; no
    index array crosses the bus."""
    dev = ptr.device
    num_dst, total = ptr.numel() - 1, col_local.numel()
    dst = torch.repeat_interleave(torch.arange(num_dst, dtype=torch.int64, device=dev), ptr.diff().to(torch.int64),
                                  output_size=total)  # output_size: no synchronising read of the sum
    cache = {"host": _engine().graph.DeviceBuiltGraph(ptr, col_local, num_src)}
    return DGLBlock(col_local.to(torch.int64), dst, num_src, num_dst, device=dev, _csr_cache=cache)


def to_block(g: DGLGraph, dst_nodes=None, include_dst_in_src: bool = True) -> DGLBlock:
    """dgl.to_block: the block whose destination nodes are `dst_nodes` (default: the nodes of g
    with an in-edge, ascending) and whose source nodes are dst_nodes followed by every other
    source of g's edges in the order of its first appearance in edge-id order (pg_block_compact).
    Edge i of the block is edge i of g. srcdata[dgl.NID] / dstdata[dgl.NID] hold g's node ids,
    edata[dgl.EID] g's edge ids (the ids g itself carries in edata[dgl.EID] when it is a
    sampled frontier). Every edge of g must end in dst_nodes."""
    if g.is_block:
        raise NotImplementedError("dgl.to_block of a block")
    if not include_dst_in_src:
        raise NotImplementedError("dgl.to_block(include_dst_in_src=False) is not supported")
    dev = g.device
    src, dst = g._src.to(dev), g._dst.to(dev)
    n = g.num_nodes()
    if dst_nodes is None:
        dst_nodes = torch.unique(dst)  # sorted
    dst_nodes = _as_ids(dst_nodes).to(dev)
    src_ids, col_local = _engine().ops.block_compact(dst_nodes, src, n)
    inv = torch.full((n,), -1, dtype=torch.int64, device=dev)
    inv[dst_nodes] = torch.arange(dst_nodes.numel(), device=dev)
    dst_local = inv[dst]
    if dst.numel() and int(dst_local.min()) < 0:
        raise ValueError("dgl.to_block: an edge ends at a node that is not in dst_nodes")
    b = DGLBlock(col_local.to(torch.int64).cpu(), dst_local.cpu(), src_ids.numel(), dst_nodes.numel(), device=dev)
    b.srcdata[NID] = src_ids.to(torch.int64)
    b.dstdata[NID] = dst_nodes
    b.edata[EID] = g.edata[EID] if EID in g.edata else torch.arange(src.numel(), device=dev)
    return b


from . import sampling  # noqa: E402,F401  (dgl.sampling)
from . import dataloading  # noqa: E402,F401  (dgl.dataloading)

__all__ = ["DGLGraph", "DGLBlock", "DGLError", "graph", "create_block", "to_block", "add_self_loop",
           "remove_self_loop", "seed", "NID", "EID", "function", "nn", "ops", "sampling", "dataloading"]
