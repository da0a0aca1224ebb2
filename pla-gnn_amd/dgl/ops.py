"""dgl.ops: edge_softmax (DGL 0.8.2's ``dgl.ops.edge_softmax`` /
``dgl.nn.functional.edge_softmax``) on the engine's pg_edge_softmax_fwd / _bwd."""
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


__all__ = ["edge_softmax"]
