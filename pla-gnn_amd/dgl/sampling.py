"""dgl.sampling: neighbour sampling on the engine's pg_sample_count / pg_sample_fill."""
from __future__ import annotations

import torch


def _check_sampling(edge_dir, prob, replace):
    if edge_dir != "in":
        raise NotImplementedError("sample_neighbors: only edge_dir='in' is supported")
    if prob is not None:
        raise NotImplementedError("sample_neighbors: per-edge probabilities are not supported")
    if replace:
        raise NotImplementedError("sample_neighbors: sampling with replacement is not supported")


def _sample_csr(g, nodes, fanout):
    """(seeds int64, ptr, col, eid int32) on g's device: the sampled in-CSR of `nodes`, drawn
    with the next value of the counter dgl.seed starts."""
    import dgl
    from plagnn import ops

    if not isinstance(g, dgl.DGLGraph) or g.is_block:
        raise TypeError("expected a (non-block) dgl.DGLGraph built by this package")
    seeds = dgl._as_ids(nodes).to(g.device)
    ptr, col, eid = ops.sample_neighbors(g._device_graph(g.device), seeds, int(fanout), dgl._next_sample_seed())
    return seeds, ptr, col, eid


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, **kwargs):
    """dgl.sampling.sample_neighbors: up to `fanout` in-edges of every node of `nodes`, uniformly
    without replacement (fanout = -1: all of them), as a graph on g's node set whose
    edata[dgl.EID] holds the ids of the picked edges in g. An edge is kept when its key, a
    stateless function of (the call's seed, its edge id), is among the fanout smallest of its
    row; the call's seed comes from a counter that dgl.seed starts, so runs repeat."""
    import dgl

    _check_sampling(edge_dir, prob, replace)
    seeds, ptr, col, eid = _sample_csr(g, nodes, fanout)
    dst = torch.repeat_interleave(seeds, ptr.diff().to(torch.int64))
    sg = dgl.DGLGraph(col.to(torch.int64).cpu(), dst.cpu(), g.num_nodes(), device=g.device)
    sg.edata[dgl.EID] = eid.to(torch.int64)
    return sg


__all__ = ["sample_neighbors"]
