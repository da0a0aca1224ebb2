"""dgl.sampling: neighbour sampling on the engine's pg_sample_count / pg_sample_fill (with
excluded edges: pg_sample_count_excl / pg_sample_fill_excl), negative pairs on
pg_negative_sample."""
from __future__ import annotations

import contextlib

import torch


def _check_sampling(edge_dir, prob, replace):
    if edge_dir != "in":
        raise NotImplementedError("sample_neighbors: only edge_dir='in' is supported")
    if prob is not None:
        raise NotImplementedError("sample_neighbors: per-edge probabilities are not supported")
    if replace:
        raise NotImplementedError("sample_neighbors: sampling with replacement is not supported")


def _check_graph(g):
    import dgl

    if not isinstance(g, dgl.DGLGraph) or g.is_block:
        raise TypeError("expected a (non-block) dgl.DGLGraph built by this package")


@contextlib.contextmanager
def _excluded(g, eids):
    """The graph's exclusion bit set with the bits of `eids` set (None: no bit set at all, and
    None is yielded): they are set on entry and the same ids cleared on exit, also when the
    body raises, so the bit set is zero between batches at O(batch) cost."""
    import dgl
    from plagnn import ops

    if eids is None:
        yield None
        return
    dg = g._device_graph(g.device)
    ids = dgl._as_ids(eids).to(g.device)
    bits = dg.exclusion_bits()
    try:
        ops.edge_bits_update(bits, dg.num_edges, ids, set=True, check=True)
        yield bits
    finally:
        ops.edge_bits_update(bits, dg.num_edges, ids, set=False, check=False)


def _sample_csr(g, nodes, fanout, exclude=None):
    """(seeds int64, ptr, col, eid int32) on g's device: the sampled in-CSR of `nodes`, drawn
    with the next value of the counter dgl.seed starts. exclude: the bit set _excluded yields."""
    import dgl
    from plagnn import ops

    _check_graph(g)
    seeds = dgl._as_ids(nodes).to(g.device)
    ptr, col, eid = ops.sample_neighbors(g._device_graph(g.device), seeds, int(fanout), dgl._next_sample_seed(),
                                         exclude=exclude)
    return seeds, ptr, col, eid


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, exclude_edges=None, **kwargs):
    """dgl.sampling.sample_neighbors: up to `fanout` in-edges of every node of `nodes`, uniformly
    without replacement (fanout = -1: all of them), as a graph on g's node set whose
    edata[dgl.EID] holds the ids of the picked edges in g. An edge is kept when its key, a
    stateless function of (the call's seed, its edge id), is among the fanout smallest of its
    row; the call's seed comes from a counter that dgl.seed starts, so runs repeat.
    exclude_edges: ids of edges that are never picked; a node still receives `fanout` of the
    edges that remain."""
    import dgl

    _check_sampling(edge_dir, prob, replace)
    _check_graph(g)
    with _excluded(g, exclude_edges) as bits:
        seeds, ptr, col, eid = _sample_csr(g, nodes, fanout, bits)
    dst = torch.repeat_interleave(seeds, ptr.diff().to(torch.int64))
    sg = dgl.DGLGraph(col.to(torch.int64).cpu(), dst.cpu(), g.num_nodes(), device=g.device)
    sg.edata[dgl.EID] = eid.to(torch.int64)
    return sg


def _first_of_each_pair(src, dst, n_dst: int):
    """Indices (ascending) of the first slot of every distinct (src, dst) pair: a stable sort of
    the pairs' keys, then the slots where the key changes."""
    key = src.to(torch.int64) * int(n_dst) + dst.to(torch.int64)
    skey, order = torch.sort(key, stable=True)
    first = torch.ones_like(skey, dtype=torch.bool)
    first[1:] = skey[1:] != skey[:-1]
    return order[first].sort().values


def global_uniform_negative_sampling(g, num_samples, exclude_self_loops=True, replace=False, etype=None,
                                     redundancy=None):
    """dgl.sampling.global_uniform_negative_sampling: up to `num_samples` pairs (src, dst) that
    are not edges of g (and, with exclude_self_loops, have src != dst), both ends drawn uniformly
    (pg_negative_sample with rejection, 32 attempts per slot, slot ids 0 .. num_samples - 1). A
    slot whose attempts all fail is dropped, so fewer pairs than asked may come back, as in DGL.
    replace=False also drops repeated pairs, keeping each pair's first slot (a torch sort in this
    function). `redundancy` (DGL's oversampling factor) is accepted and ignored: the attempts per
    slot play its part. The seed comes from the counter dgl.seed starts."""
    import dgl
    from plagnn import ops

    _check_graph(g)
    if etype is not None:
        raise NotImplementedError("global_uniform_negative_sampling: etype is not supported")
    n = int(num_samples)
    if n < 0:
        raise ValueError("global_uniform_negative_sampling: num_samples must not be negative")
    src, dst, _ = ops.negative_sample(g._device_graph(g.device), None, None, n, 1, dgl._next_sample_seed(), tries=32,
                                      reject_edge=True, reject_self=bool(exclude_self_loops))
    keep = src >= 0
    src, dst = src[keep].to(torch.int64), dst[keep].to(torch.int64)
    if not replace and src.numel():
        first = _first_of_each_pair(src, dst, g.num_nodes())
        src, dst = src[first], dst[first]
    return src, dst


__all__ = ["sample_neighbors", "global_uniform_negative_sampling"]
