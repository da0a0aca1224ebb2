"""dgl.dataloading: multi-layer neighbour samplers that return blocks, the edge-prediction
wrapper around them (as_edge_prediction_sampler, negative_sampler) and a minimal single-process
DataLoader over node or edge ids. Choosing the neighbours (pg_sample_count /
pg_sample_fill) and relabelling them (pg_block_compact) run on the graph's device. On a HIP
device each block's transpose and work schedules are built there too (DeviceGraph.from_in_csr:
pg_csr_transpose_dev, pg_schedule_count_dev, pg_schedule_build_dev): per block the host reads
three small things back (the entry count, the source count, the schedule counts) and no index
array. On the CPU device, or with plagnn.graph.DEVICE_BUILD = False, the host builds them
(CSRGraph.from_in_csr). Seed edges left out of the blocks (exclude_eids) go through a bit set
over edge ids that the batch sets and clears (pg_edge_bits_update) and pg_sample_*_excl."""
from __future__ import annotations

import torch

from . import negative_sampler  # noqa: F401  (dgl.dataloading.negative_sampler)


def _resolve(device) -> torch.device:
    """`device` with its index filled in ('cuda' is the current HIP device), so that 'cuda' and
    'cuda:0' compare equal."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class NeighborSampler:
    """dgl.dataloading.NeighborSampler(fanouts): fanouts[i] in-neighbours per node for layer i
    (-1: all), layer 0 the one nearest the input features. edge_dir='out', prob and replace
    are not supported."""

    def __init__(self, fanouts, edge_dir="in", prob=None, replace=False, **kwargs):
        from ..sampling import _check_sampling

        _check_sampling(edge_dir, prob, replace)
        self.fanouts = [int(f) for f in fanouts]

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        """(input_nodes, output_nodes, blocks): the outermost (output) layer is sampled first
        and the list is built back to front, as DGL does. The sampled CSR goes straight to the
        block's engine graph (no COO round trip). exclude_eids: ids of edges that no layer may
        pick (a destination still receives `fanout` of its other in-edges); their bits are set
        before the first layer and cleared after the last, also when a layer raises."""
        import dgl

        from ..sampling import _check_graph, _excluded

        _check_graph(g)
        output_nodes = dgl._as_ids(seed_nodes).to(g.device)
        with _excluded(g, exclude_eids) as bits:
            return self._sample_layers(g, output_nodes, bits)

    def _sample_layers(self, g, output_nodes, bits):
        import dgl
        from plagnn import graph as engine_graph
        from plagnn import ops

        from ..sampling import _sample_csr

        seeds = output_nodes
        blocks = []
        for fanout in reversed(self.fanouts):
            seeds, ptr, col, eid = _sample_csr(g, seeds, fanout, bits)
            src_ids, col_local = ops.block_compact(seeds, col, g.num_nodes())
            if engine_graph.DEVICE_BUILD and ptr.device.type == "cuda":
                b = dgl._block_from_device_csr(ptr, col_local, src_ids.numel())
            else:
                b = dgl._block_from_in_csr(ptr.cpu().numpy(), col_local.cpu().numpy(), src_ids.numel(), g.device)
            src_ids = src_ids.to(torch.int64)
            b.srcdata[dgl.NID] = src_ids
            b.dstdata[dgl.NID] = seeds
            b.edata[dgl.EID] = eid.to(torch.int64)
            blocks.insert(0, b)
            seeds = src_ids
        return seeds, output_nodes, blocks

    sample = sample_blocks


MultiLayerNeighborSampler = NeighborSampler


class MultiLayerFullNeighborSampler(NeighborSampler):
    """Every in-neighbour at each of n_layers layers."""

    def __init__(self, n_layers, **kwargs):
        super().__init__([-1] * int(n_layers), **kwargs)


class _EdgePredictionSampler:
    """What as_edge_prediction_sampler returns: sample(g, seed_edges) ->
    (input_nodes, pair_graph, blocks), or (input_nodes, pair_graph, neg_graph, blocks) with a
    negative sampler.

    pair_graph holds the seed edges in the order given on a compacted node set: edata[dgl.EID]
    = the seed edge ids, ndata[dgl.NID] = the parent ids of its nodes. neg_graph holds the
    negative pairs in slot order on the same node set, with the same ndata[dgl.NID]. The node set
    is ops.block_compact of cat(pos_src, pos_dst, neg_src, neg_dst) with no destination list:
    nodes in the order of their first appearance. The blocks are sampler.sample_blocks(g,
    pair_graph.ndata[dgl.NID], exclude_eids=...), so blocks[-1].dstdata[dgl.NID] equals the pair
    graphs' NID. The two small pair graphs are built through the host-side DGLGraph constructor
    (one copy of 2 (1 + k) batch-size ids to the host), as dgl.sampling.sample_neighbors builds
    its result; the per-batch kernels are the sampler's."""

    def __init__(self, sampler, exclude, reverse_eids, negative_sampler):
        import dgl

        if exclude not in (None, "self", "reverse_id"):
            raise NotImplementedError(f"as_edge_prediction_sampler: exclude={exclude!r} is not supported "
                                      "(None, 'self' and 'reverse_id' are)")
        if exclude == "reverse_id" and reverse_eids is None:
            raise ValueError("as_edge_prediction_sampler: exclude='reverse_id' needs reverse_eids")
        self.sampler, self.exclude, self.negative_sampler = sampler, exclude, negative_sampler
        self.reverse_eids = None if reverse_eids is None else dgl._as_ids(reverse_eids)

    def _excluded_ids(self, g, seed_edges):
        if self.exclude is None:
            return None
        if self.exclude == "self":
            return seed_edges
        if self.reverse_eids.device != seed_edges.device:
            self.reverse_eids = self.reverse_eids.to(seed_edges.device)
        return torch.cat([seed_edges, self.reverse_eids[seed_edges]])

    def sample(self, g, seed_edges):
        import dgl
        from plagnn import ops

        seed_edges = dgl._as_ids(seed_edges).to(g.device)
        src, dst = g.find_edges(seed_edges)
        ends = [src, dst]
        if self.negative_sampler is not None:
            ends += [t.to(g.device) for t in self.negative_sampler(g, seed_edges)]
        nodes, local = ops.block_compact(torch.empty(0, dtype=torch.int64, device=g.device), torch.cat(ends),
                                         g.num_nodes())
        nodes, local = nodes.to(torch.int64), local.to(torch.int64).cpu()
        n_pos, n_neg = seed_edges.numel(), ends[-1].numel() if len(ends) == 4 else 0
        pair_graph = dgl.DGLGraph(local[:n_pos], local[n_pos:2 * n_pos], nodes.numel(), device=g.device)
        pair_graph.ndata[dgl.NID] = nodes
        pair_graph.edata[dgl.EID] = seed_edges
        graphs = [pair_graph]
        if self.negative_sampler is not None:
            neg_graph = dgl.DGLGraph(local[2 * n_pos:2 * n_pos + n_neg], local[2 * n_pos + n_neg:], nodes.numel(),
                                     device=g.device)
            neg_graph.ndata[dgl.NID] = nodes
            graphs.append(neg_graph)
        input_nodes, _, blocks = self.sampler.sample_blocks(g, nodes, exclude_eids=self._excluded_ids(g, seed_edges))
        return (input_nodes, *graphs, blocks)


def as_edge_prediction_sampler(sampler, exclude=None, reverse_eids=None, negative_sampler=None, **kwargs):
    """dgl.dataloading.as_edge_prediction_sampler: `sampler` (a NeighborSampler) seeded by edges.
    exclude: None, 'self' (the seed edges are left out of the blocks) or 'reverse_id' (and the
    edges reverse_eids[seed] with them); 'reverse_types' and callables are not supported.
    negative_sampler: a callable (g, eids) -> (src, dst), dgl.dataloading.negative_sampler.*.
    See _EdgePredictionSampler for what sample() returns."""
    if kwargs.get("reverse_etypes") is not None or kwargs.get("prefetch_labels") is not None:
        raise NotImplementedError("as_edge_prediction_sampler: reverse_etypes / prefetch_labels are not supported")
    return _EdgePredictionSampler(sampler, exclude, reverse_eids, negative_sampler)


def _to_device(x, device):
    if isinstance(x, (list, tuple)):
        return type(x)(_to_device(y, device) for y in x)
    return x.to(device)


class DataLoader:
    """dgl.dataloading.DataLoader(graph, indices, graph_sampler, device=None, batch_size=1,
    shuffle=False, drop_last=False): iterates what the sampler's sample(graph, batch) returns,
    (input_nodes, output_nodes, blocks) over batches of node ids for a NeighborSampler,
    (input_nodes, pair_graph[, neg_graph], blocks) over batches of edge ids for an
    edge-prediction sampler, in this process (num_workers > 0 raises). `shuffle` draws a
    permutation per epoch from `generator` (a torch.Generator; default: torch's global one).
    Batches are moved to `device` when it differs from the graph's."""

    def __init__(self, graph, indices, graph_sampler, device=None, batch_size=1, shuffle=False, drop_last=False,
                 num_workers=0, generator=None, **kwargs):
        import dgl

        if num_workers:
            raise NotImplementedError("DataLoader: num_workers > 0 is not supported (single process only)")
        if kwargs.get("use_ddp") or kwargs.get("use_uva"):
            raise NotImplementedError("DataLoader: use_ddp / use_uva are not supported")
        self.graph, self.sampler = graph, graph_sampler
        self.indices = dgl._as_ids(indices)
        self.device = _resolve(device) if device is not None else _resolve(graph.device)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.generator = generator
        if self.batch_size < 1:
            raise ValueError("DataLoader: batch_size must be positive")

    def __len__(self):
        n = self.indices.numel()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        ids = self.indices
        if self.shuffle:
            ids = ids[torch.randperm(ids.numel(), generator=self.generator).to(ids.device)]
        for i in range(len(self)):
            batch = ids[i * self.batch_size:(i + 1) * self.batch_size]
            out = tuple(self.sampler.sample(self.graph, batch))
            if self.device != _resolve(self.graph.device):
                out = _to_device(out, self.device)
            yield out


NodeDataLoader = DataLoader


class EdgeDataLoader(DataLoader):
    """dgl.dataloading.EdgeDataLoader(g, eids, graph_sampler, exclude=None, reverse_eids=None,
    negative_sampler=None, **kw), DGL 0.8's wrapper: a DataLoader over edge ids whose sampler is
    as_edge_prediction_sampler(graph_sampler, exclude, reverse_eids, negative_sampler)."""

    def __init__(self, g, eids, graph_sampler, exclude=None, reverse_eids=None, negative_sampler=None, **kwargs):
        super().__init__(g, eids, as_edge_prediction_sampler(graph_sampler, exclude=exclude,
                                                             reverse_eids=reverse_eids,
                                                             negative_sampler=negative_sampler), **kwargs)


__all__ = ["NeighborSampler", "MultiLayerNeighborSampler", "MultiLayerFullNeighborSampler", "DataLoader",
           "NodeDataLoader", "EdgeDataLoader", "as_edge_prediction_sampler", "negative_sampler"]
