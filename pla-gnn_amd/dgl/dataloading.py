"""dgl.dataloading: multi-layer neighbour samplers that return blocks, and a minimal
single-process DataLoader over node ids. Choosing the neighbours (pg_sample_count /
pg_sample_fill) and relabelling them (pg_block_compact) run on the graph's device. On a HIP
device each block's transpose and work schedules are built there too (DeviceGraph.from_in_csr:
pg_csr_transpose_dev, pg_schedule_count_dev, pg_schedule_build_dev): per block the host reads
three small things back (the entry count, the source count, the schedule counts) and no index
array. On the CPU device, or with plagnn.graph.DEVICE_BUILD = False, the host builds them
(CSRGraph.from_in_csr)."""
from __future__ import annotations

import torch


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
        from .sampling import _check_sampling

        _check_sampling(edge_dir, prob, replace)
        self.fanouts = [int(f) for f in fanouts]

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        """(input_nodes, output_nodes, blocks): the outermost (output) layer is sampled first
        and the list is built back to front, as DGL does. The sampled CSR goes straight to the
        block's engine graph (no COO round trip)."""
        import dgl
        from plagnn import graph as engine_graph
        from plagnn import ops

        from .sampling import _sample_csr

        if exclude_eids is not None:
            raise NotImplementedError("exclude_eids is not supported")
        output_nodes = dgl._as_ids(seed_nodes).to(g.device)
        seeds = output_nodes
        blocks = []
        for fanout in reversed(self.fanouts):
            seeds, ptr, col, eid = _sample_csr(g, seeds, fanout)
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


class DataLoader:
    """dgl.dataloading.DataLoader(graph, indices, graph_sampler, device=None, batch_size=1,
    shuffle=False, drop_last=False): iterates (input_nodes, output_nodes, blocks) over
    batches of node ids, in this process (num_workers > 0 raises). `shuffle` draws a
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
            inp, out, blocks = self.sampler.sample(self.graph, batch)
            if self.device != _resolve(self.graph.device):
                inp, out, blocks = inp.to(self.device), out.to(self.device), [b.to(self.device) for b in blocks]
            yield inp, out, blocks


NodeDataLoader = DataLoader

__all__ = ["NeighborSampler", "MultiLayerNeighborSampler", "MultiLayerFullNeighborSampler", "DataLoader",
           "NodeDataLoader"]
