"""dgl.dataloading.negative_sampler: negative pairs for link prediction, on pg_negative_sample.
A sampler is called as sampler(g, eids) with the ids of the positive edges and returns (src, dst)
int64 on g's device, k pairs per positive edge in slot order (edge i's pairs at i * k .. i * k +
k - 1). The seed of a call comes from the counter dgl.seed starts."""
from __future__ import annotations

import torch


class Uniform:
    """negative_sampler.Uniform(k) (PerSourceUniform): for every positive edge u -> v, k pairs
    u -> v' with v' uniform over the nodes. No rejection, as in DGL: a pair may be an edge. The
    draws are keyed by the positive edge's id, so an edge gets the same negatives wherever it
    stands in its batch."""

    def __init__(self, k):
        self.k = int(k)
        if self.k < 1:
            raise ValueError("negative_sampler.Uniform: k must be positive")

    def __call__(self, g, eids):
        import dgl
        from plagnn import ops

        from ..sampling import _check_graph

        _check_graph(g)
        eids = dgl._as_ids(eids).to(g.device)
        src, _ = g.find_edges(eids)
        neg_src, neg_dst, _ = ops.negative_sample(g._device_graph(g.device), src, eids, eids.numel(), self.k,
                                                  dgl._next_sample_seed(), tries=1)
        return neg_src.to(torch.int64), neg_dst.to(torch.int64)


PerSourceUniform = Uniform


class GlobalUniform:
    """negative_sampler.GlobalUniform(k, exclude_self_loops=True, replace=False): k * len(eids)
    pairs drawn by dgl.sampling.global_uniform_negative_sampling (non-edges only; fewer may
    come back). `redundancy` is accepted and ignored, as there."""

    def __init__(self, k, exclude_self_loops=True, replace=False, redundancy=None):
        self.k = int(k)
        if self.k < 1:
            raise ValueError("negative_sampler.GlobalUniform: k must be positive")
        self.exclude_self_loops, self.replace = bool(exclude_self_loops), bool(replace)

    def __call__(self, g, eids):
        import dgl

        from ..sampling import global_uniform_negative_sampling

        n = dgl._as_ids(eids).numel() * self.k
        return global_uniform_negative_sampling(g, n, self.exclude_self_loops, self.replace)


__all__ = ["Uniform", "PerSourceUniform", "GlobalUniform"]
