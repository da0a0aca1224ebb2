"""dgl.nn.pytorch: SAGEConv (the reference's layer, code/model.py:7, 13-15), GraphConv,
GATConv, GATv2Conv and EdgeConv, with DGL 0.8.2's constructor signatures, parameter names and initialisation, computed by
the plagnn engine."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import plagnn
from plagnn import ops


def _check_graph(graph):
    import dgl

    if not isinstance(graph, dgl.DGLGraph):
        raise TypeError("expected a dgl.DGLGraph built by this package")


def _pair_feats(in_feats):
    """dgl.utils.expand_as_pair of a layer's in_feats: (source width, destination width)."""
    if isinstance(in_feats, tuple):
        return int(in_feats[0]), int(in_feats[1])
    return in_feats, in_feats


def _expand(graph, feat):
    """dgl.utils.expand_as_pair(feat, graph): a (feat_src, feat_dst) pair as given (a block
    only: a square graph here has one node frame); one tensor on a block feeds its first
    num_dst rows to the destinations (include_dst_in_src); on a square graph both are feat."""
    if isinstance(feat, tuple):
        if not graph.is_block:
            raise NotImplementedError("a (feat_src, feat_dst) pair needs a block (dgl.to_block / dgl.create_block)")
        return feat[0], feat[1]
    if graph.is_block:
        return feat, feat[:graph.num_dst_nodes()]
    return feat, feat


class SAGEConv(nn.Module):
    """DGL 0.8.2 ``SAGEConv(in_feats, out_feats, aggregator_type, feat_drop=0., bias=True,
    norm=None, activation=None)``.

    'pool' (the reference's aggregator): ``relu(fc_pool(h))`` max-aggregated over in-edges,
    then ``fc_self(h) + fc_neigh(neigh) + bias``; the whole layer runs as one fused
    autograd function on the engine (ops.SagePool). 'mean' and 'gcn' are provided for
    the aggregator variants the reference does not use (reference-unpinned); 'lstm' is
    not supported.
    """

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True,
                 norm=None, activation=None):
        super().__init__()
        valid = {"mean", "pool", "gcn", "lstm"}
        if aggregator_type not in valid:
            raise KeyError(f"Invalid aggregator_type. Must be one of {valid}. "
                           f"But got {aggregator_type!r} instead.")
        if aggregator_type == "lstm":
            raise NotImplementedError("SAGEConv 'lstm' is not provided by this engine")
        self._in_src_feats, self._in_dst_feats = _pair_feats(in_feats)
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self.norm = norm
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation
        if aggregator_type == "pool":
            self.fc_pool = nn.Linear(self._in_src_feats, self._in_src_feats)
        self.fc_neigh = nn.Linear(self._in_src_feats, out_feats, bias=False)
        if aggregator_type != "gcn":
            self.fc_self = nn.Linear(self._in_dst_feats, out_feats, bias=False)
        if bias:
            self.bias = nn.parameter.Parameter(torch.zeros(out_feats))
        else:
            self.register_buffer("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self._aggre_type == "pool":
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        if self._aggre_type != "gcn":
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, graph, feat, edge_weight=None):
        _check_graph(graph)
        if isinstance(feat, tuple):
            feat = (self.feat_drop(feat[0]), self.feat_drop(feat[1]))
        else:
            feat = self.feat_drop(feat)
        feat_src, feat_dst = _expand(graph, feat)
        dg = graph._device_graph(feat_src.device)
        ews = dg.edge_weight_slots(edge_weight)
        if self._aggre_type == "pool" and not graph.is_block:
            rst = ops.SagePool.apply(feat_src.float(), self.fc_pool.weight, self.fc_pool.bias,
                                     self.fc_self.weight, self.fc_neigh.weight, self.bias, dg, ews)
        elif self._aggre_type == "pool":
            # a block: the layer as DGL composes it, the max aggregation on the engine's
            # rectangular graph (the fused ops.SagePool assumes one node set)
            pooled = F.relu(self.fc_pool(feat_src)).float()
            h_neigh = ops.MaxAggregate.apply(pooled, dg, ews).to(feat_src.dtype)
            rst = self.fc_self(feat_dst) + self.fc_neigh(h_neigh)
            if self.bias is not None:
                rst = rst + self.bias
        else:
            lin_before_mp = self._in_src_feats > self._out_feats
            h = self.fc_neigh(feat_src) if lin_before_mp else feat_src
            if self._aggre_type == "mean":
                h_neigh = ops.SumAggregate.apply(h, dg, ews, True)
            else:  # gcn: (sum of neighbours + self) / (in-degree + 1)
                s = ops.SumAggregate.apply(h, dg, ews, False)
                degs = dg.in_degrees()
                if not graph.is_block:
                    h_self = h
                elif isinstance(feat, tuple):
                    h_self = self.fc_neigh(feat_dst) if lin_before_mp else feat_dst
                else:
                    h_self = h[:graph.num_dst_nodes()]
                h_neigh = (s + h_self) / (degs.unsqueeze(-1).to(feat_src.dtype) + 1)
            if not lin_before_mp:
                h_neigh = self.fc_neigh(h_neigh)
            rst = h_neigh if self._aggre_type == "gcn" else self.fc_self(feat_dst) + h_neigh
            if self.bias is not None:
                rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst

    def extra_repr(self):
        return f"in={self._in_src_feats}, out={self._out_feats}, aggregator_type={self._aggre_type!r}"


class GraphConv(nn.Module):
    """DGL 0.8.2 ``GraphConv(in_feats, out_feats, norm='both', weight=True, bias=True,
    activation=None, allow_zero_in_degree=False)`` on the engine's sum aggregation.
    Not used by the reference (BASELINE config 0 names it): reference-unpinned."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True,
                 activation=None, allow_zero_in_degree=False):
        super().__init__()
        if norm not in ("none", "both", "right", "left"):
            raise ValueError(f'Invalid norm value. Must be either "none", "both", "right" or '
                             f'"left". But got "{norm}".')
        self._in_feats, self._out_feats, self._norm = in_feats, out_feats, norm
        self._allow_zero_in_degree = allow_zero_in_degree
        self.weight = nn.Parameter(torch.Tensor(in_feats, out_feats)) if weight else None
        self.bias = nn.Parameter(torch.Tensor(out_feats)) if bias else None
        self._activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, graph, feat, weight=None, edge_weight=None):
        _check_graph(graph)
        feat, _ = _expand(graph, feat)  # only the source features are read; norms are per side
        dg = graph._device_graph(feat.device)
        eg = graph._engine_graph()
        if not self._allow_zero_in_degree and eg.has_zero_in_degree():
            raise plagnn.PlagnnError("There are 0-in-degree nodes in the graph; add self-loops "
                                     "or set allow_zero_in_degree=True")
        ews = dg.edge_weight_slots(edge_weight)
        if self._norm in ("left", "both"):
            degs = dg.out_degrees().float().clamp(min=1)
            norm = torch.pow(degs, -0.5) if self._norm == "both" else 1.0 / degs
            feat = feat * norm.reshape(-1, 1)
        w = weight if weight is not None else self.weight
        if self._in_feats > self._out_feats:
            if w is not None:
                feat = feat @ w
            rst = ops.SumAggregate.apply(feat, dg, ews, False)
        else:
            rst = ops.SumAggregate.apply(feat, dg, ews, False)
            if w is not None:
                rst = rst @ w
        if self._norm in ("right", "both"):
            degs = dg.in_degrees().float().clamp(min=1)
            norm = torch.pow(degs, -0.5) if self._norm == "both" else 1.0 / degs
            rst = rst * norm.reshape(-1, 1)
        if self.bias is not None:
            rst = rst + self.bias
        if self._activation is not None:
            rst = self._activation(rst)
        return rst


class GATConv(nn.Module):
    """DGL 0.8.2 ``GATConv(in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0.,
    negative_slope=0.2, residual=False, activation=None, allow_zero_in_degree=False,
    bias=True)``, its forward written as DGL writes it on the shim's own primitives:
    apply_edges(u_add_v), edge_softmax and update_all(u_mul_e, sum), which run on the engine's
    multi-head kernels. Not used by the reference: reference-unpinned."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2,
                 residual=False, activation=None, allow_zero_in_degree=False, bias=True):
        super().__init__()
        if isinstance(in_feats, tuple):
            # the suite pins this rejection; blocks and (feat_src, feat_dst) pairs of one width
            # run through the shared fc, as DGL does for an int in_feats
            raise NotImplementedError("GATConv with a tuple in_feats (separate fc_src / fc_dst) is not supported")
        self._num_heads = num_heads
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.attn_r = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        if bias:
            self.bias = nn.Parameter(torch.FloatTensor(size=(num_heads * out_feats,)))
        else:
            self.register_buffer("bias", None)
        if residual:
            if self._in_dst_feats != out_feats * num_heads:
                self.res_fc = nn.Linear(self._in_dst_feats, num_heads * out_feats, bias=False)
            else:
                self.res_fc = nn.Identity()
        else:
            self.register_buffer("res_fc", None)
        self.reset_parameters()
        self.activation = activation

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        import dgl.function as fn
        from dgl.ops import edge_softmax

        _check_graph(graph)
        with graph.local_scope():
            if not self._allow_zero_in_degree and graph._engine_graph().has_zero_in_degree():
                raise plagnn.PlagnnError("There are 0-in-degree nodes in the graph; add self-loops "
                                         "or set allow_zero_in_degree=True")
            H, out = self._num_heads, self._out_feats
            if isinstance(feat, tuple):
                h_src, h = _expand(graph, (self.feat_drop(feat[0]), self.feat_drop(feat[1])))
                ft = self.fc(h_src).view(-1, H, out)
                ft_dst = self.fc(h).view(-1, H, out)
            else:
                h_src = h = self.feat_drop(feat)
                ft = ft_dst = self.fc(h).view(-1, H, out)
                if graph.is_block:  # the destinations are the first num_dst sources
                    ft_dst = ft[:graph.num_dst_nodes()]
                    h = h[:graph.num_dst_nodes()]
            el = (ft * self.attn_l).sum(dim=-1).unsqueeze(-1)
            er = (ft_dst * self.attn_r).sum(dim=-1).unsqueeze(-1)
            graph.srcdata.update({"ft": ft, "el": el})
            graph.dstdata.update({"er": er})
            graph.apply_edges(fn.u_add_v("el", "er", "e"))
            e = self.leaky_relu(graph.edata.pop("e"))
            graph.edata["a"] = self.attn_drop(edge_softmax(graph, e))
            graph.update_all(fn.u_mul_e("ft", "a", "m"), fn.sum("m", "ft"))
            rst = graph.dstdata["ft"]
            if self.res_fc is not None:
                rst = rst + self.res_fc(h).view(h.shape[0], -1, self._out_feats)
            if self.bias is not None:
                rst = rst + self.bias.view(1, self._num_heads, self._out_feats)
            if self.activation:
                rst = self.activation(rst)
            if get_attention:
                return rst, graph.edata["a"]
            return rst


class GATv2Conv(nn.Module):
    """DGL 0.8 ``GATv2Conv(in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0.,
    negative_slope=0.2, residual=False, activation=None, allow_zero_in_degree=False, bias=True,
    share_weights=False)`` (Brody, Alon, Yahav, "How Attentive are Graph Attention Networks?",
    ICLR 2022): e_uv = attn . leaky_relu(fc_src(h_u) + fc_dst(h_v)) per head, softmax over the
    in-edges of v, and the source projections fc_src(h_u) summed with those weights.

    The score does not factor into per-node scalars, so it runs on its own fused kernel
    (ops.GATv2Score: no (E, H, out) tensor, forward or backward); the softmax and the
    aggregation are the engine's multi-head kernels. Parameters are named as DGL's (fc_src,
    fc_dst, attn, res_fc; fc_dst is fc_src with share_weights) and initialised as DGL does
    (xavier_normal_ with the relu gain, zero biases). As in DGL, ``bias`` is the bias of the
    linear maps (the residual map included); the layer has no separate output bias. The
    message is the source projection, as in the paper's eq. 7 with W split into [W_l | W_r]
    and in DGL. Not used by the reference, and written from the paper and the DGL 0.8 module
    as documented (DGL is not installed where this is built): reference-unpinned."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2,
                 residual=False, activation=None, allow_zero_in_degree=False, bias=True, share_weights=False):
        super().__init__()
        if isinstance(in_feats, tuple):
            # the suite pins this rejection; blocks and (feat_src, feat_dst) pairs of one width
            # are accepted with an int in_feats
            raise NotImplementedError("GATv2Conv with a tuple in_feats is not supported")
        self._num_heads = num_heads
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self._negative_slope = float(negative_slope)
        self.fc_src = nn.Linear(self._in_src_feats, out_feats * num_heads, bias=bias)
        if share_weights:
            self.fc_dst = self.fc_src
        else:
            self.fc_dst = nn.Linear(self._in_dst_feats, out_feats * num_heads, bias=bias)
        self.attn = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        if residual:
            if self._in_dst_feats != out_feats * num_heads:
                self.res_fc = nn.Linear(self._in_dst_feats, num_heads * out_feats, bias=bias)
            else:
                self.res_fc = nn.Identity()
        else:
            self.register_buffer("res_fc", None)
        self.activation = activation
        self.share_weights = share_weights
        self.bias = bias
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc_src.weight, gain=gain)
        if self.bias:
            nn.init.constant_(self.fc_src.bias, 0)
        if not self.share_weights:
            nn.init.xavier_normal_(self.fc_dst.weight, gain=gain)
            if self.bias:
                nn.init.constant_(self.fc_dst.bias, 0)
        nn.init.xavier_normal_(self.attn, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)
            if self.bias:
                nn.init.constant_(self.res_fc.bias, 0)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        _check_graph(graph)
        if not self._allow_zero_in_degree and graph._engine_graph().has_zero_in_degree():
            raise plagnn.PlagnnError("There are 0-in-degree nodes in the graph; add self-loops "
                                     "or set allow_zero_in_degree=True")
        H, out = self._num_heads, self._out_feats
        if isinstance(feat, tuple):
            h_src, h = _expand(graph, (self.feat_drop(feat[0]), self.feat_drop(feat[1])))
            feat = h_src
            el = self.fc_src(h_src).float()
            er = self.fc_dst(h).float()
        else:
            h_src = h = self.feat_drop(feat)
            el = self.fc_src(h).float()
            if graph.is_block:  # the destinations are the first num_dst sources
                h = h[:graph.num_dst_nodes()]
                er = el[:h.shape[0]] if self.share_weights else self.fc_dst(h).float()
            else:
                er = el if self.share_weights else self.fc_dst(h).float()
        dg = graph._device_graph(feat.device)
        s = ops.GATv2Score.apply(el, er, self.attn, dg, H, self._negative_slope)  # (E, H), slot order
        a = self.attn_drop(ops.EdgeSoftmax.apply(s, dg))
        rst = ops.SumAggregateHeads.apply(el, dg, a, H).to(feat.dtype).view(-1, H, out)
        if self.res_fc is not None:
            rst = rst + self.res_fc(h).view(h.shape[0], -1, out)
        if self.activation:
            rst = self.activation(rst)
        if get_attention:
            # slot order -> edge-id order: eid is a permutation, so every element is written once
            return rst, torch.empty_like(a).index_copy(0, dg.eid, a).to(feat.dtype).unsqueeze(-1)
        return rst


class EdgeConv(nn.Module):
    """DGL 0.8.2 ``EdgeConv(in_feat, out_feat, batch_norm=False, allow_zero_in_degree=False)``
    (Wang et al., Dynamic Graph CNN): h_v = max over in-edges (u -> v) of
    theta(h_v - h_u) + phi(h_v) (v_sub_u, as DGL's code has it), written on the shim's own primitives (vector edge features on
    pg_gsddmm / pg_gspmm): apply_edges(v_sub_u), theta on the edge tensor, apply_edges(e_add_v),
    optionally batch norm over the edges, update_all(copy_e, max). Parameters are named as
    DGL's (theta, phi, bn). Not used by the reference: reference-unpinned."""

    def __init__(self, in_feat, out_feat, batch_norm=False, allow_zero_in_degree=False):
        super().__init__()
        if isinstance(in_feat, tuple):  # DGL's EdgeConv has one width too: theta reads h_v - h_u
            raise NotImplementedError("EdgeConv takes one in_feat; a (feat_src, feat_dst) pair of that width "
                                      "is accepted by forward on a block")
        self.batch_norm = batch_norm
        self._allow_zero_in_degree = allow_zero_in_degree
        self.theta = nn.Linear(in_feat, out_feat)
        self.phi = nn.Linear(in_feat, out_feat)
        if batch_norm:
            self.bn = nn.BatchNorm1d(out_feat)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, g, feat):
        import dgl.function as fn

        _check_graph(g)
        h_src, h_dst = _expand(g, feat)
        with g.local_scope():
            if not self._allow_zero_in_degree and g._engine_graph().has_zero_in_degree():
                raise plagnn.PlagnnError("There are 0-in-degree nodes in the graph; add self-loops "
                                         "or set allow_zero_in_degree=True")
            g.srcdata["x"] = h_src
            g.dstdata["x"] = h_dst
            g.apply_edges(fn.v_sub_u("x", "x", "theta"))
            g.edata["theta"] = self.theta(g.edata["theta"])
            g.dstdata["phi"] = self.phi(h_dst)
            g.apply_edges(fn.e_add_v("theta", "phi", "e"))
            if self.batch_norm:
                g.edata["e"] = self.bn(g.edata["e"])
            g.update_all(fn.copy_e("e", "e"), fn.max("e", "x"))
            return g.dstdata["x"]


__all__ = ["SAGEConv", "GraphConv", "GATConv", "GATv2Conv", "EdgeConv"]
