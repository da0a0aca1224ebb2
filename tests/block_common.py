"""Shared by test_block_cpu.py and test_gpu_block.py: neighbour sampling (pg_sample_count /
pg_sample_fill), block compaction (pg_block_compact), rectangular graphs in the aggregation
kernels, and the dgl shim's blocks, samplers, loader and bipartite layers, each check
parametrised by the device.

References
  sampler      pg_sample_*_cpu is the statement of the device result (bitwise); its properties
               (counts, membership, no repeats, ascending edge ids) are checked from the parent
               CSR alone, its uniformity against binomial bounds.
  compaction   pg_block_compact_cpu, plus a restatement in Python of the ordering rule.
  rectangular  a bipartite graph of ns sources and nd destinations is the square graph on
               max(ns, nd) nodes whose other nodes are isolated, with the same in-CSR slot
               order (the same stable sort): the float64 restatements of gspmm_common,
               gat_common, gatv2_common and sddmm_common run on that square graph with
               zero-padded operands, and the kernels on the rectangular graph must meet them
               at those files' bars (grid inputs: bitwise).
  full graph   MultiLayerFullNeighborSampler blocks keep every in-edge of their destinations in
               ascending edge id, which is the parent's row order: aggregations are bitwise
               the parent's rows; layers within 1e-5 of each tensor's magnitude (the tolerance
               of the existing layer tests; the GEMM tiling may differ with M).
"""
import functools

import numpy as np
import pytest
import torch

import gat_common as gc
import gatv2_common as gv
import gspmm_common as gs
import sddmm_common as sc
from sddmm_common import U, _leaf, close

FANOUT = 5
FANOUTS = [0, 1, FANOUT, 70, 600, -1]  # 600: a hub row whose candidates do not fit LDS
NEW_SYMBOLS = ["pg_sample_count", "pg_sample_count_workspace", "pg_sample_fill", "pg_block_compact",
               "pg_block_compact_workspace", "pg_sample_count_cpu", "pg_sample_fill_cpu", "pg_block_compact_cpu"]


def lds_keys():
    from plagnn import _lib

    return _lib.PG_SAMPLE_LDS_KEYS


# ------------------------------------------------------------------ sampler
@functools.lru_cache(maxsize=None)
def sampler_graph():
    """A parent graph with in-degrees at every edge of the algorithm: 0, 1, fanout - 1, fanout,
    fanout + 1, 63, 64, 65 (the wave width), the LDS key capacity and one more, and a hub row
    past twice the capacity. Edges in shuffled order, so slot -> edge id is not the identity."""
    import plagnn

    cap = lds_keys()
    degs = [0, 1, FANOUT - 1, FANOUT, FANOUT + 1, 63, 64, 65, 0, 200, cap, cap + 1, 2 * cap + 37]
    n = 700
    rng = np.random.default_rng(5)
    dst = np.concatenate([np.full(d, v, np.int64) for v, d in enumerate(degs)])
    src = rng.integers(0, n, len(dst)).astype(np.int64)
    perm = rng.permutation(len(dst))
    g = plagnn.CSRGraph(src[perm], dst[perm], n)
    assert list(g.in_degrees()[:len(degs)]) == degs and (g.eid != np.arange(len(dst))).any()
    return g, len(degs)


def sample(dev, g, seeds, fanout, seed):
    from plagnn import ops

    ptr, col, eid = ops.sample_neighbors(g.on(dev), torch.as_tensor(seeds, dtype=torch.int64), fanout, seed)
    assert ptr.dtype == col.dtype == eid.dtype == torch.int32 and ptr.device.type == torch.device(dev).type
    return ptr.cpu().numpy(), col.cpu().numpy(), eid.cpu().numpy()


def rows_of(ptr, col, eid):
    return [(tuple(col[ptr[i]:ptr[i + 1]]), tuple(eid[ptr[i]:ptr[i + 1]])) for i in range(len(ptr) - 1)]


def check_sampler_properties(g, seeds, fanout, ptr, col, eid):
    """Independent of the twin: counts, membership in the parent row, no repeats, ascending."""
    gp, gc_, ge = g.fwd.ptr, g.fwd.col, g.eid
    assert ptr[0] == 0 and len(ptr) == len(seeds) + 1 and ptr[-1] == len(col) == len(eid)
    for i, s in enumerate(seeds):
        deg = int(gp[s + 1] - gp[s])
        want = deg if fanout < 0 else min(deg, fanout)
        c, e = col[ptr[i]:ptr[i + 1]], eid[ptr[i]:ptr[i + 1]]
        assert len(e) == want, f"seed {s}: {len(e)} entries, min(deg, fanout) = {want}"
        assert (np.diff(e) > 0).all(), f"seed {s}: edge ids do not ascend strictly (repeats or disorder)"
        parent = dict(zip(ge[gp[s]:gp[s + 1]].tolist(), gc_[gp[s]:gp[s + 1]].tolist()))
        assert all(parent.get(int(a), -1) == int(b) for a, b in zip(e, c)), f"seed {s}: not an entry of its row"


def check_sampler(dev, fanout):
    """Device against the CPU twin (bitwise), repeatability, permutation of the seeds."""
    g, k = sampler_graph()
    rng = np.random.default_rng(fanout + 11)
    seeds = np.concatenate([np.arange(k), [k - 1, 3, 3, 650], rng.integers(0, g.num_dst, 40)])
    got = sample(dev, g, seeds, fanout, 1234)
    check_sampler_properties(g, seeds, fanout, *got)
    twin = sample("cpu", g, seeds, fanout, 1234)
    for a, b, name in zip(got, twin, ("ptr", "col", "eid")):
        assert np.array_equal(a, b), f"fanout {fanout}: {name} differs from pg_sample_*_cpu"
    again = sample(dev, g, seeds, fanout, 1234)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two runs differ"
    perm = rng.permutation(len(seeds))
    moved = rows_of(*sample(dev, g, seeds[perm], fanout, 1234))
    rows = rows_of(*got)
    assert moved == [rows[p] for p in perm], "a row depends on its place in seeds"
    if 0 < fanout < 60:
        other = rows_of(*sample(dev, g, seeds, fanout, 1235))
        assert other != rows, "another seed gives the same sample"
        assert rows[k - 1] == rows[k], "a repeated seed in one call draws the same entries"


def check_sampler_empty(dev):
    import plagnn

    g, _ = sampler_graph()
    for fanout in (3, -1):
        ptr, col, eid = sample(dev, g, np.zeros(0, np.int64), fanout, 1)
        assert list(ptr) == [0] and len(col) == 0 and len(eid) == 0
    e = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 9)
    ptr, col, eid = sample(dev, e, np.arange(9), 4, 1)
    assert list(ptr) == [0] * 10 and len(col) == 0
    with pytest.raises(ValueError):
        sample(dev, g, np.array([g.num_dst]), 2, 1)


def check_sampler_many_seeds(dev):
    """More seeds than one scan tile holds, and more tiles than one pass of the tile scan."""
    g, k = sampler_graph()
    for n_seeds in (1025, 256 * 1024 + 700):
        seeds = np.random.default_rng(n_seeds).integers(0, 10, n_seeds)
        got = sample(dev, g, seeds, 2, 9)
        deg = np.minimum(g.in_degrees()[seeds], 2)
        assert np.array_equal(got[0], np.concatenate([[0], np.cumsum(deg)])), "out_ptr is not the exclusive scan"
        twin = sample("cpu", g, seeds, 2, 9)
        assert all(np.array_equal(a, b) for a, b in zip(got, twin))


def check_uniformity():
    """On the CPU twin (deterministic): one row of degree 10, fanout 3, seeds 0 .. 3999: every
    edge's inclusion count within 1200 +- 145 (five standard deviations of Binomial(4000, 0.3));
    two rows of degree 10 in one call pick the same position set at most 70 times (expectation
    4000 / C(10, 3) = 33, standard deviation 5.7)."""
    import plagnn

    dst = np.repeat(np.arange(2), 10)
    g = plagnn.CSRGraph(np.arange(20) % 7, dst, 20)
    counts = np.zeros(10, np.int64)
    same = 0
    for s in range(4000):
        ptr, col, eid = sample("cpu", g, [0, 1], 3, s)
        assert list(ptr) == [0, 3, 6]
        counts[eid[:3]] += 1
        same += tuple(eid[:3]) == tuple(eid[3:] - 10)
    print("inclusion counts", counts.tolist(), "equal position sets", same)
    assert (np.abs(counts - 1200) <= 145).all(), counts
    assert same <= 70, same


# ------------------------------------------------------------------ compaction
def compact(dev, dst_ids, col, n_parent):
    from plagnn import ops

    src_ids, col_local = ops.block_compact(torch.as_tensor(dst_ids, dtype=torch.int64).to(dev),
                                           torch.as_tensor(col, dtype=torch.int64).to(dev), n_parent)
    assert src_ids.dtype == col_local.dtype == torch.int32
    return src_ids.cpu().numpy(), col_local.cpu().numpy()


def compact_py(dst_ids, col):
    order = list(dst_ids)
    seen = {v: i for i, v in enumerate(order)}
    for c in col:
        if c not in seen:
            seen[c] = len(order)
            order.append(c)
    return np.array(order, np.int32), np.array([seen[c] for c in col], np.int32)


def check_compact(dev):
    # a source that appears first late in col (11), a dst id that is also a source (5, 2)
    src_ids, col_local = compact(dev, [5, 2, 9], [7, 2, 7, 3, 5, 11, 3], 12)
    assert src_ids.tolist() == [5, 2, 9, 7, 3, 11] and col_local.tolist() == [3, 1, 3, 4, 0, 5, 4]
    rng = np.random.default_rng(2)
    for n_parent, n_dst, nnz in ((50, 7, 300), (5000, 1300, 9000), (400000, 1024, 270000)):
        dst_ids = rng.permutation(n_parent)[:n_dst]
        col = rng.integers(0, n_parent, nnz)
        got = compact(dev, dst_ids, col, n_parent)
        ref = compact_py(dst_ids.tolist(), col.tolist())
        twin = compact("cpu", dst_ids, col, n_parent)
        for a, b, c in zip(got, ref, twin):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.array_equal(got[0][got[1]], col), "src_ids[col_local] != col"
        assert np.array_equal(got[0][:n_dst], dst_ids)
    with pytest.raises(ValueError, match="duplicate"):
        compact(dev, [4, 1, 4], [0, 1], 6)
    with pytest.raises(ValueError):
        compact(dev, [4, 1], [0, 6], 6)
    src_ids, col_local = compact(dev, [3, 0], [], 5)
    assert src_ids.tolist() == [3, 0] and len(col_local) == 0
    src_ids, col_local = compact(dev, [], [], 5)
    assert len(src_ids) == 0 and len(col_local) == 0


# ------------------------------------------------------------------ rectangular kernels
@functools.lru_cache(maxsize=None)
def rect(ns, nd, hub=300):
    """(rectangular CSRGraph, its square embedding, src, dst): random edges plus a 300-edge hub
    row (destination 0, split at the default chunk), in shuffled order."""
    import plagnn

    rng = np.random.default_rng(ns * 100 + nd)
    e0 = 4 * max(ns, nd)
    src = np.concatenate([rng.integers(0, ns, e0), rng.integers(0, ns, hub)]).astype(np.int64)
    dst = np.concatenate([rng.integers(1, nd, e0), np.zeros(hub, np.int64)])
    dst[:3] = nd - 1
    src[3:6] = ns - 1
    perm = rng.permutation(len(src))
    src, dst = src[perm], dst[perm]
    g = plagnn.CSRGraph.from_coo_rect(src, dst, ns, nd)
    sq = plagnn.CSRGraph(src, dst, max(ns, nd))
    assert (g.num_src, g.num_dst, g.fwd.n_rows, g.bwd.n_rows, g.fwd.n_cols, g.bwd.n_cols) == (ns, nd, nd, ns, ns, nd)
    assert g.fwd.n_merges == 1 and g.fwd.max_deg >= hub
    assert np.array_equal(g.fwd.ptr, sq.fwd.ptr[:nd + 1]) and np.array_equal(g.fwd.col, sq.fwd.col)
    assert np.array_equal(g.bwd.ptr, sq.bwd.ptr[:ns + 1]) and np.array_equal(g.bwd.col, sq.bwd.col)
    assert np.array_equal(g.bwd.eslot, sq.bwd.eslot) and np.array_equal(g.eid, sq.eid)
    if ns != nd:
        with pytest.raises(ValueError):
            g.num_nodes
    return g, sq, src, dst


def check_from_in_csr(ns, nd):
    """from_in_csr on a finished in-CSR gives the transpose and schedules of the COO build."""
    import plagnn

    g, _, _, _ = rect(ns, nd)
    h = plagnn.CSRGraph.from_in_csr(g.fwd.ptr, g.fwd.col, ns)
    assert (h.num_src, h.num_dst, h.num_edges) == (ns, nd, g.num_edges) and np.array_equal(h.eid, np.arange(h.num_edges))
    for a, b in ((h.fwd, g.fwd), (h.bwd, g.bwd)):
        for f in ("ptr", "col", "items", "merges"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert (a.n_rows, a.n_cols, a.n_items, a.n_merges, a.n_slots, a.max_deg) == \
               (b.n_rows, b.n_cols, b.n_items, b.n_merges, b.n_slots, b.max_deg)
    assert np.array_equal(h.bwd.eslot, g.bwd.eslot) and np.array_equal(h.bwd.epos, g.bwd.epos)
    with pytest.raises(ValueError):
        plagnn.CSRGraph.from_in_csr([0, 2], [0], 3)


def pad_rows(a, n):
    out = np.zeros((n,) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


def sides(g, transpose):
    """(rows of the output, rows of the gathered operand)."""
    return (g.num_src, g.num_dst) if transpose else (g.num_dst, g.num_src)


def check_rect_gspmm(dev, ns, nd, op, reduce, family, transpose=False, F=12):
    from plagnn import ops

    g, sq, _, _ = rect(ns, nd)
    N = sq.num_nodes
    n_out, n_in = sides(g, transpose)
    rng = np.random.default_rng(7)
    if family == "gauss":
        L, R = rng.standard_normal((n_in, F)).astype(np.float32), rng.standard_normal((g.num_edges, F)).astype(np.float32)
    else:
        L, R = gs.grid_nodes(rng, n_in, F), gs.grid_edges(rng, g.num_edges, F)
    row, colr, pos, erow, earg, ptr = gs.entries(sq, transpose)
    m = gs.messages(op, pad_rows(L, N), "u", R, "e", row, colr, erow)
    ref, bar, arg = gs.reduce_ref(m, row, ptr, N, reduce)
    Lt = sc.to_dev(L, dev) if op != "copy_rhs" else None
    Rt = sc.to_dev(R, dev) if op != "copy_lhs" else None
    res = ops.gspmm(g.on(dev), op, reduce, Lt, Rt, "u", "e", transpose=transpose)
    got, rec = res if reduce in ("max", "min") else (res, None)
    name = f"rect {ns}x{nd} gspmm {op}/{reduce} {family} T={transpose}"
    assert tuple(got.shape) == (n_out, F), name
    assert not ref[n_out:].any()
    ref, bar = ref[:n_out], bar[:n_out]
    if family == "grid" and reduce != "mean":
        assert np.array_equal(got.cpu().numpy().astype(np.float64), ref), f"{name}: not bitwise the reference"
        if rec is not None:
            assert np.array_equal(sc.argpos_np(rec), arg[:n_out]), f"{name}: records differ from the first winner"
    elif family == "grid":
        gc.within(got, ref, 2.0 ** -23 * np.abs(ref) + 1e-300, name)
    else:
        gc.within(got, ref, bar, name)


def check_rect_gsddmm(dev, ns, nd, lt, rt, family, op="mul", F=8):
    from plagnn import ops

    g, sq, _, _ = rect(ns, nd)
    N = sq.num_nodes
    rows = {"u": ns, "v": nd, "e": g.num_edges}
    rng = np.random.default_rng(9)
    if family == "gauss":
        L, R = (rng.standard_normal((rows[t], F)).astype(np.float32) for t in (lt, rt))
    else:
        L = gs.grid_edges(rng, rows[lt], F) if lt == "e" else gs.grid_nodes(rng, rows[lt], F)
        R = gs.grid_edges(rng, rows[rt], F)
    row, colr, pos, erow, earg, ptr = gs.entries(sq, False)
    emb = lambda a, t: a if t == "e" else pad_rows(a, N)  # noqa: E731
    m = gs.messages(op, emb(L, lt), lt, emb(R, rt), rt, row, colr, erow)
    ref = np.zeros_like(m)
    ref[erow] = m
    got = ops.gsddmm(g.on(dev), op, sc.to_dev(L, dev), sc.to_dev(R, dev), lt, rt)
    name = f"rect {ns}x{nd} gsddmm {lt}_{op}_{rt} {family}"
    if family == "grid":
        assert np.array_equal(got.cpu().numpy().astype(np.float64), ref), f"{name}: not bitwise the reference"
    else:
        gc.within(got, ref, 2 * U * np.abs(ref) + 1e-300, name)


def check_rect_heads(dev, ns, nd, H=3, Fh=8):
    """edge_softmax forward / backward, spmm_sum_heads in both directions, sddmm_dot_heads and
    sddmm_dot (plain, mean, max form) against gat_common's / sddmm_common's references."""
    from plagnn import ops

    g, sq, _, _ = rect(ns, nd)
    N, E, F = sq.num_nodes, g.num_edges, H * Fh
    dg = g.on(dev)
    rng = np.random.default_rng(13)
    tag = f"rect {ns}x{nd}"
    s = (rng.standard_normal((E, H)) * 3).astype(np.float32)
    a64, bar, _ = gc.softmax_ref(sq, s)
    a = ops.edge_softmax(dg, sc.to_dev(s, dev))
    gc.within(a, a64, bar, tag + " softmax fwd")
    an, da = a.cpu().numpy(), rng.standard_normal((E, H)).astype(np.float32)
    ref, bar = gc.softmax_bwd_ref(sq, an, da)
    gc.within(ops.edge_softmax_backward(dg, a, sc.to_dev(da, dev)), ref, bar, tag + " softmax bwd")
    for transpose in (False, True):
        n_out, n_in = sides(g, transpose)
        X = rng.standard_normal((n_in, F)).astype(np.float32)
        ref, bar, _ = gc.sum_heads_ref(sq, an, pad_rows(X, N), H, transpose)
        out = ops.spmm_sum_heads(dg, a, sc.to_dev(X, dev), H, transpose=transpose)
        assert tuple(out.shape) == (n_out, F) and not ref[n_out:].any()
        gc.within(out, ref[:n_out], bar[:n_out], f"{tag} sum_heads T={transpose}")
    D, X = rng.standard_normal((nd, F)).astype(np.float32), rng.standard_normal((ns, F)).astype(np.float32)
    ref, bar = gc.sddmm_heads_ref(sq, pad_rows(D, N), pad_rows(X, N), H)
    gc.within(ops.sddmm_dot_heads(dg, sc.to_dev(D, dev), sc.to_dev(X, dev), H), ref, bar, tag + " sddmm heads")
    Dt, Xt = sc.to_dev(D, dev), sc.to_dev(X, dev)
    for mean in (False, True):
        ref, bar = sc.sddmm_ref(sq, pad_rows(D, N), pad_rows(X, N), mean=mean)
        gc.within(ops.sddmm_dot(dg, Dt, Xt, mean=mean), ref, bar, f"{tag} sddmm mean={mean}")
    out, argpos = ops.spmm_max(dg, Xt)
    assert tuple(out.shape) == (nd, F)
    pad_arg = torch.full((N, F), -1, dtype=argpos.dtype)
    pad_arg[:nd] = argpos.cpu()
    ref, bar = sc.sddmm_ref(sq, pad_rows(D, N), pad_rows(X, N), argpos=pad_arg)
    gc.within(ops.sddmm_dot(dg, Dt, Xt, argpos=argpos), ref, bar, tag + " sddmm max form")


def check_rect_aggregates(dev, ns, nd, F=12):
    """ops.MaxAggregate / SumAggregate (sum, mean), weighted and not, with gradients in the
    features and the weights, and the GATv2 score with its three gradients, against float64 torch
    (gspmm_common.reduce64, gatv2_common.score64) at 1e-5 of each tensor's magnitude."""
    from plagnn import ops

    g, _, src, dst = rect(ns, nd)
    dg = g.on(dev)
    E = g.num_edges
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    rng = np.random.default_rng(17)
    for reduce in ("max", "sum", "mean"):
        for weighted in (False, True):
            x, w = gc._randn(rng, ns, F), gc._randn(rng, E)
            xd, wd, x64, w64 = _leaf(x, dev), _leaf(w, dev), _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
            ews = dg.edge_weight_slots(wd) if weighted else None
            out = ops.MaxAggregate.apply(xd, dg, ews) if reduce == "max" else \
                ops.SumAggregate.apply(xd, dg, ews, reduce == "mean")
            assert tuple(out.shape) == (nd, F)
            m64 = x64[s] * w64[:, None] if weighted else x64[s]
            ref = gs.reduce64(m64, d, nd, reduce)
            gs._compare(out, ref, (xd, wd) if weighted else (xd,), (x64, w64) if weighted else (x64,), rng,
                        f"rect {ns}x{nd} {reduce} weighted={weighted}")
            assert tuple(xd.grad.shape) == (ns, F)
    H, Fh = 3, 4
    xl, xr, attn = gc._randn(rng, ns, H * Fh), gc._randn(rng, nd, H * Fh), gc._randn(rng, 1, H, Fh)
    leaves = [_leaf(t, dev) for t in (xl, xr, attn)]
    leaves64 = [_leaf(t, dtype=torch.float64) for t in (xl, xr, attn)]
    sc_slots = ops.GATv2Score.apply(leaves[0], leaves[1], leaves[2], dg, H, 0.2)
    out = torch.empty_like(sc_slots).index_copy(0, dg.eid, sc_slots)  # slot order -> edge-id order
    ref = gv.score64(s, d, leaves64[0].view(ns, H, Fh), leaves64[1].view(nd, H, Fh), leaves64[2], 0.2)
    gs._compare(out, ref, leaves, leaves64, rng, f"rect {ns}x{nd} gatv2 score")
    assert tuple(leaves[0].grad.shape) == (ns, H * Fh) and tuple(leaves[1].grad.shape) == (nd, H * Fh)


# ------------------------------------------------------------------ the shim on blocks
def check_block_surface(dev):
    import dgl
    import dgl.function as fn

    u, v = torch.tensor([0, 3, 4, 1, 4, 2]), torch.tensor([0, 0, 1, 1, 1, 2])
    b = dgl.create_block((u, v), num_src_nodes=5, num_dst_nodes=3).to(dev)
    assert b.is_block and isinstance(b, dgl.DGLGraph) and not dgl.graph((u, v)).is_block
    assert (b.num_src_nodes(), b.num_dst_nodes(), b.number_of_src_nodes(), b.number_of_dst_nodes()) == (5, 3, 5, 3)
    assert b.num_edges() == 6 and b.in_degrees().tolist() == [2, 3, 1] and b.out_degrees().tolist() == [1, 1, 1, 1, 2]
    with pytest.raises(ValueError):
        b.ndata["h"] = torch.zeros(5)
    with pytest.raises(ValueError):
        b.ndata["h"]
    with pytest.raises(ValueError):
        b.srcdata["h"] = torch.zeros(3, 2)
    x = torch.arange(10, dtype=torch.float32, device=dev).reshape(5, 2)
    b.srcdata["h"] = x
    b.dstdata["h"] = -x[:3]
    assert "h" in b.srcdata and b.srcdata["h"] is not b.dstdata["h"]
    with b.local_scope():
        b.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
        assert "o" in b.dstdata and "o" not in b.srcdata
        assert torch.equal(b.dstdata["o"].cpu(), torch.stack([x[0] + x[3], x[4] + x[1] + x[4], x[2]]).cpu())
        b.apply_edges(fn.u_add_v("h", "h", "e"))
        assert torch.equal(b.edata["e"].cpu(), (x[u] - x[v]).cpu())
    assert "o" not in b.dstdata and "e" not in b.edata
    c = b.to(dev)
    assert c.is_block and torch.equal(c.srcdata["h"], x) and c.num_dst_nodes() == 3
    assert dgl.NID == dgl.EID == "_ID"


def check_block_update_all(dev, ns, nd):
    """update_all / apply_edges builtins on a block read u from srcdata, v from dstdata, write
    reducers to dstdata; against float64 torch with gradients."""
    import dgl
    import dgl.function as fn

    _, _, src, dst = rect(ns, nd)
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    E = len(src)
    rng = np.random.default_rng(23)
    b = dgl.create_block((s, d), ns, nd).to(dev)
    for msg, reduce in (("copy_u", "max"), ("u_mul_e", "sum"), ("u_mul_e", "mean"), ("e_sub_u", "min"),
                        ("u_add_e", "max"), ("copy_e", "sum"), ("u_div_e", "sum"), ("copy_u", "min")):
        shape = (6,)
        x, y = gc._randn(rng, ns, *shape), gc._randn(rng, E, *shape)
        if "div" in msg:
            y = y.sign() * (y.abs() + 0.5)
        xd, yd, x64, y64 = _leaf(x, dev), _leaf(y, dev), _leaf(x, dtype=torch.float64), _leaf(y, dtype=torch.float64)
        b.srcdata["h"], b.edata["w"] = xd, yd
        if msg == "copy_u":
            mf, m64, leaves = fn.copy_u("h", "m"), x64[s], ((xd,), (x64,))
        elif msg == "copy_e":
            mf, m64, leaves = fn.copy_e("w", "m"), y64 * 1.0, ((yd,), (y64,))
        else:
            lt, op, rt = msg.split("_")
            names, vals = {"u": "h", "e": "w"}, {"u": x64[s], "e": y64}
            mf, m64, leaves = getattr(fn, msg)(names[lt], names[rt], "m"), gs.op64(op, vals[lt], vals[rt]), \
                ((xd, yd), (x64, y64))
        b.update_all(mf, getattr(fn, reduce)("m", "o"))
        out = b.dstdata["o"]
        assert tuple(out.shape) == (nd,) + shape
        gs._compare(out, gs.reduce64(m64, d, nd, reduce), leaves[0], leaves[1], rng, f"block {ns}x{nd} {msg}/{reduce}")
    # scalar and per-head weights (pg_spmm_sum / pg_spmm_max_fwd / pg_spmm_sum_heads)
    x, w = gc._randn(rng, ns, 2, 4), gc._randn(rng, E, 2, 1)
    xd, wd, x64, w64 = _leaf(x, dev), _leaf(w, dev), _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    b.srcdata["h"], b.edata["a"] = xd, wd
    b.update_all(fn.u_mul_e("h", "a", "m"), fn.sum("m", "o"))
    ref = gs.reduce64((x64[s] * w64).reshape(E, 8), d, nd, "sum").reshape(nd, 2, 4)
    gs._compare(b.dstdata["o"], ref, (xd, wd), (x64, w64), rng, f"block {ns}x{nd} heads")
    for msg in ("u_dot_v", "u_add_v", "v_sub_u", "u_mul_v", "e_add_v", "u_div_e"):
        lt, op, rt = msg.split("_")
        rows = {"u": ns, "v": nd, "e": E}
        l, r = gc._randn(rng, rows[lt], 2, 4), gc._randn(rng, rows[rt], 2, 4)
        if op == "div":
            r = r.sign() * (r.abs() + 0.5)
        ld, rd, l64, r64 = _leaf(l, dev), _leaf(r, dev), _leaf(l, dtype=torch.float64), _leaf(r, dtype=torch.float64)
        frames = {"u": b.srcdata, "v": b.dstdata, "e": b.edata}
        frames[lt]["p"], frames[rt]["q"] = ld, rd
        pick = {"u": lambda t: t[s], "v": lambda t: t[d], "e": lambda t: t}
        b.apply_edges(getattr(fn, msg)("p", "q", "z"))
        gs._compare(b.edata["z"], gs.op64(op, pick[lt](l64), pick[rt](r64)), (ld, rd), (l64, r64), rng,
                    f"block {ns}x{nd} apply_edges {msg}")
    z = gc._randn(rng, E, 3)
    zd, z64 = _leaf(z, dev), _leaf(z, dtype=torch.float64)
    gs._compare(dgl.ops.edge_softmax(b, zd), gc.softmax64(d, nd, z64), (zd,), (z64,), rng, f"block {ns}x{nd} edge_softmax")


def check_to_block(dev):
    import dgl

    u, v = torch.tensor([7, 2, 7, 3, 5, 11, 3]), torch.tensor([5, 5, 2, 2, 9, 9, 5])
    g = dgl.graph((u, v), num_nodes=12).to(dev)
    b = dgl.to_block(g, torch.tensor([5, 2, 9]))
    assert b.srcdata[dgl.NID].tolist() == [5, 2, 9, 7, 3, 11] and b.dstdata[dgl.NID].tolist() == [5, 2, 9]
    bu, bv = b.edges()
    assert b.srcdata[dgl.NID][bu].tolist() == u.tolist() and b.dstdata[dgl.NID][bv].tolist() == v.tolist()
    assert b.edata[dgl.EID].tolist() == list(range(7)) and b.device.type == torch.device(dev).type
    d = dgl.to_block(g)  # default: the nodes with an in-edge, ascending
    assert d.dstdata[dgl.NID].tolist() == [2, 5, 9] and d.srcdata[dgl.NID].tolist() == [2, 5, 9, 7, 3, 11]
    with pytest.raises(NotImplementedError):
        dgl.to_block(g, include_dst_in_src=False)
    with pytest.raises(ValueError, match="duplicate"):
        dgl.to_block(g, torch.tensor([5, 2, 9, 5]))
    with pytest.raises(ValueError):
        dgl.to_block(g, torch.tensor([5, 2]))


@functools.lru_cache(maxsize=None)
def parent_case(n=200, e=1500, seed=3):
    from conftest import random_graph

    src, dst = random_graph(n, e, seed=seed, self_loop=True)
    return torch.from_numpy(src), torch.from_numpy(dst), n


def parent_graph(dev):
    import dgl

    src, dst, n = parent_case()
    return dgl.graph((src, dst), num_nodes=n).to(dev)


def check_sample_neighbors_shim(dev):
    import dgl

    g = parent_graph(dev)
    src, dst, n = parent_case()
    dgl.seed(5)
    nodes = torch.tensor([3, 50, 199, 7])
    sg = dgl.sampling.sample_neighbors(g, nodes, 4)
    assert not sg.is_block and sg.num_nodes() == n and sg.device.type == torch.device(dev).type
    su, sv = (t.cpu() for t in sg.edges())
    eid = sg.edata[dgl.EID].cpu()
    assert torch.equal(src[eid], su) and torch.equal(dst[eid], sv), "EID does not map to the parent's edges"
    deg = torch.bincount(dst, minlength=n)
    assert torch.equal(torch.bincount(sv, minlength=n)[nodes], deg[nodes].clamp(max=4)) and len(sv) == int(deg[nodes].clamp(max=4).sum())
    again = dgl.sampling.sample_neighbors(g, nodes, 4)
    assert not torch.equal(again.edata[dgl.EID].cpu(), eid), "the counter did not advance"
    dgl.seed(5)
    assert torch.equal(dgl.sampling.sample_neighbors(g, nodes, 4).edata[dgl.EID].cpu(), eid), "dgl.seed does not repeat"
    full = dgl.sampling.sample_neighbors(g, nodes, -1)
    assert len(full.edata[dgl.EID]) == int(deg[nodes].sum())
    for kw in ({"edge_dir": "out"}, {"replace": True}, {"prob": "p"}):
        with pytest.raises(NotImplementedError):
            dgl.sampling.sample_neighbors(g, nodes, 4, **kw)
    b = dgl.to_block(sg, nodes)
    assert torch.equal(b.edata[dgl.EID].cpu(), eid) and b.dstdata[dgl.NID].tolist() == nodes.tolist()


def check_blocks_valid(g_src, g_dst, inp, out, blocks):
    import dgl

    assert torch.equal(blocks[0].srcdata[dgl.NID].cpu(), inp.cpu()) and torch.equal(blocks[-1].dstdata[dgl.NID].cpu(), out.cpu())
    for a, b in zip(blocks, blocks[1:]):
        assert a.num_dst_nodes() == b.num_src_nodes()
        assert torch.equal(a.dstdata[dgl.NID], b.srcdata[dgl.NID])
    for b in blocks:
        assert b.is_block and torch.equal(b.srcdata[dgl.NID][:b.num_dst_nodes()], b.dstdata[dgl.NID])
        u, v = (t.cpu() for t in b.edges())
        eid = b.edata[dgl.EID].cpu()
        assert torch.equal(g_src[eid], b.srcdata[dgl.NID].cpu()[u]) and torch.equal(g_dst[eid], b.dstdata[dgl.NID].cpu()[v])
        assert len(torch.unique(b.srcdata[dgl.NID])) == b.num_src_nodes()


def check_loader(dev):
    import dgl
    from dgl.dataloading import DataLoader, MultiLayerNeighborSampler, NeighborSampler, NodeDataLoader

    assert MultiLayerNeighborSampler is NeighborSampler and NodeDataLoader is DataLoader
    g = parent_graph(dev)
    src, dst, n = parent_case()
    train = torch.from_numpy(np.random.default_rng(1).permutation(n)[:50].copy())
    sampler = NeighborSampler([3, 4])

    def run(seed, **kw):
        dgl.seed(seed)
        return list(DataLoader(g, train, sampler, batch_size=16, **kw))

    batches = run(0)
    assert len(batches) == 4 and [len(o) for _, o, _ in batches] == [16, 16, 16, 2]
    assert len(run(0, drop_last=True)) == 3 and len(DataLoader(g, train, sampler, batch_size=16, drop_last=True)) == 3
    for i, (inp, out, blocks) in enumerate(batches):
        assert torch.equal(out.cpu(), train[16 * i:16 * i + 16]) and len(blocks) == 2
        assert out.device.type == torch.device(dev).type
        check_blocks_valid(src, dst, inp, out, blocks)
        deg = torch.bincount(dst, minlength=n)
        assert torch.equal(blocks[1].in_degrees().cpu(), deg[out.cpu()].clamp(max=4))
        assert torch.equal(blocks[0].in_degrees().cpu(), deg[blocks[0].dstdata[dgl.NID].cpu()].clamp(max=3))
    key = lambda bs: [(b.edata[dgl.EID].tolist(), b.srcdata[dgl.NID].tolist()) for _, _, bl in bs for b in bl]  # noqa: E731
    assert key(run(0)) == key(batches), "the same dgl.seed gives other blocks"
    assert key(run(1)) != key(batches), "another dgl.seed gives the same blocks"
    gen = torch.Generator().manual_seed(3)
    shuffled = list(DataLoader(g, train, sampler, batch_size=16, shuffle=True, generator=gen))
    got = torch.cat([o.cpu() for _, o, _ in shuffled])
    assert not torch.equal(got, train) and torch.equal(got.sort().values, train.sort().values)
    with pytest.raises(NotImplementedError):
        DataLoader(g, train, sampler, batch_size=16, num_workers=2)


# ------------------------------------------------------------------ equivalence with the full graph
def full_blocks(dev, n_layers=2):
    import dgl
    from dgl.dataloading import MultiLayerFullNeighborSampler

    g = parent_graph(dev)
    seeds = torch.from_numpy(np.random.default_rng(4).permutation(parent_case()[2])[:17].copy())
    inp, out, blocks = MultiLayerFullNeighborSampler(n_layers).sample_blocks(g, seeds)
    check_blocks_valid(parent_case()[0], parent_case()[1], inp, out, blocks)
    return g, seeds, inp, blocks


def check_full_aggregations_bitwise(dev):
    """update_all alone on full-neighbour blocks: bitwise the parent's rows (max, sum, mean)."""
    import dgl
    import dgl.function as fn

    g, seeds, inp, blocks = full_blocks(dev)
    x = gc._randn(np.random.default_rng(6), g.num_nodes(), 10).to(dev)
    for reduce in ("max", "sum", "mean"):
        g.ndata["h"] = x
        g.update_all(fn.copy_u("h", "m"), getattr(fn, reduce)("m", "o"))
        for b in blocks:
            b.srcdata["h"] = x[b.srcdata[dgl.NID]]
            b.update_all(fn.copy_u("h", "m"), getattr(fn, reduce)("m", "o"))
            assert torch.equal(b.dstdata["o"], g.ndata["o"][b.dstdata[dgl.NID]]), f"{reduce}: not bitwise the parent's rows"


LAYERS = ["sage_pool", "sage_mean", "sage_gcn", "graphconv_right", "gat", "gat_res", "gatv2", "edgeconv"]


def make_layer(kind, fin, fout):
    import dgl.nn.pytorch as dnn

    torch.manual_seed(21)
    if kind.startswith("sage_"):
        return dnn.SAGEConv(fin, fout, kind[5:])
    if kind == "graphconv_right":
        return dnn.GraphConv(fin, fout, norm="right")
    if kind in ("gat", "gat_res"):
        return dnn.GATConv(fin, fout, 2, residual=kind == "gat_res")
    if kind == "gatv2":
        return dnn.GATv2Conv(fin, fout, 2, residual=True)
    return dnn.EdgeConv(fin, fout)


def check_layer_equivalence(dev, kind, pair):
    """Two layers on MultiLayerFullNeighborSampler(2) blocks, outputs at 17 seeds, against the
    same layers on the full graph: outputs, input and parameter gradients within 1e-5 of each
    tensor's magnitude. pair: the blocks get (feat_src, feat_dst), else one tensor. GraphConv
    runs with norm='right' (in-degrees, which full-neighbour blocks keep; a block's source
    out-degrees are not the parent's, so 'both' differs by design: check_graphconv_both)."""
    import dgl

    g, seeds, inp, blocks = full_blocks(dev)
    fin, hid = 12, 8
    heads = 2 if kind.startswith("gat") else 1
    l1, l2 = make_layer(kind, fin, hid).to(dev), make_layer(kind, hid * heads, 6).to(dev)
    x = gc._randn(np.random.default_rng(8), g.num_nodes(), fin)
    dz = None
    res = []
    for on_blocks in (False, True):
        for p in list(l1.parameters()) + list(l2.parameters()):
            p.grad = None
        xd = _leaf(x, dev)
        h = xd[inp.to(dev)] if on_blocks else xd
        for layer, b in zip((l1, l2), blocks):
            gr = b if on_blocks else g
            feat = (h, h[:b.num_dst_nodes()]) if (on_blocks and pair) else h
            h = torch.relu(layer(gr, feat)).flatten(1)
        out = h if on_blocks else h[seeds.to(dev)]
        if dz is None:
            dz = gc._randn(np.random.default_rng(9), *out.shape).to(dev)
        (out * dz).sum().backward()
        res.append((out.detach(), xd.grad, [p.grad.clone() for p in list(l1.parameters()) + list(l2.parameters())]))
    (o0, gx0, gp0), (o1, gx1, gp1) = res
    close(o1, o0, 1e-5, f"{kind} out")
    close(gx1, gx0, 1e-5, f"{kind} d feat")
    for k, (a, b) in enumerate(zip(gp1, gp0)):
        close(a, b, 1e-5, f"{kind} d param {k}")


def check_graphconv_both(dev, ns=37, nd=11):
    """GraphConv norm='both' on a block: source out-degrees and destination in-degrees of the
    block, each clamped at 1 (DGL 0.8), against float64 torch; SAGEConv 'gcn' divides by
    in-degree + 1 and adds the destination rows; a tuple in_feats on SAGEConv."""
    import dgl
    import dgl.nn.pytorch as dnn

    _, _, src, dst = rect(ns, nd)
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    b = dgl.create_block((s, d), ns, nd).to(dev)
    rng = np.random.default_rng(31)
    x = gc._randn(rng, ns, 6)
    torch.manual_seed(1)
    conv = dnn.GraphConv(6, 4, norm="both").to(dev)
    xd, x64 = _leaf(x, dev), _leaf(x, dtype=torch.float64)
    W, bias = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    od = torch.bincount(s, minlength=ns).clamp(min=1).double()
    idg = torch.bincount(d, minlength=nd).clamp(min=1).double()
    ref = torch.zeros(nd, 6, dtype=torch.float64).index_add_(0, d, (x64 * od[:, None] ** -0.5)[s])
    ref = (ref @ W) * idg[:, None] ** -0.5 + bias
    gs._compare(conv(b, xd), ref, (xd,), (x64,), rng, "block GraphConv both")
    sage = dnn.SAGEConv((6, 6), 4, "gcn").to(dev)
    xd, x64 = _leaf(x, dev), _leaf(x, dtype=torch.float64)
    Wn, bn = sage.fc_neigh.weight.detach().cpu().double(), sage.bias.detach().cpu().double()
    agg = torch.zeros(nd, 6, dtype=torch.float64).index_add_(0, d, x64[s])
    ref = ((agg + x64[:nd]) / (torch.bincount(d, minlength=nd).double()[:, None] + 1)) @ Wn.t() + bn
    gs._compare(sage(b, xd), ref, (xd,), (x64,), rng, "block SAGEConv gcn")
    pool = dnn.SAGEConv((6, 3), 4, "pool").to(dev)
    assert pool.fc_self.weight.shape == (4, 3) and pool.fc_pool.weight.shape == (6, 6)
    y = pool(b, (x.to(dev), gc._randn(rng, nd, 3).to(dev)))
    assert tuple(y.shape) == (nd, 4)
    with pytest.raises(NotImplementedError):
        dnn.SAGEConv(6, 4, "lstm")


def check_exports():
    from plagnn import _lib

    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.pg_version() == 13
