"""Shared by test_linkpred_cpu.py and test_gpu_linkpred.py: link-prediction mini-batches
(pg_edge_bits_update, pg_sample_count_excl / pg_sample_fill_excl, pg_edge_lookup,
pg_negative_sample) and the dgl shim built on them (exclude_edges / exclude_eids, find_edges,
has_edges_between, edge_ids, the negative samplers, as_edge_prediction_sampler, EdgeDataLoader),
each check parametrised by the device.

References
  exclusion   sampling with an exclusion set equals sampling the graph with those entries
              deleted and the edge ids kept: the expected result is the existing
              pg_sample_count_cpu / pg_sample_fill_cpu, called through the C ABI on the filtered
              in-CSR with its slot -> edge id map. Device and _excl_cpu twin equal it bitwise.
  lookup      a Python dictionary (u, v) -> smallest edge id.
  negatives   the CPU twin bitwise; the flags' meaning and the ranges in numpy; uniformity of
              the twin against five-sigma binomial bounds (derived, not measured).
  loader      the parent's COO: every rule is restated from (src, dst, reverse_eids).
  end to end  the CPU device, within 1e-5 of each tensor's magnitude (the bar of the block
              layer tests; the batches are identical index for index).
"""
import functools

import numpy as np
import pytest
import torch

import block_common as bc
from sddmm_common import close

FANOUTS = bc.FANOUTS
NEW_SYMBOLS = ["pg_edge_bits_update", "pg_sample_count_excl", "pg_sample_count_excl_workspace",
               "pg_sample_fill_excl", "pg_edge_lookup", "pg_negative_sample", "pg_edge_bits_update_cpu",
               "pg_sample_count_excl_cpu", "pg_sample_fill_excl_cpu", "pg_edge_lookup_cpu", "pg_negative_sample_cpu"]


def t64(a, dev="cpu"):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).to(dev)


# ------------------------------------------------------------------ 1. exclusion equals deletion
def deleted_reference(g, mask, seeds, fanout, seed):
    """pg_sample_count_cpu / pg_sample_fill_cpu on g's in-CSR without the entries whose edge id
    is set in `mask`, with the surviving entries' slot -> edge id map: (ptr, col, eid)."""
    from plagnn import _lib

    ptr, col, eid = g.fwd.ptr, g.fwd.col, g.eid.astype(np.int32)
    keep = ~mask[eid]
    rows = np.repeat(np.arange(g.num_dst), np.diff(ptr))
    fptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=g.num_dst))]).astype(np.int32)
    fcol, feid = np.ascontiguousarray(col[keep]), np.ascontiguousarray(eid[keep])
    s = _lib.PgCsr()
    s.n_rows, s.n_cols, s.nnz = g.num_dst, g.num_src, len(fcol)
    s.ptr, s.col = fptr.ctypes.data, (fcol.ctypes.data if len(fcol) else 0)
    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    out_ptr = np.zeros(len(seeds) + 1, np.int32)
    _lib.call("pg_sample_count_cpu", s, seeds.ctypes.data, len(seeds), fanout, out_ptr.ctypes.data)
    ocol, oeid = np.zeros(max(1, out_ptr[-1]), np.int32), np.zeros(max(1, out_ptr[-1]), np.int32)
    _lib.call("pg_sample_fill_cpu", s, feid.ctypes.data if len(feid) else 0, seeds.ctypes.data, len(seeds), fanout,
              seed, out_ptr.ctypes.data, ocol.ctypes.data, oeid.ctypes.data)
    return out_ptr, ocol[:out_ptr[-1]], oeid[:out_ptr[-1]]


def sample_excl(dev, g, seeds, fanout, seed, ids):
    """ops.sample_neighbors(exclude=) with the bits of `ids` set for the call and cleared after."""
    from plagnn import ops

    dg = g.on(dev)
    bits = dg.exclusion_bits()
    assert bits.dtype == torch.int32 and bits.numel() == max(1, (g.num_edges + 31) // 32) and not bits.any()
    ops.edge_bits_update(bits, g.num_edges, t64(ids), set=True)
    try:
        ptr, col, eid = ops.sample_neighbors(dg, t64(seeds), fanout, seed, exclude=bits)
    finally:
        ops.edge_bits_update(bits, g.num_edges, t64(ids), set=False)
    assert not bits.any(), "the bit set is not zero after clearing the ids that were set"
    assert ptr.dtype == col.dtype == eid.dtype == torch.int32 and ptr.device.type == torch.device(dev).type
    return ptr.cpu().numpy(), col.cpu().numpy(), eid.cpu().numpy()


def row_ids(g, row):
    return g.eid[g.fwd.ptr[row]:g.fwd.ptr[row + 1]]


def exclusion_sets(g, fanout):
    """name -> edge ids. Rows of sampler_graph(): 0..12 with in-degrees 0, 1, 4, 5, 6, 63, 64, 65,
    0, 200, cap, cap + 1, 2 cap + 37."""
    cap = bc.lds_keys()
    rng = np.random.default_rng(100 + fanout)
    E = g.num_edges
    deg = g.in_degrees()
    sets = {"none": np.zeros(0, np.int64), "random30": rng.permutation(E)[:int(0.3 * E)]}
    # every edge of rows 4 and 7; rows left with exactly fanout - 1, fanout, fanout + 1 entries
    parts = [row_ids(g, 4), row_ids(g, 7)]
    rows = [r for r in (12, 11, 10, 9, 6) if deg[r] >= fanout + 1][:3]
    for r, left in zip(rows, (fanout + 1, fanout, fanout - 1)):
        if left >= 0:
            parts.append(rng.permutation(row_ids(g, r))[:deg[r] - left])
    sets["rows_and_boundaries"] = np.concatenate(parts)
    # one edge out of the cap + 1 row; the hub row down to cap + 1 entries
    sets["lds_threshold"] = np.concatenate([rng.permutation(row_ids(g, 11))[:1],
                                            rng.permutation(row_ids(g, 12))[:deg[12] - (cap + 1)]])
    assert deg[11] == cap + 1 and deg[12] == 2 * cap + 37
    return sets


def check_exclusion(dev, fanout):
    g, k = bc.sampler_graph()
    rng = np.random.default_rng(fanout + 31)
    seeds = np.concatenate([np.arange(k), [k - 1, 3, 3, 650], rng.integers(0, g.num_dst, 40)])
    for name, ids in exclusion_sets(g, fanout).items():
        mask = np.zeros(g.num_edges, bool)
        mask[ids] = True
        want = deleted_reference(g, mask, seeds, fanout, 1234)
        got = sample_excl(dev, g, seeds, fanout, 1234, ids)
        twin = sample_excl("cpu", g, seeds, fanout, 1234, ids)
        for a, b, c, what in zip(got, want, twin, ("ptr", "col", "eid")):
            assert np.array_equal(a, b), f"fanout {fanout}, {name}: {what} differs from sampling the filtered graph"
            assert np.array_equal(c, b), f"fanout {fanout}, {name}: the twin's {what} differs from the filtered graph"
        assert not mask[got[2]].any(), f"fanout {fanout}, {name}: an excluded edge id was sampled"
        if name == "none":
            plain = bc.sample(dev, g, seeds, fanout, 1234)
            assert all(np.array_equal(a, b) for a, b in zip(got, plain)), "a zero bit set changes the sample"
        if name in ("random30", "rows_and_boundaries"):
            again = sample_excl(dev, g, seeds, fanout, 1234, ids)
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), f"{name}: two runs differ"
            perm = rng.permutation(len(seeds))
            moved = bc.rows_of(*sample_excl(dev, g, seeds[perm], fanout, 1234, ids))
            rows = bc.rows_of(*got)
            assert moved == [rows[p] for p in perm], f"{name}: a row depends on its place in seeds"


def check_exclusion_empty(dev):
    import plagnn

    g, _ = bc.sampler_graph()
    ptr, col, eid = sample_excl(dev, g, np.zeros(0, np.int64), 3, 1, [5, 6])
    assert list(ptr) == [0] and len(col) == 0 and len(eid) == 0
    e = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 9)
    ptr, col, eid = sample_excl(dev, e, np.arange(9), 4, 1, [])
    assert list(ptr) == [0] * 10 and len(col) == 0
    with pytest.raises(ValueError):
        sample_excl(dev, g, np.array([g.num_dst]), 2, 1, [1])
    assert not g.on(dev).exclusion_bits().any()


# ------------------------------------------------------------------ 2. bit sets
def check_bits(dev):
    from plagnn import ops

    n_ids = 1000
    bits = torch.zeros((n_ids + 31) // 32, dtype=torch.int32, device=dev)
    ids = np.array([0, 31, 32, 33, 999, 500, 500, 500, 31, 64], np.int64)
    ops.edge_bits_update(bits, n_ids, t64(ids), set=True)
    got = bits.cpu().numpy().view(np.uint32)
    want = np.zeros(len(got), np.uint32)
    for e in ids:
        want[e >> 5] |= np.uint32(1) << np.uint32(e & 31)
    assert np.array_equal(got, want), "set bits differ from bit (e & 31) of word (e >> 5)"
    ops.edge_bits_update(bits, n_ids, t64([500, 0]), set=False)
    want[500 >> 5] &= ~(np.uint32(1) << np.uint32(500 & 31))
    want[0] &= ~np.uint32(1)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want), "clearing touched other bits"
    ops.edge_bits_update(bits, n_ids, t64(ids), set=False)
    assert not bits.any(), "set then clear does not leave zeros"
    rng = np.random.default_rng(0)
    many = rng.integers(0, n_ids, 5000)
    ops.edge_bits_update(bits, n_ids, t64(many), set=True)
    assert int(sum(bin(int(w)).count("1") for w in bits.cpu().numpy().view(np.uint32))) == len(np.unique(many))
    ops.edge_bits_update(bits, n_ids, t64(many), set=False)
    assert not bits.any()
    for bad in ([n_ids], [-1], [3, n_ids, 4]):
        for set_ in (True, False):
            before = bits.clone()
            with pytest.raises(ValueError):
                ops.edge_bits_update(bits, n_ids, t64(bad), set=set_)
            good = [e for e in bad if 0 <= e < n_ids]
            ops.edge_bits_update(bits, n_ids, t64(good), set=False)
            assert torch.equal(bits, before) and not bits.any(), "an out-of-range id changed the bit set"
    ops.edge_bits_update(bits, n_ids, t64([]), set=True)
    assert not bits.any()


# ------------------------------------------------------------------ 3. edge lookup
def lookup_dict(src, dst):
    d = {}
    for e, (u, v) in enumerate(zip(src.tolist(), dst.tolist())):
        d.setdefault((u, v), e)
    return d


def lookup(dev, g, u, v):
    from plagnn import ops

    out = ops.edge_lookup(g.on(dev), t64(u), t64(v))
    assert out.dtype == torch.int32 and out.device.type == torch.device(dev).type
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def lookup_graph():
    """300 nodes: random edges with repeats (multi-edges), self-loops, a hub row of 700 in-edges
    at node 0 (more than one pass of the wave, duplicates of column 7 early and late), node 299
    without in-edges; shuffled, so slot -> edge id is not the identity."""
    import plagnn

    rng = np.random.default_rng(8)
    n = 300
    src = np.concatenate([rng.integers(0, n, 1500), np.arange(50), rng.integers(0, n, 698), [7, 7]])
    dst = np.concatenate([rng.integers(1, n - 1, 1500), np.arange(50), np.zeros(700, np.int64)])
    src, dst = np.concatenate([src, src[:200]]), np.concatenate([dst, dst[:200]])
    perm = rng.permutation(len(src))
    src, dst = src[perm].astype(np.int64), dst[perm].astype(np.int64)
    g = plagnn.CSRGraph(src, dst, n)
    assert g.in_degrees()[0] >= 700 and g.in_degrees()[n - 1] == 0
    return g, src, dst


def check_lookup(dev):
    import plagnn

    g, src, dst = lookup_graph()
    n = g.num_dst
    d = lookup_dict(src, dst)
    rng = np.random.default_rng(9)
    u = np.concatenate([src, rng.integers(0, n, 2000), [7, 5, 299, -1, 3, n, 2], np.arange(n)])
    v = np.concatenate([dst, rng.integers(0, n, 2000), [0, 299, 299, 4, -1, 2, n], np.arange(n)])
    want = np.array([d.get((a, b), -1) if 0 <= a < n and 0 <= b < n else -1 for a, b in zip(u.tolist(), v.tolist())],
                    np.int32)
    got = lookup(dev, g, u, v)
    assert np.array_equal(got, want), "edge ids differ from the dictionary's smallest id"
    assert np.array_equal(got, lookup("cpu", g, u, v)), "differs from pg_edge_lookup_cpu"
    assert (want[:len(src)] <= np.arange(len(src))).all() and (want[:len(src)] < np.arange(len(src))).any()
    assert len(lookup(dev, g, [], [])) == 0
    # a rectangular graph from a finished in-CSR (edge id = slot): 5 sources, 3 destinations
    r = plagnn.CSRGraph.from_in_csr([0, 2, 2, 5], [4, 1, 0, 4, 4], 5)
    ru, rv = [4, 1, 0, 4, 3, 4, 1, 4, 5], [0, 0, 2, 2, 2, 1, 2, 3, 0]
    assert lookup(dev, r, ru, rv).tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1]
    assert lookup("cpu", r, ru, rv).tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1]


# ------------------------------------------------------------------ 4. negatives
def negatives(dev, g, pos_src, pos_id, n_pos, k, seed, **kw):
    from plagnn import ops

    s, d, f = ops.negative_sample(g.on(dev), None if pos_src is None else t64(pos_src),
                                  None if pos_id is None else t64(pos_id), n_pos, k, seed, **kw)
    assert s.dtype == d.dtype == f.dtype == torch.int32 and s.numel() == d.numel() == n_pos * k
    return s.cpu().numpy(), d.cpu().numpy(), int(f[0])


def check_negatives(dev):
    import plagnn
    from plagnn import _lib

    g, src, dst = lookup_graph()
    n = g.num_dst
    edges = set(zip(src.tolist(), dst.tolist()))
    rng = np.random.default_rng(12)
    pos = rng.permutation(len(src))[:333]
    k = 3
    for pos_src in (src[pos], None):
        for kw in ({}, {"reject_edge": True}, {"reject_self": True}, {"reject_edge": True, "reject_self": True}):
            got = negatives(dev, g, pos_src, pos, len(pos), k, 77, tries=8, **kw)
            twin = negatives("cpu", g, pos_src, pos, len(pos), k, 77, tries=8, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(got[:2], twin[:2])) and got[2] == twin[2], \
                f"differs from pg_negative_sample_cpu ({kw}, pos_src {'given' if pos_src is not None else 'drawn'})"
            s, d, fails = got
            ok = s >= 0
            assert fails == int((~ok).sum()) and ((s < 0) == (d < 0)).all()
            assert (s[ok] < g.num_src).all() and (d[ok] < n).all() and (d[ok] >= 0).all()
            if pos_src is not None:
                assert np.array_equal(s[ok], np.repeat(pos_src, k)[ok]), "neg_src is not repeat(pos_src, k)"
            if kw.get("reject_edge"):
                assert not any((a, b) in edges for a, b in zip(s[ok].tolist(), d[ok].tolist())), "an edge came back"
            if kw.get("reject_self"):
                assert (s[ok] != d[ok]).all(), "a self-pair came back"
            if not kw:
                assert fails == 0
    # the draws are keyed by the positive's id: permuting the positives permutes the output
    base = negatives(dev, g, src[pos], pos, len(pos), k, 5, reject_edge=True)
    perm = rng.permutation(len(pos))
    moved = negatives(dev, g, src[pos][perm], pos[perm], len(pos), k, 5, reject_edge=True)
    for a, b in zip(base[:2], moved[:2]):
        assert np.array_equal(a.reshape(-1, k)[perm], b.reshape(-1, k)), "a slot depends on its place in the batch"
    other = negatives(dev, g, src[pos], pos, len(pos), k, 6, reject_edge=True)
    assert not np.array_equal(base[1], other[1]), "another seed gives the same negatives"
    noid = negatives(dev, g, src[pos], None, len(pos), k, 5, reject_edge=True)
    byidx = negatives(dev, g, src[pos], np.arange(len(pos)), len(pos), k, 5, reject_edge=True)
    assert np.array_equal(noid[1], byidx[1]), "pos_id = NULL is not the slot's index"
    # an out-of-range source fails its slots only
    bad = src[pos].copy()
    bad[4], bad[9] = n, -1
    s, d, fails = negatives(dev, g, bad, pos, len(pos), k, 5)
    assert fails == 2 * k and (s.reshape(-1, k)[[4, 9]] == -1).all() and (d.reshape(-1, k)[[4, 9]] == -1).all()
    assert (np.delete(s.reshape(-1, k), [4, 9], 0) >= 0).all()
    assert negatives(dev, g, None, None, 0, 2, 1)[2] == 0
    # the complete graph with self-loops: every attempt is an edge
    c = np.arange(6)
    full = plagnn.CSRGraph(np.repeat(c, 6), np.tile(c, 6), 6)
    s, d, fails = negatives(dev, full, np.arange(36) // 6, np.arange(36), 36, 2, 3, reject_edge=True, tries=64)
    assert fails == 72 and (s == -1).all() and (d == -1).all()
    s, d, fails = negatives(dev, full, None, None, 10, 2, 3, reject_edge=True)
    assert fails == 20 and (s == -1).all() and (d == -1).all()
    # rejected arguments: nothing is launched, the outputs are not touched
    for kw, kk in (({"tries": 0}, 2), ({"tries": 65}, 2), ({}, 0)):
        with pytest.raises(_lib.PlagnnError):
            negatives(dev, g, src[pos], pos, len(pos), kk, 1, **kw)


def check_negative_uniformity():
    """On the CPU twin (deterministic). One positive edge from source 0, 10 nodes, k = 1, seeds
    0 .. 3999. No flags: every destination's count within 400 +- 95 (five standard deviations of
    Binomial(4000, 0.1), sigma = 18.97). REJECT_EDGE with 0 -> {0 .. 4} edges, tries = 32: only
    5 .. 9 appear, each count within 800 +- 127 (five sigma of Binomial(4000, 0.2), sigma = 25.3),
    no failures (4000 * 2^-32 expected)."""
    import plagnn

    g = plagnn.CSRGraph(np.zeros(5, np.int64), np.arange(5), 10)
    plain, rej = np.zeros(10, np.int64), np.zeros(10, np.int64)
    fails = 0
    for seed in range(4000):
        s, d, f = negatives("cpu", g, [0], [0], 1, 1, seed, tries=1)
        assert s[0] == 0 and f == 0
        plain[d[0]] += 1
        s, d, f = negatives("cpu", g, [0], [0], 1, 1, seed, tries=32, reject_edge=True)
        fails += f
        if not f:
            rej[d[0]] += 1
    print("destination counts", plain.tolist(), "with rejection", rej.tolist(), "failures", fails)
    assert (np.abs(plain - 400) <= 95).all(), plain
    assert fails == 0 and (rej[:5] == 0).all(), (fails, rej)
    assert (np.abs(rej[5:] - 800) <= 127).all(), rej


# ------------------------------------------------------------------ 5. the shim's surface
def check_shim_queries(dev):
    import dgl

    g0, src, dst = lookup_graph()
    n = g0.num_dst
    g = dgl.graph((t64(src), t64(dst)), num_nodes=n).to(dev)
    d = lookup_dict(src, dst)
    eids = t64([0, 5, len(src) - 1, 5])
    u, v = g.find_edges(eids.to(dev))
    assert u.device.type == torch.device(dev).type and u.dtype == torch.int64
    assert torch.equal(u.cpu(), t64(src)[eids]) and torch.equal(v.cpu(), t64(dst)[eids])
    with pytest.raises(dgl.DGLError):
        g.find_edges(t64([len(src)]))
    rng = np.random.default_rng(3)
    qu, qv = np.concatenate([src[:300], rng.integers(0, n, 300)]), np.concatenate([dst[:300], rng.integers(0, n, 300)])
    has = g.has_edges_between(t64(qu), t64(qv))
    assert has.dtype == torch.bool and has.cpu().tolist() == [(a, b) in d for a, b in zip(qu.tolist(), qv.tolist())]
    assert bool(g.has_edges_between(int(src[0]), int(dst[0]))[0])
    got = g.edge_ids(t64(src), t64(dst))
    assert got.dtype == torch.int64 and got.cpu().tolist() == [d[(a, b)] for a, b in zip(src.tolist(), dst.tolist())]
    miss = next((a, b) for a in range(n) for b in range(n) if (a, b) not in d)
    with pytest.raises(dgl.DGLError):
        g.edge_ids(t64([src[0], miss[0]]), t64([dst[0], miss[1]]))
    with pytest.raises(NotImplementedError):
        g.edge_ids(t64(src[:2]), t64(dst[:2]), return_uv=True)
    with pytest.raises(dgl.DGLError):
        g.has_edges_between(t64([n]), t64([0]))


def check_shim_sampling(dev):
    import dgl

    g = bc.parent_graph(dev)
    src, dst, n = bc.parent_case()
    E = len(src)
    dgl.seed(5)
    nodes = torch.arange(0, n, 3)
    excl = t64(np.random.default_rng(2).permutation(E)[:E // 2])
    sg = dgl.sampling.sample_neighbors(g, nodes, 4, exclude_edges=excl)
    eid = sg.edata[dgl.EID].cpu()
    assert not np.isin(eid.numpy(), excl.numpy()).any(), "an excluded edge was sampled"
    su, sv = (t.cpu() for t in sg.edges())
    assert torch.equal(src[eid], su) and torch.equal(dst[eid], sv)
    left = torch.bincount(dst[np.setdiff1d(np.arange(E), excl.numpy())], minlength=n)
    assert torch.equal(torch.bincount(sv, minlength=n)[nodes], left[nodes].clamp(max=4)), \
        "a row does not hold min(remaining, fanout) edges"
    assert not g._device_graph(g.device).exclusion_bits().any()
    dgl.seed(5)
    plain = dgl.sampling.sample_neighbors(g, nodes, 4)
    dgl.seed(5)
    none = dgl.sampling.sample_neighbors(g, nodes, 4, exclude_edges=None)
    assert torch.equal(plain.edata[dgl.EID], none.edata[dgl.EID])
    # global negatives
    edges = set(zip(src.tolist(), dst.tolist()))
    for replace in (False, True):
        s, d = dgl.sampling.global_uniform_negative_sampling(g, 3000, replace=replace, redundancy=2.0)
        assert s.dtype == torch.int64 and s.device.type == torch.device(dev).type and 0 < len(s) == len(d) <= 3000
        pairs = list(zip(s.cpu().tolist(), d.cpu().tolist()))
        assert not any(p in edges for p in pairs) and all(a != b for a, b in pairs)
        assert all(0 <= a < n and 0 <= b < n for a, b in pairs)
        if not replace:
            assert len(set(pairs)) == len(pairs), "a pair is repeated with replace=False"
        else:
            assert len(set(pairs)) < len(pairs) == 3000  # 3000 draws over < 40000 pairs: repeats are certain
    s, d = dgl.sampling.global_uniform_negative_sampling(g, 500, exclude_self_loops=False, replace=True)
    assert len(s) == 500
    dgl.seed(9)
    a = dgl.sampling.global_uniform_negative_sampling(g, 100)
    dgl.seed(9)
    b = dgl.sampling.global_uniform_negative_sampling(g, 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "dgl.seed does not repeat the negatives"
    with pytest.raises(NotImplementedError):
        dgl.sampling.global_uniform_negative_sampling(g, 10, etype="e")


def check_negative_samplers(dev):
    import dgl
    from dgl.dataloading import negative_sampler as ns

    assert ns.PerSourceUniform is ns.Uniform
    g = bc.parent_graph(dev)
    src, dst, n = bc.parent_case()
    eids = t64([3, 77, 1200, 3])
    dgl.seed(1)
    s, d = ns.Uniform(4)(g, eids.to(dev))
    assert s.dtype == d.dtype == torch.int64 and s.device.type == torch.device(dev).type
    assert torch.equal(s.cpu(), src[eids].repeat_interleave(4)) and len(d) == 16
    assert bool(((d >= 0) & (d < n)).all())
    assert torch.equal(d[:4], d[12:]), "the same positive edge id in one call draws other negatives"
    s, d = ns.GlobalUniform(5)(g, eids)
    edges = set(zip(src.tolist(), dst.tolist()))
    pairs = list(zip(s.cpu().tolist(), d.cpu().tolist()))
    assert 0 < len(pairs) <= 20 and not any(p in edges for p in pairs) and len(set(pairs)) == len(pairs)
    with pytest.raises(ValueError):
        ns.Uniform(0)


def check_exports():
    import dgl
    from plagnn import _lib, ops

    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.pg_version() == 13 and _lib.ABI_VERSION == 13
    for name in ("edge_bits_update", "sample_neighbors", "edge_lookup", "negative_sample"):
        assert callable(getattr(ops, name))
    assert {"EdgeDataLoader", "as_edge_prediction_sampler", "negative_sampler"} <= set(dgl.dataloading.__all__)
    assert "global_uniform_negative_sampling" in dgl.sampling.__all__ and "DGLError" in dgl.__all__
    assert set(dgl.dataloading.negative_sampler.__all__) == {"Uniform", "PerSourceUniform", "GlobalUniform"}
    for mod in (dgl, dgl.sampling, dgl.dataloading, dgl.dataloading.negative_sampler):
        assert all(hasattr(mod, a) for a in mod.__all__)


# ------------------------------------------------------------------ 6. the edge loader
@functools.lru_cache(maxsize=None)
def bidirected_case():
    """block_common.parent_case() made bidirected: edge e + E is the reverse of edge e."""
    src, dst, n = bc.parent_case()
    E = len(src)
    rev = torch.cat([torch.arange(E) + E, torch.arange(E)])
    return torch.cat([src, dst]), torch.cat([dst, src]), n, rev


def bidirected_graph(dev):
    import dgl

    src, dst, n, _ = bidirected_case()
    return dgl.graph((src, dst), num_nodes=n).to(dev)


def loader_batches(dev, exclude, fanouts, seed=0, k=2, batch_size=64, n_seed_edges=200):
    import dgl
    from dgl.dataloading import EdgeDataLoader, NeighborSampler, negative_sampler

    src, dst, n, rev = bidirected_case()
    g = bidirected_graph(dev)
    train = t64(np.random.default_rng(1).permutation(len(src))[:n_seed_edges])
    dgl.seed(seed)
    loader = EdgeDataLoader(g, train, NeighborSampler(fanouts), exclude=exclude, reverse_eids=rev,
                            negative_sampler=negative_sampler.Uniform(k), batch_size=batch_size)
    return g, train, list(loader)


def batch_key(batches):
    import dgl

    key = []
    for inp, pg, ng, blocks in batches:
        key.append([inp.tolist(), pg.ndata[dgl.NID].tolist(), pg.edata[dgl.EID].tolist()] +
                   [t.tolist() for t in pg.edges()] + [t.tolist() for t in ng.edges()] +
                   [b.edata[dgl.EID].tolist() for b in blocks] + [b.srcdata[dgl.NID].tolist() for b in blocks])
    return key


def check_edge_loader(dev):
    import dgl
    from dgl.dataloading import DataLoader, NeighborSampler, as_edge_prediction_sampler

    src, dst, n, rev = bidirected_case()
    k = 2
    g, train, batches = loader_batches(dev, "reverse_id", [3, -1], k=k)
    assert [b[1].num_edges() for b in batches] == [64, 64, 64, 8]
    bits = g._device_graph(g.device).exclusion_bits()
    for i, (inp, pg, ng, blocks) in enumerate(batches):
        seeds = train[64 * i:64 * i + 64]
        assert pg.device.type == torch.device(dev).type and not pg.is_block and not ng.is_block
        nid = pg.ndata[dgl.NID].cpu()
        assert torch.equal(pg.edata[dgl.EID].cpu(), seeds), "pair_graph does not hold the seed edges in order"
        pu, pv = (t.cpu() for t in pg.edges())
        assert torch.equal(nid[pu], src[seeds]) and torch.equal(nid[pv], dst[seeds]), "pair_graph != find_edges(batch)"
        assert torch.equal(ng.ndata[dgl.NID].cpu(), nid) and ng.num_nodes() == pg.num_nodes() == len(nid)
        nu, nv = (t.cpu() for t in ng.edges())
        assert ng.num_edges() == k * len(seeds) and torch.equal(nid[nu], src[seeds].repeat_interleave(k))
        assert len(torch.unique(nid)) == len(nid), "the pair graphs' node set repeats a node"
        first = torch.cat([src[seeds], dst[seeds], nid[nu], nid[nv]]).tolist()
        assert nid.tolist() == list(dict.fromkeys(first)), "nodes are not in the order of first appearance"
        assert torch.equal(blocks[-1].dstdata[dgl.NID].cpu(), nid)
        bc.check_blocks_valid(src, dst, inp, nid, blocks)
        # fanout -1 on the last block: every in-edge of its destinations but the seeds and reverses
        out = torch.cat([seeds, rev[seeds]])
        got = blocks[-1].edata[dgl.EID].cpu().numpy()
        assert not np.isin(got, out.numpy()).any(), "a seed edge or its reverse is in the last block"
        all_in = np.nonzero(np.isin(dst.numpy(), nid.numpy()))[0]
        assert np.array_equal(np.sort(got), np.setdiff1d(all_in, out.numpy())), "another in-edge is missing"
        assert not np.isin(blocks[0].edata[dgl.EID].cpu().numpy(), out.numpy()).any(), "excluded in the first block"
        assert not bits.any(), "the exclusion bit set is not zero after a batch"
    # exclude=None: the seed edges and their reverses are there, so the exclusion above acted
    _, _, plain = loader_batches(dev, None, [3, -1], k=k)
    for i, (inp, pg, ng, blocks) in enumerate(plain):
        seeds = train[64 * i:64 * i + 64]
        got = blocks[-1].edata[dgl.EID].cpu().numpy()
        assert np.isin(torch.cat([seeds, rev[seeds]]).numpy(), got).all()
    _, _, own = loader_batches(dev, "self", [-1], k=k)
    got = own[0][3][-1].edata[dgl.EID].cpu().numpy()
    revs = np.setdiff1d(rev[train[:64]].numpy(), train[:64].numpy())  # a reverse may be a seed itself
    assert not np.isin(train[:64].numpy(), got).any() and len(revs) > 32 and np.isin(revs, got).all()
    # repeatability; without a negative sampler; other values of exclude
    assert batch_key(loader_batches(dev, "reverse_id", [3, -1])[2]) == batch_key(batches)
    assert batch_key(loader_batches(dev, "reverse_id", [3, -1], seed=1)[2]) != batch_key(batches)
    sampler = as_edge_prediction_sampler(NeighborSampler([2]), exclude="self")
    out3 = next(iter(DataLoader(g, train, sampler, batch_size=16)))
    assert len(out3) == 3 and out3[1].num_edges() == 16 and torch.equal(out3[2][-1].dstdata[dgl.NID], out3[1].ndata[dgl.NID])
    for bad in ("reverse_types", lambda e: e):
        with pytest.raises(NotImplementedError):
            as_edge_prediction_sampler(NeighborSampler([2]), exclude=bad)
    # the bits are cleared when the sampler raises mid-batch: a seed node outside the graph is
    # found by the first layer's count, after the bits were set; an exclude id outside the graph
    with pytest.raises(ValueError):
        NeighborSampler([2, 2]).sample_blocks(g, t64([1, n]), exclude_eids=t64([0, 1, 2]))
    assert not bits.any(), "bits left set after a failed batch"
    with pytest.raises(ValueError):
        NeighborSampler([2]).sample_blocks(g, t64([1, 2]), exclude_eids=t64([0, len(src)]))
    assert not bits.any(), "bits left set after a bad exclude id"


def check_edge_loader_equals_cpu(dev):
    a = loader_batches(dev, "reverse_id", [4, 5])[2]
    b = loader_batches("cpu", "reverse_id", [4, 5])[2]
    assert batch_key(a) == batch_key(b), "the device's batches differ from the CPU device's"


# ------------------------------------------------------------------ 7. end to end
def link_loss(dev, fin=12, hid=8):
    """Two SAGEConv('mean') layers on the blocks, u_dot_v on both pair graphs, BCE with logits:
    (loss, parameter gradients, feature gradient) over the first batch."""
    import dgl
    import dgl.function as fn
    import dgl.nn.pytorch as dnn
    import torch.nn.functional as F

    g, train, batches = loader_batches(dev, "reverse_id", [4, 5], k=3)
    inp, pg, ng, blocks = batches[0]
    torch.manual_seed(3)
    l1, l2 = dnn.SAGEConv(fin, hid, "mean").to(dev), dnn.SAGEConv(hid, hid, "mean").to(dev)
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((g.num_nodes(), fin)).astype(np.float32)).to(dev)
    x.requires_grad_(True)
    h = torch.relu(l1(blocks[0], x[inp]))
    h = l2(blocks[1], h)
    scores = []
    for gr in (pg, ng):
        with gr.local_scope():
            gr.ndata["h"] = h
            gr.apply_edges(fn.u_dot_v("h", "h", "s"))
            scores.append(gr.edata["s"].reshape(-1))
    logits = torch.cat(scores)
    labels = torch.cat([torch.ones_like(scores[0]), torch.zeros_like(scores[1])])
    loss = F.binary_cross_entropy_with_logits(logits, labels)
    loss.backward()
    grads = [p.grad for p in list(l1.parameters()) + list(l2.parameters())]
    return loss.detach(), grads, x.grad


def check_end_to_end(dev):
    loss, grads, gx = link_loss(dev)
    assert torch.isfinite(loss) and loss.item() > 0
    for i, gr in enumerate(grads + [gx]):
        assert gr is not None and torch.isfinite(gr).all() and gr.abs().max().item() > 0, f"gradient {i}"
    if torch.device(dev).type == "cpu":
        return
    loss0, grads0, gx0 = link_loss("cpu")
    close(loss.reshape(1), loss0.reshape(1), 1e-5, "link loss")
    close(gx, gx0, 1e-5, "link d feat")
    for i, (a, b) in enumerate(zip(grads, grads0)):
        close(a, b, 1e-5, f"link d param {i}")
