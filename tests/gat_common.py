"""Shared by test_gat_cpu.py and test_gpu_gat.py: float64 references for the multi-head
attention entry points (pg_edge_softmax_fwd / _bwd, pg_spmm_sum_heads, pg_sddmm_dot_heads),
computed with numpy / torch on the CPU from the edge list (the oracle is not involved), and the
checks both files run (on the CPU device and on the GPU).

Error bars, u = 2^-24 (each is derived, not fitted):
  softmax forward   |a - a64| <= (3 R + deg + 8) u a64 + 2^-126, R = the row's largest m - s for
                    that head: the rounding of s - m scaled by the exponent (also through a
                    scaled-exp2 fast path), deg additions of positive terms, a few ulps of exp
                    and the divide;
  softmax backward  |ds - ds64| <= u a ((deg + 5) S + 3 |da|) + 2^-126, S = sum_row |a da|;
  spmm_sum_heads    (deg + 2) u sum_k |A X| + 1e-30 per output element;
  sddmm_dot_heads   (Fh + 2) u sum_j |Dm X| + 1e-30 (tests/sddmm_common.py's bar with Fh for F).
Autograd through the shim: 1e-5 of each tensor's magnitude (sddmm_common.close).
"""
import functools

import numpy as np
import torch

import sddmm_common as sc
from sddmm_common import U, _leaf, close

TINY = 2.0 ** -126
# (H, Fh): generic paths (3, 5), (3, 100); a head that straddles the 256-column tile (4, 96)
SHAPES = [(1, 32), (2, 8), (3, 5), (4, 64), (8, 16), (4, 96), (3, 100)]
GRAPHS = ["random", "hub", "hub64"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """random: ~40 zero in-degree rows; hub: one split row at the default chunk; hub64: many
    pieces in both directions."""
    import plagnn
    from conftest import hub_graph, random_graph

    if name == "random":
        src, dst = random_graph(300, 600, self_loop=False)
        g = plagnn.CSRGraph(src, dst, 300)
        assert (g.in_degrees() == 0).sum() >= 20 and (g.in_degrees() == 1).any()
    elif name == "hub":
        src, dst = hub_graph(200, 300)
        g = plagnn.CSRGraph(src, dst, 200)
        assert g.fwd.n_merges == 1
    elif name == "hub_whole":  # the same hub row kept whole: one wave walks its 300+ entries
        src, dst = hub_graph(200, 300)
        g = plagnn.CSRGraph(src, dst, 200, chunk=1024)
        assert g.fwd.n_merges == 0 and g.fwd.max_deg > 256
    else:
        src, dst = hub_graph(64, 2000)
        g = plagnn.CSRGraph(src, dst, 64, chunk=64, chunk_bwd=64)
        assert g.fwd.n_merges >= 1 and g.bwd.n_merges >= 1 and g.fwd.n_slots > 8
    return g


def edge_buf(values, dev, pad):
    """(E, H) device tensor holding `values`; pad > 0: a view of an (E, H + pad) buffer whose
    other columns hold a sentinel."""
    E, H = values.shape
    if pad == 0:
        return sc.to_dev(values, dev), None
    buf = torch.full((E, H + pad), 7.0, dtype=torch.float32, device=dev)
    buf[:, :H] = sc.to_dev(values, dev)
    return buf[:, :H], buf


def empty_edge(E, H, dev, pad):
    buf = torch.full((E, H + pad), 7.0, dtype=torch.float32, device=dev)
    return buf[:, :H], buf


def pads_untouched(buf, H):
    return buf is None or bool((buf[:, H:] == 7.0).all())


def within(got, ref, bar, name, factor=1.0):
    sc.assert_within(got, ref, bar, name, factor=factor)


# ------------------------------------------------------------------ float64 references
def softmax_ref(g, s):
    """(a64, bar, in-degree per slot) of the edge softmax of float32 scores s (E, H), slot order."""
    dst, _, _ = sc.slot_edges(g)
    n, H = g.num_nodes, s.shape[1]
    s64 = s.astype(np.float64)
    m = np.full((n, H), -np.inf)
    np.maximum.at(m, dst, s64)
    ex = np.exp(s64 - m[dst])
    tot = np.zeros((n, H))
    np.add.at(tot, dst, ex)
    a64 = ex / tot[dst]
    gap = np.where(np.isfinite(s64), m[dst] - s64, 0.0)
    R = np.zeros((n, H))
    np.maximum.at(R, dst, gap)
    deg = np.diff(g.fwd.ptr).astype(np.float64)[dst][:, None]
    bar = (3 * R[dst] + deg + 8) * U * a64 + TINY
    return a64, bar, deg


def softmax_bwd_ref(g, a, da):
    dst, _, _ = sc.slot_edges(g)
    n, H = g.num_nodes, a.shape[1]
    a64, d64 = a.astype(np.float64), da.astype(np.float64)
    dot = np.zeros((n, H))
    np.add.at(dot, dst, a64 * d64)
    S = np.zeros((n, H))
    np.add.at(S, dst, np.abs(a64 * d64))
    deg = np.diff(g.fwd.ptr).astype(np.float64)[dst][:, None]
    ref = a64 * (d64 - dot[dst])
    bar = U * a64 * ((deg + 5) * S[dst] + 3 * np.abs(d64)) + TINY
    return ref, bar


def _rows(g, transpose):
    """(output row, gathered row, weight slot) of every entry of the in-CSR / the out-CSR."""
    if not transpose:
        dst, src, _ = sc.slot_edges(g)
        return dst, src, np.arange(len(src))
    ptr = g.bwd.ptr.astype(np.int64)
    row = np.repeat(np.arange(g.num_nodes), np.diff(ptr))
    return row, g.bwd.col.astype(np.int64), g.bwd.eslot.astype(np.int64)


def sum_heads_ref(g, A, X, H, transpose=False):
    row, colr, slot = _rows(g, transpose)
    n, F = X.shape
    Fh = F // H
    prod = torch.from_numpy(A.astype(np.float64)[slot])[:, :, None] * \
        torch.from_numpy(X.astype(np.float64)[colr]).reshape(-1, H, Fh)
    prod = prod.reshape(-1, F)
    r = torch.from_numpy(row)
    ref = torch.zeros(n, F, dtype=torch.float64).index_add_(0, r, prod)
    ab = torch.zeros(n, F, dtype=torch.float64).index_add_(0, r, prod.abs())
    deg = np.bincount(row, minlength=n).astype(np.float64)[:, None]
    return ref.numpy(), (deg + 2) * U * ab.numpy() + 1e-30, deg[:, 0]


def sddmm_heads_ref(g, D, X, H):
    dst, src, _ = sc.slot_edges(g)
    Fh = D.shape[1] // H
    prod = D.astype(np.float64)[dst].reshape(-1, H, Fh) * X.astype(np.float64)[src].reshape(-1, H, Fh)
    return prod.sum(-1), (Fh + 2) * U * np.abs(prod).sum(-1) + 1e-30


# ------------------------------------------------------------------ kernel-level checks
def scores(g, H, sigma, seed=0):
    return (np.random.default_rng(seed + 7 * H).standard_normal((g.num_edges, H)) * sigma).astype(np.float32)


def run_softmax_fwd(dev, g, s, name, pad=0):
    """ops.edge_softmax on `dev` within the forward bar; returns (a, a64, bar)."""
    from plagnn import ops

    H = s.shape[1]
    st, _ = edge_buf(s, dev, pad)
    out, obuf = empty_edge(g.num_edges, H, dev, pad)
    a = ops.edge_softmax(g.on(dev), st, out=out if pad else None)
    assert a.shape == (g.num_edges, H) and a.dtype == torch.float32
    assert pads_untouched(obuf, H)
    a64, bar, deg = softmax_ref(g, s)
    within(a, a64, bar, name)
    return a, a64, bar


def check_softmax_fwd(dev, gname, H, sigma, pad=0):
    g = graph(gname)
    s = scores(g, H, sigma)
    a, a64, bar = run_softmax_fwd(dev, g, s, f"softmax fwd {gname} H={H} sigma={sigma} pad={pad}", pad)
    an = a.detach().cpu().numpy().astype(np.float64)
    dst, _, _ = sc.slot_edges(g)
    deg = np.diff(g.fwd.ptr)
    rowsum = np.zeros((g.num_nodes, H))
    np.add.at(rowsum, dst, an)
    live = deg > 0
    err = np.abs(rowsum[live] - 1.0)
    lim = ((deg[live] + 8) * U)[:, None]
    print(f"row sums: max |sum - 1| / ((deg + 8) u) = {(err / lim).max():.3f}")
    assert (err <= lim).all()
    ones = deg[dst] == 1
    if gname == "random":
        assert ones.any()
    assert (an[ones] == 1.0).all(), "a degree-1 row gives exactly 1"


def check_softmax_shift(dev, gname, H):
    """Scores moved by 1000 stay finite and within the bar of the shifted float32 scores
    (exp overflows without the max subtraction)."""
    g = graph(gname)
    s = (scores(g, H, 10.0, seed=1) + np.float32(1000.0)).astype(np.float32)
    a, _, _ = run_softmax_fwd(dev, g, s, f"softmax shift {gname} H={H}")
    assert bool(torch.isfinite(a).all())


def check_softmax_neg_inf(dev, H):
    """A third of the hub row's scores at -inf: exact zeros there, the rest within the bar."""
    g = graph("hub")
    s = scores(g, H, 1.0, seed=2)
    dst, _, _ = sc.slot_edges(g)
    hub = np.flatnonzero(dst == 0)
    assert len(hub) > 256
    rng = np.random.default_rng(3)
    mask = np.zeros(s.shape, bool)
    mask[hub] = rng.random((len(hub), H)) < 1 / 3
    mask[hub[0]] = False  # every head keeps a finite score
    s[mask] = -np.inf
    a, _, _ = run_softmax_fwd(dev, g, s, f"softmax -inf H={H}")
    assert mask.sum() > 50 and bool((a.cpu()[torch.from_numpy(mask)] == 0).all())


def softmax_bwd_case(g, H, seed=4):
    a64, _, _ = softmax_ref(g, scores(g, H, 1.0, seed=seed))
    a = a64.astype(np.float32)
    da = np.random.default_rng(seed + H).standard_normal(a.shape).astype(np.float32)
    return a, da


def run_softmax_bwd(dev, g, a, da, name, pad=0):
    from plagnn import ops

    H = a.shape[1]
    at, _ = edge_buf(a, dev, pad)
    dt, _ = edge_buf(da, dev, pad)
    out, obuf = empty_edge(g.num_edges, H, dev, pad)
    ds = ops.edge_softmax_backward(g.on(dev), at, dt, out=out if pad else None)
    assert pads_untouched(obuf, H)
    ref, bar = softmax_bwd_ref(g, a, da)
    within(ds, ref, bar, name)
    return ds, ref, bar


def check_softmax_bwd(dev, gname, H, pad=0):
    g = graph(gname)
    a, da = softmax_bwd_case(g, H)
    run_softmax_bwd(dev, g, a, da, f"softmax bwd {gname} H={H} pad={pad}", pad)


def heads_case(g, H, Fh, seed=5):
    rng = np.random.default_rng(seed + 100 * H + Fh)
    A = rng.standard_normal((g.num_edges, H)).astype(np.float32)
    X = rng.standard_normal((g.num_nodes, H * Fh)).astype(np.float32)
    D = rng.standard_normal((g.num_nodes, H * Fh)).astype(np.float32)
    return A, X, D


def run_sum_heads(dev, g, A, X, H, transpose, name, pad=0):
    from plagnn import ops

    At, _ = edge_buf(A, dev, pad)
    out = ops.spmm_sum_heads(g.on(dev), At, sc.to_dev(X, dev), H, transpose=transpose)
    assert out.shape == X.shape and out.dtype == torch.float32
    ref, bar, deg = sum_heads_ref(g, A, X, H, transpose)
    within(out, ref, bar, name)
    assert bool((out.cpu()[torch.from_numpy(deg == 0)] == 0).all()), "rows without entries are exactly 0"
    return out, ref, bar


def check_sum_heads(dev, gname, H, Fh, transpose, pad=0):
    g = graph(gname)
    A, X, _ = heads_case(g, H, Fh)
    run_sum_heads(dev, g, A, X, H, transpose, f"sum_heads {gname} H={H} Fh={Fh} T={transpose} pad={pad}", pad)


def run_sddmm_heads(dev, g, D, X, H, name, pad=0):
    from plagnn import ops

    out, obuf = empty_edge(g.num_edges, H, dev, pad)
    de = ops.sddmm_dot_heads(g.on(dev), sc.to_dev(D, dev), sc.to_dev(X, dev), H, out=out if pad else None)
    assert de.shape == (g.num_edges, H) and de.dtype == torch.float32
    assert pads_untouched(obuf, H)
    ref, bar = sddmm_heads_ref(g, D, X, H)
    within(de, ref, bar, name)
    return de, ref, bar


def check_sddmm_heads(dev, gname, H, Fh, pad=0):
    g = graph(gname)
    _, X, D = heads_case(g, H, Fh)
    run_sddmm_heads(dev, g, D, X, H, f"sddmm_heads {gname} H={H} Fh={Fh} pad={pad}", pad)


def check_empty_shapes(dev):
    import plagnn
    from plagnn import ops

    g0 = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    dg = g0.on(dev)
    e = torch.zeros(0, 4, device=dev)
    assert ops.edge_softmax(dg, e).shape == (0, 4)
    assert ops.edge_softmax_backward(dg, e, e).shape == (0, 4)
    out = ops.spmm_sum_heads(dg, e, torch.ones(5, 8, device=dev), 4)
    assert out.shape == (5, 8) and not out.any()
    assert ops.sddmm_dot_heads(dg, torch.ones(5, 8, device=dev), torch.ones(5, 8, device=dev), 4).shape == (0, 4)


def check_rejections(dev):
    """H = 65 is rejected at the C-ABI; mismatched head counts in the wrappers."""
    import pytest
    from plagnn import _lib, ops

    g = graph("hub")
    dg = g.on(dev)
    E, n = g.num_edges, g.num_nodes
    s65 = torch.zeros(E, 65, device=dev)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.edge_softmax(dg, s65)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.edge_softmax_backward(dg, s65, s65)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.spmm_sum_heads(dg, s65, torch.zeros(n, 65, device=dev), 65)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.sddmm_dot_heads(dg, torch.zeros(n, 65, device=dev), torch.zeros(n, 65, device=dev), 65)
    with pytest.raises(ValueError):
        ops.spmm_sum_heads(dg, torch.zeros(E, 3, device=dev), torch.zeros(n, 8, device=dev), 4)
    with pytest.raises(ValueError):
        ops.spmm_sum_heads(dg, torch.zeros(E, 3, device=dev), torch.zeros(n, 8, device=dev), 3)
    with pytest.raises(ValueError):
        ops.edge_softmax_backward(dg, torch.zeros(E, 3, device=dev), torch.zeros(E, 4, device=dev))
    s = torch.zeros(E, 4, device=dev)
    with pytest.raises(_lib.PlagnnError, match="alias"):
        ops.edge_softmax(dg, s, out=s)


# ------------------------------------------------------------------ shim-level checks
def softmax64(dst, n, z):
    """Edge softmax over destinations of z (E, H) float64, differentiable."""
    H = z.shape[1]
    idx = dst[:, None].expand(-1, H)
    m = torch.full((n, H), -np.inf, dtype=torch.float64).scatter_reduce(0, idx, z.detach(), "amax")
    ex = torch.exp(z - m[dst])
    tot = torch.zeros(n, H, dtype=torch.float64).index_add_(0, dst, ex)
    return ex / tot[dst]


def shim_case(dev, seed=31, n=200, hub=300, self_loop=True):
    import dgl
    from conftest import hub_graph, random_graph

    src, dst = hub_graph(n, hub, seed=seed) if self_loop else random_graph(n, 2 * n, seed=seed, self_loop=False)
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).to(dev)
    return torch.from_numpy(src), torch.from_numpy(dst), g, np.random.default_rng(seed)


def _randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def check_shim_edge_softmax(dev, H=4):
    import dgl
    from dgl.nn.functional import edge_softmax

    assert dgl.ops.edge_softmax is edge_softmax
    src, dst, g, rng = shim_case(dev)
    E, n = len(src), g.num_nodes()
    z, dA = _randn(rng, E, H, 1) * 3, _randn(rng, E, H, 1)
    zd = _leaf(z, dev)
    a = edge_softmax(g, zd)
    assert a.shape == zd.shape and a.dtype == zd.dtype
    a.backward(dA.to(dev))
    z64 = _leaf(z.reshape(E, H), dtype=torch.float64)
    a64 = softmax64(dst, n, z64)
    a64.backward(dA.reshape(E, H).double())
    close(a.reshape(E, H), a64, 1e-5, "edge_softmax")
    close(zd.grad.reshape(E, H), z64.grad, 1e-5, "d logits")
    # a trailing shape of its own, and a 1-D tensor
    a2 = edge_softmax(g, z.reshape(E, 2, H // 2).to(dev))
    close(a2.reshape(E, H), a64, 1e-5, "edge_softmax (E, 2, H/2)")
    a1 = edge_softmax(g, z[:, 0, 0].to(dev))
    close(a1, a64[:, 0], 1e-5, "edge_softmax (E,)")


def check_shim_update_all_heads(dev, H=4, Fh=8):
    import dgl.function as fn

    src, dst, g, rng = shim_case(dev, seed=33)
    E, n = len(src), g.num_nodes()
    x, w, dZ = _randn(rng, n, H, Fh), _randn(rng, E, H, 1), _randn(rng, n, H, Fh)
    xd, wd = _leaf(x, dev), _leaf(w, dev)
    g.ndata["h"], g.edata["w"] = xd, wd
    g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "o"))
    y = g.ndata["o"]
    assert tuple(y.shape) == (n, H, Fh)
    y.backward(dZ.to(dev))
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    y64 = torch.zeros(n, H, Fh, dtype=torch.float64).index_add_(0, dst, x64[src] * w64)
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    close(wd.grad, w64.grad, 1e-5, "d edge weight")  # edge-id order: slots are a permutation of it


def check_shim_u_add_v(dev, shape=(4, 1), twice=False):
    import dgl.function as fn

    src, dst, g, rng = shim_case(dev, seed=35)
    E, n = len(src), g.num_nodes()
    a, b, dE = _randn(rng, n, *shape), _randn(rng, n, *shape), _randn(rng, E, *shape)
    grads = []
    for _ in range(2 if twice else 1):
        ad, bd = _leaf(a, dev), _leaf(b, dev)
        g.ndata["a"], g.ndata["b"] = ad, bd
        g.apply_edges(fn.u_add_v("a", "b", "e"))
        out = g.edata["e"]
        assert tuple(out.shape) == (E,) + tuple(shape)
        out.backward(dE.to(dev))
        grads.append((ad.grad, bd.grad))
    a64, b64 = _leaf(a, dtype=torch.float64), _leaf(b, dtype=torch.float64)
    ref = a64[src] + b64[dst]
    ref.backward(dE.double())
    assert torch.equal(out.detach().cpu(), (a[src] + b[dst])), "one float32 addition per element"
    close(grads[0][0], a64.grad, 1e-5, "d lhs")
    close(grads[0][1], b64.grad, 1e-5, "d rhs")
    if twice:
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), \
            "u_add_v gradients differ between two runs"


def check_shim_u_dot_v_heads(dev, H=4, Fh=8):
    import dgl.function as fn

    src, dst, g, rng = shim_case(dev, seed=37)
    E, n = len(src), g.num_nodes()
    a, b, dE = _randn(rng, n, H, Fh), _randn(rng, n, H, Fh), _randn(rng, E, H, 1)
    ad, bd = _leaf(a, dev), _leaf(b, dev)
    g.ndata["a"], g.ndata["b"] = ad, bd
    g.apply_edges(fn.u_dot_v("a", "b", "s"))
    out = g.edata["s"]
    assert tuple(out.shape) == (E, H, 1)
    out.backward(dE.to(dev))
    a64, b64 = _leaf(a, dtype=torch.float64), _leaf(b, dtype=torch.float64)
    prod = a64[src] * b64[dst]
    ref = prod.sum(-1, keepdim=True)
    ref.backward(dE.double())
    bar = (Fh + 2) * U * prod.detach().abs().sum(-1, keepdim=True).numpy() + 1e-30
    within(out, ref.detach().numpy(), bar, "u_dot_v heads")
    close(ad.grad, a64.grad, 1e-5, "d lhs")
    close(bd.grad, b64.grad, 1e-5, "d rhs")
    # 2-D operands keep their (E, 1) result
    g.ndata["a"], g.ndata["b"] = a.reshape(n, -1).to(dev), b.reshape(n, -1).to(dev)
    g.apply_edges(fn.u_dot_v("a", "b", "s"))
    assert tuple(g.edata["s"].shape) == (E, 1)


def gat64(src, dst, n, x, p, H, out, slope, residual):
    ft = (x @ p["fc.weight"].t()).view(n, H, out)
    el, er = (ft * p["attn_l"]).sum(-1), (ft * p["attn_r"]).sum(-1)
    a = softmax64(dst, n, torch.nn.functional.leaky_relu(el[src] + er[dst], slope))
    rst = torch.zeros(n, H, out, dtype=torch.float64).index_add_(0, dst, ft[src] * a[:, :, None])
    if residual:
        rst = rst + ((x @ p["res_fc.weight"].t()) if "res_fc.weight" in p else x).view(n, -1, out)
    return rst + p["bias"].view(1, H, out), a


def check_gatconv(dev, fin, fout, H, residual, self_loop=True):
    """GATConv against a pure-torch float64 GAT with the same parameters: output, attention,
    every parameter's and the input's gradient, the state_dict keys."""
    from dgl.nn.pytorch import GATConv

    src, dst, g, rng = shim_case(dev, seed=41, self_loop=self_loop)
    E, n = len(src), g.num_nodes()
    torch.manual_seed(7)
    conv = GATConv(fin, fout, H, residual=residual, allow_zero_in_degree=not self_loop).to(dev)
    keys = ["fc.weight", "attn_l", "attn_r", "bias"] + (["res_fc.weight"] if residual and fin != H * fout else [])
    assert sorted(conv.state_dict().keys()) == sorted(keys)
    assert conv.attn_l.shape == (1, H, fout) and conv.bias.shape == (H * fout,) and not conv.bias.any()
    with torch.no_grad():
        conv.bias.copy_(_randn(rng, H * fout) * 0.1)
    x, dZ, dA = _randn(rng, n, fin), _randn(rng, n, H, fout), _randn(rng, E, H, 1)
    xd = _leaf(x, dev)
    y, att = conv(g, xd, get_attention=True)
    assert tuple(y.shape) == (n, H, fout) and tuple(att.shape) == (E, H, 1)
    ((y * dZ.to(dev)).sum() + (att * dA.to(dev)).sum()).backward()
    assert "ft" not in g.ndata and "a" not in g.edata, "forward runs in a local scope"
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    x64 = _leaf(x, dtype=torch.float64)
    y64, a64 = gat64(src, dst, n, x64, p64, H, fout, 0.2, residual)
    ((y64 * dZ.double()).sum() + (a64 * dA.reshape(E, H).double()).sum()).backward()
    close(y, y64, 1e-5, "out")
    close(att.reshape(E, H), a64, 1e-5, "attention")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(v.grad, p64[k].grad, 1e-5, "d " + k)


def check_gatconv_zero_in_degree(dev):
    import pytest
    import plagnn
    from dgl.nn.pytorch import GATConv

    src, dst, g, rng = shim_case(dev, seed=41, self_loop=False)
    assert int((g.in_degrees() == 0).sum()) > 0
    conv = GATConv(6, 4, 2).to(dev)
    with pytest.raises(plagnn.PlagnnError, match="0-in-degree"):
        conv(g, torch.zeros(g.num_nodes(), 6, device=dev))
    with pytest.raises(NotImplementedError):
        GATConv((6, 6), 4, 2)
    with pytest.raises(NotImplementedError):
        x = torch.zeros(g.num_nodes(), 6, device=dev)
        GATConv(6, 4, 2, allow_zero_in_degree=True).to(dev)(g, (x, x))


def check_shim_rejections(dev):
    import pytest
    import dgl.function as fn
    from dgl.nn.functional import edge_softmax

    src, dst, g, rng = shim_case(dev, seed=43)
    E, n = len(src), g.num_nodes()
    z = torch.zeros(E, 4, 1, device=dev)
    with pytest.raises(NotImplementedError):
        edge_softmax(g, z, norm_by="src")
    with pytest.raises(NotImplementedError):
        edge_softmax(g, z[:10], eids=torch.arange(10))
    g.ndata["h"], g.edata["w"] = torch.zeros(n, 4, 8, device=dev), z
    for op in ("max", "mean"):
        with pytest.raises(NotImplementedError):
            g.update_all(fn.u_mul_e("h", "w", "m"), getattr(fn, op)("m", "o"))
    g.edata["w3"] = torch.zeros(E, 3, 1, device=dev)
    with pytest.raises(ValueError, match="heads"):
        g.update_all(fn.u_mul_e("h", "w3", "m"), fn.sum("m", "o"))
    g.ndata["h2"], g.edata["w2"] = torch.zeros(n, 32, device=dev), torch.zeros(E, 4, device=dev)
    with pytest.raises(NotImplementedError):  # (N, H*Fh) with (E, H) is not inferred
        g.update_all(fn.u_mul_e("h2", "w2", "m"), fn.sum("m", "o"))
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.copy_u("h", "m"))
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.u_add_v("h", "h", "e"), edges=torch.arange(3))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.u_add_v("h", "h", "m"), fn.sum("m", "o"))


def check_one_weight_per_edge_unchanged(dev, monkeypatch):
    """update_all(u_mul_e, sum) with one weight per edge ((E,), (E, 1) and (E, 1, 1) against
    (N, 1, F) features) still issues spmm_sum, never the heads entry."""
    import dgl.function as fn
    from plagnn import ops

    calls = {"sum": 0, "heads": 0}
    real_sum, real_heads = ops.spmm_sum, ops.spmm_sum_heads

    def spmm_sum(*a, **k):
        calls["sum"] += 1
        return real_sum(*a, **k)

    def spmm_sum_heads(*a, **k):
        calls["heads"] += 1
        return real_heads(*a, **k)

    monkeypatch.setattr(ops, "spmm_sum", spmm_sum)
    monkeypatch.setattr(ops, "spmm_sum_heads", spmm_sum_heads)
    src, dst, g, rng = shim_case(dev, seed=45)
    E, n = len(src), g.num_nodes()
    x, w = _randn(rng, n, 8), _randn(rng, E)
    ref = torch.zeros(n, 8, dtype=torch.float64).index_add_(0, dst, x.double()[src] * w.double()[:, None])
    for xs, ws in (((n, 8), (E,)), ((n, 8), (E, 1)), ((n, 1, 8), (E, 1, 1))):
        g.ndata["h"], g.edata["w"] = x.reshape(xs).to(dev), w.reshape(ws).to(dev)
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "o"))
        assert tuple(g.ndata["o"].shape) == xs
        close(g.ndata["o"].reshape(n, 8), ref, 1e-5, f"out {ws}")
    assert calls == {"sum": 3, "heads": 0}
