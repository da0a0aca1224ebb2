"""Shared by test_sddmm_cpu.py and test_gpu_sddmm.py: float64 references for pg_sddmm_dot and
for the edge-weight gradients of the weighted aggregations, computed here with numpy / torch
on the CPU from the edge list (the oracle is not involved), and the checks both files run
(on the CPU device and on the GPU).

Error bar of a per-edge dot product (any summation order): F products, each rounded once,
and F - 1 additions give |got - exact| <= F * u * sum_f |D[v,f] X[u,f]| to first order
(u = 2^-24), one more rounding for the mean's division, one spare:
    |got - ref64| <= (F + 2) * 2^-24 * sum_f |D[v,f] * X[u,f]| + 1e-30
with the sum over the matching f only in the max form, and both sides divided by the row's
entry count in the mean form. A wrong index, a lost tile or a double count is off by orders
of magnitude.

Autograd bar: 1e-5 of each tensor's magnitude (as tests/test_gpu_graphconv.py). For a max
aggregation the reference is formed from the engine's own argmax records (captured from its
ops.spmm_max call) and, for the relu in SAGEConv('pool'), from the engine's own sign
decisions, so near-ties cannot flip a winner between float32 and float64.
"""
import numpy as np
import torch

U = 2.0 ** -24


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def slot_edges(g):
    """(dst, src, position inside its row) of every in-CSR slot of a plagnn.CSRGraph."""
    ptr, col = g.fwd.ptr.astype(np.int64), g.fwd.col.astype(np.int64)
    deg = np.diff(ptr)
    dst = np.repeat(np.arange(g.num_nodes), deg)
    pos = np.arange(len(col)) - ptr[dst]
    return dst, col, pos


def argpos_np(argpos):
    """Records as int64, "none" (0xFFFF / -1) as -1."""
    a = argpos.detach().cpu().numpy()
    if a.dtype == np.int16:
        a = a.view(np.uint16).astype(np.int64)
        a[a == 0xFFFF] = -1
        return a
    return a.astype(np.int64)


def sddmm_ref(g, D, X, mean=False, argpos=None):
    """(float64 reference, error bar) of pg_sddmm_dot in slot order; D, X numpy float32."""
    dst, src, pos = slot_edges(g)
    F = D.shape[1]
    prod = D.astype(np.float64)[dst] * X.astype(np.float64)[src]
    if argpos is not None:
        prod = prod * (argpos_np(argpos)[dst] == pos[:, None])
    ref = prod.sum(1)
    bar = (F + 2) * U * np.abs(prod).sum(1) + 1e-30
    if mean:
        deg = np.diff(g.fwd.ptr).astype(np.float64)[dst]
        ref, bar = ref / deg, bar / deg
    return ref, bar


def assert_within(got, ref, bar, name, factor=1.0):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    err = np.abs(got - ref)
    worst = int(np.argmax(err - factor * bar)) if err.size else 0
    print(f"{name}: E = {err.size}, max err {err.max() if err.size else 0.0:.3e}, "
          f"max err / bar {(err / bar).max() if err.size else 0.0:.3f}")
    assert (err <= factor * bar).all(), f"{name}: slot {worst}: err {err[worst]:.3e} > bar {bar[worst]:.3e}"


def close(a, b, tol, name):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, f"{name}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item()
    print(f"{name}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= tol * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------ float64 aggregations
def agg_sum64(src, dst, n, X, w, mean=False):
    """sum_e w_e X[src_e] into dst_e (float64 torch, edge-id order); mean: / in-degree."""
    out = torch.zeros(n, X.shape[1], dtype=torch.float64).index_add_(0, dst, X[src] * w[:, None])
    if mean:
        deg = torch.bincount(dst, minlength=n).clamp(min=1).double()
        out = out / deg[:, None]
    return out


def agg_max64(g, X, w, argpos):
    """The max aggregation with the winners fixed by `argpos` (the engine's records):
    out[v,f] = w[e] X[src_e, f] for the recorded edge e, 0 where there is none. w in
    edge-id order; differentiable in X and w."""
    a = torch.from_numpy(argpos_np(argpos))
    ptr = torch.from_numpy(g.fwd.ptr.astype(np.int64))
    col = torch.from_numpy(g.fwd.col.astype(np.int64))
    eid = torch.from_numpy(g.eid.astype(np.int64))
    none = a < 0
    k = (ptr[:-1, None] + a).masked_fill(none, 0)
    vals = torch.gather(X, 0, col[k]) * w[eid[k]]
    return vals.masked_fill(none, 0.0)


class MaxRecorder:
    """Wraps plagnn.ops.spmm_max: keeps every call's (input, argpos, dead_none)."""

    def __init__(self, monkeypatch):
        from plagnn import ops

        self.calls = []
        real = ops.spmm_max

        def spmm_max(dg, X, ew_slots=None, out=None, argpos=None, dead_none=False):
            o, a = real(dg, X, ew_slots, out=out, argpos=argpos, dead_none=dead_none)
            self.calls.append((X.detach().clone(), a.detach().clone(), dead_none))
            return o, a

        monkeypatch.setattr(ops, "spmm_max", spmm_max)


def layer_case(dev, n, hub, seed, zero_w=False):
    """hub_graph on `dev` through the shim, with edge weights in (0.1, 1) (zero_w: a third
    of them exactly 0) that require grad."""
    import dgl
    from conftest import hub_graph

    src, dst = hub_graph(n, hub, seed=seed)  # self-loops appended: every in-degree >= 1
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 1.0, len(src)).astype(np.float32)
    if zero_w:
        w[rng.random(len(src)) < 1 / 3] = 0.0
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).to(dev)
    return torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(w), g, rng


def _leaf(t, dev=None, dtype=None):
    t = t.detach().clone()
    if dtype is not None:
        t = t.to(dtype)
    if dev is not None:
        t = t.to(dev)
    return t.requires_grad_(True)


# ------------------------------------------------------------------ the checks
def check_update_all(dev, reduce_op, monkeypatch, n=200, hub=300, F=24):
    """update_all(u_mul_e, sum | mean | max) -> ops.SumAggregate / ops.MaxAggregate."""
    import dgl.function as fn

    src, dst, w, g, rng = layer_case(dev, n, hub, seed=11)
    rec = MaxRecorder(monkeypatch)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    xd, wd = _leaf(x, dev), _leaf(w.reshape(-1, 1), dev)  # DGL's (E, 1) edge feature
    g.ndata["h"], g.edata["w"] = xd, wd
    g.update_all(fn.u_mul_e("h", "w", "m"), getattr(fn, reduce_op)("m", "o"))
    y = g.ndata["o"]
    y.backward(dZ.to(dev))
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    if reduce_op == "max":
        assert len(rec.calls) == 1 and not rec.calls[0][2]
        y64 = agg_max64(g._engine_graph(), x64, w64, rec.calls[0][1])
    else:
        y64 = agg_sum64(src, dst, n, x64, w64, mean=reduce_op == "mean")
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    assert wd.grad is not None and wd.grad.shape == wd.shape
    close(wd.grad.reshape(-1), w64.grad, 1e-5, "d edge weight")


def check_sage_pool(dev, fin, fout, monkeypatch, n=200, hub=300, zero_w=False):
    """SAGEConv('pool') with a learnable edge_weight -> ops.SagePool (all three paths by
    device and width). With zero_w, edges of weight 0 win zero maxima: their gradient
    dM * P is not zero and must survive (plain records, not dead-none)."""
    from dgl.nn.pytorch import SAGEConv

    src, dst, w, g, rng = layer_case(dev, n, hub, seed=13, zero_w=zero_w)
    rec = MaxRecorder(monkeypatch)
    torch.manual_seed(3)
    conv = SAGEConv(fin, fout, "pool").to(dev)
    with torch.no_grad():
        conv.fc_pool.bias.copy_(torch.from_numpy(rng.standard_normal(fin).astype(np.float32) * 0.1))
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(fout).astype(np.float32) * 0.1))
    x = torch.from_numpy(rng.standard_normal((n, fin)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, fout)).astype(np.float32))
    xd, wd = _leaf(x, dev), _leaf(w, dev)
    y = conv(g, xd, edge_weight=wd)
    y.backward(dZ.to(dev))
    assert len(rec.calls) == 1
    P_eng, argpos, dead_none = rec.calls[0]
    assert not dead_none, "a weight gradient needs plain argmax records"
    P_eng, argpos = P_eng[:, :fin].cpu(), argpos[:, :fin].cpu()

    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    z = x64 @ p64["fc_pool.weight"].t() + p64["fc_pool.bias"]
    P64 = z * (P_eng > 0)  # relu with the engine's own sign decisions
    M64 = agg_max64(g._engine_graph(), P64, w64, argpos)
    y64 = x64 @ p64["fc_self.weight"].t() + M64 @ p64["fc_neigh.weight"].t() + p64["bias"]
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(v.grad, p64[k].grad, 1e-5, "d " + k)
    assert wd.grad is not None
    close(wd.grad, w64.grad, 1e-5, "d edge weight")
    if zero_w:
        zero = w == 0
        live = zero & (w64.grad != 0)
        print(f"edges with w = 0: {int(zero.sum())}, of them with a non-zero gradient: {int(live.sum())}")
        assert int(live.sum()) >= 10, "the case must contain zero-weight winners"
        close(wd.grad.cpu()[zero], w64.grad[zero], 1e-5, "d edge weight where w = 0")


def check_sage_pool_frozen_weight_unchanged(dev, fin, monkeypatch, n=200, hub=300):
    """A weight that does not require grad: the GPU paths keep their dead-none records and
    return no weight gradient (the calls made before this feature)."""
    from dgl.nn.pytorch import SAGEConv

    src, dst, w, g, rng = layer_case(dev, n, hub, seed=13)
    rec = MaxRecorder(monkeypatch)
    conv = SAGEConv(fin, 8, "pool").to(dev)
    x = torch.from_numpy(rng.standard_normal((n, fin)).astype(np.float32)).to(dev).requires_grad_(True)
    wd = w.to(dev)
    conv(g, x, edge_weight=wd).sum().backward()
    assert len(rec.calls) == 1 and rec.calls[0][2] == (torch.device(dev).type == "cuda")
    assert wd.grad is None and x.grad is not None


def check_sage_mean(dev, fin, fout, n=200, hub=300):
    """SAGEConv('mean') with a learnable edge_weight (lin_before_mp by fin > fout)."""
    from dgl.nn.pytorch import SAGEConv

    src, dst, w, g, rng = layer_case(dev, n, hub, seed=17)
    torch.manual_seed(4)
    conv = SAGEConv(fin, fout, "mean").to(dev)
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(fout).astype(np.float32) * 0.1))
    x = torch.from_numpy(rng.standard_normal((n, fin)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, fout)).astype(np.float32))
    xd, wd = _leaf(x, dev), _leaf(w, dev)
    y = conv(g, xd, edge_weight=wd)
    y.backward(dZ.to(dev))
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    Wn, Ws = p64["fc_neigh.weight"], p64["fc_self.weight"]
    if fin > fout:
        hn = agg_sum64(src, dst, n, x64 @ Wn.t(), w64, mean=True)
    else:
        hn = agg_sum64(src, dst, n, x64, w64, mean=True) @ Wn.t()
    y64 = x64 @ Ws.t() + hn + p64["bias"]
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(v.grad, p64[k].grad, 1e-5, "d " + k)
    close(wd.grad, w64.grad, 1e-5, "d edge weight")


def check_graphconv(dev, fin, fout, n=200, hub=300):
    """GraphConv(norm='both', edge_weight=) with a learnable weight (product order by
    fin > fout)."""
    from dgl.nn.pytorch import GraphConv

    src, dst, w, g, rng = layer_case(dev, n, hub, seed=19)
    torch.manual_seed(5)
    conv = GraphConv(fin, fout, norm="both").to(dev)
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(fout).astype(np.float32) * 0.1))
    x = torch.from_numpy(rng.standard_normal((n, fin)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, fout)).astype(np.float32))
    xd, wd = _leaf(x, dev), _leaf(w, dev)
    y = conv(g, xd, edge_weight=wd)
    y.backward(dZ.to(dev))
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    outd = torch.bincount(src, minlength=n).clamp(min=1).double()
    ind = torch.bincount(dst, minlength=n).clamp(min=1).double()
    h = x64 * outd.pow(-0.5)[:, None]
    if fin > fout:
        r = agg_sum64(src, dst, n, h @ p64["weight"], w64)
    else:
        r = agg_sum64(src, dst, n, h, w64) @ p64["weight"]
    y64 = r * ind.pow(-0.5)[:, None] + p64["bias"]
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(v.grad, p64[k].grad, 1e-5, "d " + k)
    close(wd.grad, w64.grad, 1e-5, "d edge weight")


def check_aggregate_ops(dev, kind, monkeypatch, n=200, hub=300, F=24):
    """ops.SumAggregate (sum, mean) and ops.MaxAggregate called directly with slot-order
    weights that require grad."""
    import plagnn
    from conftest import hub_graph
    from plagnn import ops

    src, dst = hub_graph(n, hub, seed=23)
    g = plagnn.CSRGraph(src, dst, n)
    dg = g.on(dev)
    rng = np.random.default_rng(23)
    w = torch.from_numpy(rng.uniform(0.1, 1.0, len(src)).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    xd, wd = _leaf(x, dev), _leaf(w, dev)
    ews = dg.edge_weight_slots(wd)
    assert ews.requires_grad, "the slot-order weights stay attached to the graph"
    rec = MaxRecorder(monkeypatch)
    if kind == "max":
        y = ops.MaxAggregate.apply(xd, dg, ews)
    else:
        y = ops.SumAggregate.apply(xd, dg, ews, kind == "mean")
    y.backward(dZ.to(dev))
    x64, w64 = _leaf(x, dtype=torch.float64), _leaf(w, dtype=torch.float64)
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    y64 = agg_max64(g, x64, w64, rec.calls[0][1]) if kind == "max" else agg_sum64(s, d, n, x64, w64, kind == "mean")
    y64.backward(dZ.double())
    close(y, y64, 1e-5, "out")
    close(xd.grad, x64.grad, 1e-5, "d feat")
    close(wd.grad, w64.grad, 1e-5, "d edge weight")


def check_u_dot_v(dev, F=12):
    """apply_edges(u_dot_v): values in edge-id order, shape (E, 1), and both input gradients,
    on a multigraph with duplicate edges and a zero-in-degree node."""
    import dgl
    import dgl.function as fn

    n = 40
    rng = np.random.default_rng(29)
    src = rng.integers(0, n, 300)
    dst = rng.integers(0, n - 1, 300)  # node n - 1 has no in-edge
    src = np.concatenate([src, src[:50], [5, 5, 5]])  # duplicates
    dst = np.concatenate([dst, dst[:50], [7, 7, 7]])
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    g = dgl.graph((s, d), num_nodes=n).to(dev)
    assert int(g.in_degrees()[n - 1]) == 0
    a = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    dE = torch.from_numpy(rng.standard_normal((len(src), 1)).astype(np.float32))
    ad, bd = _leaf(a, dev), _leaf(b, dev)
    g.ndata["a"], g.ndata["b"] = ad, bd
    g.apply_edges(fn.u_dot_v("a", "b", "s"))
    out = g.edata["s"]
    assert tuple(out.shape) == (len(src), 1)
    out.backward(dE.to(dev))
    a64, b64 = _leaf(a, dtype=torch.float64), _leaf(b, dtype=torch.float64)
    prod = a64[s] * b64[d]
    ref = prod.sum(1, keepdim=True)
    ref.backward(dE.double())
    bar = (F + 2) * U * prod.detach().abs().sum(1, keepdim=True).numpy() + 1e-30
    assert_within(out, ref.detach().numpy(), bar, "u_dot_v")
    close(ad.grad, a64.grad, 1e-5, "d lhs")
    close(bd.grad, b64.grad, 1e-5, "d rhs")
