"""Shared by test_gatv2_cpu.py and test_gpu_gatv2.py: float64 references for the fused GATv2
score entry points (pg_gatv2_score, pg_gatv2_bwd and their _cpu twins), computed with numpy from
the CSR entry lists (never from the code under test), and the checks both files run (on the CPU
device and on the GPU). slope64 = float(np.float32(slope)) throughout.

    s[k,h]     = sum_d attn[h,d] lrelu(t_k[h,d]),  t_k = XL[src_k] + XR[dst_k]
    g[k,h,d]   = ds[k,h] attn[h,d] lrelu'(t_k[h,d])      (lrelu'(0) = slope)
    dXR[v]     = sum over the in-entries of v of g,  dXL[u] = sum over the out-entries of u of g
    dattn[h,d] = sum_k ds[k,h] lrelu(t_k[h,d])

Two input families.
  Grid (bitwise): node values are multiples of 0.25 in [-2, 2], attn and ds are in {+-0.5, +-1,
    +-2}, slope = 0.25: every term is a multiple of 1/64 of magnitude <= 8, so sums over
    Fh <= 256, over hub64's longest row and over all edges of these graphs stay far below 2^24
    units and are exact in any order. Scores and all three gradients must equal the float64
    reference bit for bit. Exactly-zero pre-activations are frequent, which pins the x > 0
    convention; hub / hub64 pin the split-row combining, Fh = 100 the heads that straddle tiles.
  Gaussian, u = 2^-24 (each bar follows from the operation count, none is fitted):
    forward   |got - ref| <= (Fh + 3) u sum_d |attn_d lrelu(t_d)| + 1e-30: three roundings per
              term (the add, the slope multiply, the attn multiply) and Fh - 1 additions in any
              grouping. lrelu is positively homogeneous, so the add's rounding scales with the
              term, and the f32 sum of two f32 values has the sign of the exact sum, so no
              activation decision can flip.
    dXL, dXR  (deg + 4) u sum_k |g_k| + 1e-30, deg the row's entry count in that direction. The
              kernels factor attn out of the row sum (dX = attn * sum ds lrelu'): one rounding
              for ds * slope, deg - 1 additions and one final multiply, deg + 1 in all, within
              the count above.
    dattn     (E + 3) u sum_k |ds lrelu(t)| + 1e-30: three roundings per term, E - 1 additions.
Autograd through ops.GATv2Score and dgl.nn.pytorch.GATv2Conv: 1e-5 of each tensor's magnitude
(sddmm_common.close) against a float64 torch composition of the formula.
"""
import functools

import numpy as np
import torch

import gat_common as gc
import sddmm_common as sc
from sddmm_common import U, _leaf, close

# scalar path: (1, 1), (1, 5), (2, 3); vector path: the rest; H*Fh past one 256-column tile:
# (4, 100), (3, 100), (2, 256); heads that straddle a tile boundary: Fh = 100; the head limit
SHAPES = [(1, 1), (1, 5), (3, 4), (2, 3), (8, 8), (4, 64), (4, 100), (3, 100), (64, 4), (2, 256)]
GRAPHS = gc.GRAPHS
FAMILIES = ["grid", "gauss"]
PM = np.array([-2, -1, -0.5, 0.5, 1, 2], np.float32)


@functools.lru_cache(maxsize=None)
def case(gname, H, Fh, family):
    """Inputs (float32 numpy) and float64 references with their bars, computed once per case and
    never modified: dict with xl, xr, attn, ds, slope, and (ref, bar) under s, dxl, dxr, dattn."""
    g = gc.graph(gname)
    n, E, F = g.num_nodes, g.num_edges, H * Fh
    rng = np.random.default_rng(1000 * H + Fh + (0 if family == "grid" else 500000))
    if family == "grid":
        xl = (rng.integers(-8, 9, (n, F)) / 4.0).astype(np.float32)
        xr = (rng.integers(-8, 9, (n, F)) / 4.0).astype(np.float32)
        attn, ds, slope = rng.choice(PM, F), rng.choice(PM, (E, H)), 0.25
    else:
        xl = rng.standard_normal((n, F)).astype(np.float32)
        xr = rng.standard_normal((n, F)).astype(np.float32)
        attn = rng.standard_normal(F).astype(np.float32)
        ds, slope = rng.standard_normal((E, H)).astype(np.float32), 0.2
    slope64 = float(np.float32(slope))
    dst, src, _ = sc.slot_edges(g)
    t = xl.astype(np.float64)[src] + xr.astype(np.float64)[dst]          # (E, F)
    act = np.where(t > 0, t, slope64 * t)
    term = attn.astype(np.float64) * act
    s_ref = term.reshape(E, H, Fh).sum(-1)
    s_bar = (Fh + 3) * U * np.abs(term).reshape(E, H, Fh).sum(-1) + 1e-30
    dsx = np.repeat(ds.astype(np.float64), Fh, axis=1)                    # (E, F)
    gk = dsx * attn.astype(np.float64) * np.where(t > 0, 1.0, slope64)
    out = {"g": g, "H": H, "Fh": Fh, "xl": xl, "xr": xr, "attn": attn, "ds": ds, "slope": slope,
           "s": (s_ref, s_bar)}
    for key, row in (("dxr", dst), ("dxl", src)):
        ref, ab = np.zeros((n, F)), np.zeros((n, F))
        np.add.at(ref, row, gk)
        np.add.at(ab, row, np.abs(gk))
        deg = np.bincount(row, minlength=n).astype(np.float64)[:, None]
        out[key] = (ref, (deg + 4) * U * ab + 1e-30)
    da = dsx * act
    out["dattn"] = (da.sum(0), (E + 3) * U * np.abs(da).sum(0) + 1e-30)
    if family == "grid":
        assert (t == 0).sum() > 0, "the grid must hit exactly-zero pre-activations"
    return out


def node_buf(values, dev, pad):
    """(n, F) device tensor holding `values`; pad > 0: a view of an (n, F + pad) buffer whose
    other columns hold a sentinel."""
    n, F = values.shape
    if pad == 0:
        return sc.to_dev(values, dev), None
    buf = torch.full((n, F + pad), 7.0, dtype=torch.float32, device=dev)
    buf[:, :F] = sc.to_dev(values, dev)
    return buf[:, :F], buf


def _check(got, ref_bar, family, name, factor=1.0):
    ref, bar = ref_bar
    if family == "grid":
        g64 = got.detach().cpu().numpy().astype(np.float64)
        assert g64.shape == ref.shape, f"{name}: shape {g64.shape} vs {ref.shape}"
        bad = int((g64 != ref).sum())
        print(f"{name}: {g64.size} values, {bad} differ from the float64 reference")
        assert bad == 0, f"{name}: {bad} values are not bitwise equal to the float64 reference"
    else:
        gc.within(got, ref, bar, name, factor=factor)


def run_score(dev, c, pad=0, epad=0):
    from plagnn import ops

    g, H = c["g"], c["H"]
    xl, _ = node_buf(c["xl"], dev, pad)
    xr, _ = node_buf(c["xr"], dev, pad)
    out, obuf = gc.empty_edge(g.num_edges, H, dev, epad)
    s = ops.gatv2_score(g.on(dev), xl, xr, sc.to_dev(c["attn"], dev), H, c["slope"], out=out if epad else None)
    assert s.shape == (g.num_edges, H) and s.dtype == torch.float32
    assert gc.pads_untouched(obuf, H)
    return s


def run_bwd(dev, c, transpose, want_dx=True, want_da=True, pad=0, epad=0):
    """One backward pass; returns (dx or None, dattn or None)."""
    from plagnn import ops

    g, H, F = c["g"], c["H"], c["H"] * c["Fh"]
    xl, _ = node_buf(c["xl"], dev, pad)
    xr, _ = node_buf(c["xr"], dev, pad)
    ds, _ = gc.edge_buf(c["ds"], dev, epad)
    da = torch.full((F,), 7.0, dtype=torch.float32, device=dev) if want_da else None
    dxv, dxbuf = (None, None)
    if want_dx and pad:
        dxbuf = torch.full((g.num_nodes, F + pad), 7.0, dtype=torch.float32, device=dev)
        dxv = dxbuf[:, :F]
    dx = ops.gatv2_backward_pass(g.on(dev), ds, xl, xr, sc.to_dev(c["attn"], dev), H, c["slope"], transpose,
                                 want_dx, da, dx=dxv)
    assert (dx is None) == (not want_dx)
    if dxbuf is not None:
        assert bool((dxbuf[:, F:] == 7.0).all()), "padding columns of dX were written"
    return dx, da


def check_kernels(dev, gname, H, Fh, family, pad=0, epad=0):
    """Forward and both directions of the backward (dattn from each) against the references."""
    c = case(gname, H, Fh, family)
    tag = f"{gname} H={H} Fh={Fh} {family} pad={pad}"
    _check(run_score(dev, c, pad, epad), c["s"], family, "score " + tag)
    for transpose, key in ((False, "dxr"), (True, "dxl")):
        dx, da = run_bwd(dev, c, transpose, pad=pad, epad=epad)
        _check(dx, c[key], family, f"{key} {tag}")
        _check(da, c["dattn"], family, f"dattn (with {key}) {tag}")


def check_outputs_alone(dev, gname="hub", H=4, Fh=64):
    """Each gradient output may be NULL on its own: dX without dattn, dattn without dX (both
    directions), and neither (nothing is written)."""
    for family in FAMILIES:
        c = case(gname, H, Fh, family)
        for transpose, key in ((False, "dxr"), (True, "dxl")):
            dx, da = run_bwd(dev, c, transpose, want_dx=True, want_da=False)
            assert da is None
            _check(dx, c[key], family, f"{key} alone")
            dx, da = run_bwd(dev, c, transpose, want_dx=False, want_da=True)
            _check(da, c["dattn"], family, f"dattn alone (transpose={transpose})")
            dx, da = run_bwd(dev, c, transpose, want_dx=False, want_da=False)
            assert dx is None and da is None


def check_rejections(dev):
    """H = 65 and a NULL required buffer are rejected with an error string."""
    import pytest
    from plagnn import _lib, ops

    g = gc.graph("hub")
    dg = g.on(dev)
    E, n = g.num_edges, g.num_nodes
    x65, a65 = torch.zeros(n, 65, device=dev), torch.zeros(65, device=dev)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.gatv2_score(dg, x65, x65.clone(), a65, 65, 0.2)
    with pytest.raises(_lib.PlagnnError, match="heads"):
        ops.gatv2_backward_pass(dg, torch.zeros(E, 65, device=dev), x65, x65.clone(), a65, 65, 0.2, False, True)
    cuda = dg.is_cuda
    st = (_lib.stream_handle(torch.device(dev)),) if cuda else ()
    x, a, s = torch.zeros(n, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(E, 4, device=dev)
    gs = dg.fwd.struct(None)
    P = _lib.ptr
    for miss in range(4):  # XL, XR, attn, s
        bufs = [P(x), P(x), P(a), P(s)]
        bufs[miss] = 0
        with pytest.raises(_lib.PlagnnError, match="NULL buffer"):
            _lib.call("pg_gatv2_score" if cuda else "pg_gatv2_score_cpu", gs, bufs[0], 8, bufs[1], 8, bufs[2], 4, 2,
                      0.2, bufs[3], 4, *st)
    dx = torch.zeros(n, 8, device=dev)
    ws_n = _lib.lib().pg_gatv2_bwd_workspace(gs, 4, 2, 0) if cuda else 0
    ws = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=dev)
    for miss in range(4):  # ds, Xown, Xgat, attn
        bufs = [P(s), P(x), P(x), P(a)]
        bufs[miss] = 0
        tail = (P(ws), ws_n, *st) if cuda else ()
        with pytest.raises(_lib.PlagnnError, match="NULL buffer"):
            _lib.call("pg_gatv2_bwd" if cuda else "pg_gatv2_bwd_cpu", gs, bufs[0], 4, bufs[1], 8, bufs[2], 8, bufs[3],
                      4, 2, 0.2, P(dx), 8, 0, *tail)
    with pytest.raises(ValueError):  # wrappers: shapes that do not fit
        ops.gatv2_score(dg, x, x.clone(), torch.zeros(7, device=dev), 4, 0.2)
    with pytest.raises(ValueError):
        ops.gatv2_score(dg, x, torch.zeros(n, 12, device=dev), a, 4, 0.2)
    with pytest.raises(ValueError):
        ops.gatv2_backward_pass(dg, torch.zeros(E, 3, device=dev), x, x.clone(), a, 4, 0.2, False, True)


def check_empty_shapes(dev):
    """nnz == 0 succeeds: no scores, zero gradients."""
    import plagnn
    from plagnn import ops

    g0 = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    dg = g0.on(dev)
    x, a = torch.ones(5, 8, device=dev), torch.ones(8, device=dev)
    assert ops.gatv2_score(dg, x, x.clone(), a, 4, 0.2).shape == (0, 4)
    ds = torch.zeros(0, 4, device=dev)
    for transpose in (False, True):
        da = torch.full((8,), 7.0, device=dev)
        dx = ops.gatv2_backward_pass(dg, ds, x, x.clone(), a, 4, 0.2, transpose, True, da)
        assert dx.shape == (5, 8) and not dx.any() and not da.any()


# ------------------------------------------------------------------ autograd
def score64(src, dst, xl, xr, attn, slope):
    """(E, H) float64 scores of (n, H, Fh) projections and (1, H, Fh) attn, in the order of
    (src, dst)."""
    return (torch.nn.functional.leaky_relu(xl[src] + xr[dst], slope) * attn).sum(-1)


def count_dattn_passes(monkeypatch):
    """Wraps ops.gatv2_backward_pass; returns the dict it counts in: passes, and passes that
    were handed a dattn buffer."""
    from plagnn import ops

    calls = {"passes": 0, "dattn": 0}
    real = ops.gatv2_backward_pass

    def wrapped(dg, ds, xl, xr, attn, H, slope, transpose, want_dx, dattn=None, dx=None):
        calls["passes"] += 1
        calls["dattn"] += dattn is not None
        return real(dg, ds, xl, xr, attn, H, slope, transpose, want_dx, dattn, dx=dx)

    monkeypatch.setattr(ops, "gatv2_backward_pass", wrapped)
    return calls


def check_autograd_score(dev, monkeypatch, gname="hub", H=3, Fh=20, slope=0.2):
    """ops.GATv2Score against the float64 composition: scores and the three gradients; with
    attn frozen no pass computes dattn; only the asked-for passes run."""
    from plagnn import ops

    g = gc.graph(gname)
    dg = g.on(dev)
    n, E = g.num_nodes, g.num_edges
    rng = np.random.default_rng(71)
    xl, xr, attn, dS = gc._randn(rng, n, H * Fh), gc._randn(rng, n, H * Fh), gc._randn(rng, 1, H, Fh), \
        gc._randn(rng, E, H)
    dst, src, _ = sc.slot_edges(g)
    src, dst = torch.from_numpy(src), torch.from_numpy(dst)
    l64, r64, a64 = (_leaf(t, dtype=torch.float64) for t in (xl, xr, attn))
    s64 = score64(src, dst, l64.view(n, H, Fh), r64.view(n, H, Fh), a64, slope)
    s64.backward(dS.double())

    calls = count_dattn_passes(monkeypatch)
    ld, rd, ad = _leaf(xl, dev), _leaf(xr, dev), _leaf(attn, dev)
    s = ops.GATv2Score.apply(ld, rd, ad, dg, H, slope)
    assert tuple(s.shape) == (E, H)
    s.backward(dS.to(dev))
    assert calls == {"passes": 2, "dattn": 1}
    close(s, s64, 1e-5, "scores")
    close(ld.grad, l64.grad, 1e-5, "d xl")
    close(rd.grad, r64.grad, 1e-5, "d xr")
    close(ad.grad, a64.grad, 1e-5, "d attn")
    assert ad.grad.shape == (1, H, Fh)

    # attn frozen: the dattn work is skipped
    calls.update(passes=0, dattn=0)
    ld, rd = _leaf(xl, dev), _leaf(xr, dev)
    ops.GATv2Score.apply(ld, rd, attn.to(dev), dg, H, slope).backward(dS.to(dev))
    assert calls == {"passes": 2, "dattn": 0}
    close(ld.grad, l64.grad, 1e-5, "d xl (attn frozen)")
    close(rd.grad, r64.grad, 1e-5, "d xr (attn frozen)")
    # only attn: one pass, no node gradient; only xl: one pass on the transposed CSR
    calls.update(passes=0, dattn=0)
    ad = _leaf(attn, dev)
    ops.GATv2Score.apply(xl.to(dev), xr.to(dev), ad, dg, H, slope).backward(dS.to(dev))
    assert calls == {"passes": 1, "dattn": 1}
    close(ad.grad, a64.grad, 1e-5, "d attn (alone)")
    calls.update(passes=0, dattn=0)
    ld = _leaf(xl, dev)
    ops.GATv2Score.apply(ld, xr.to(dev), attn.to(dev), dg, H, slope).backward(dS.to(dev))
    assert calls == {"passes": 1, "dattn": 0}
    close(ld.grad, l64.grad, 1e-5, "d xl (alone)")


def _lin64(x, p, name):
    y = x @ p[name + ".weight"].t()
    return y + p[name + ".bias"] if name + ".bias" in p else y


def gatv2_64(src, dst, n, x, p, H, out, slope, residual, share):
    el = _lin64(x, p, "fc_src").view(n, H, out)
    er = el if share else _lin64(x, p, "fc_dst").view(n, H, out)
    a = gc.softmax64(dst, n, score64(src, dst, el, er, p["attn"], slope))
    rst = torch.zeros(n, H, out, dtype=torch.float64).index_add_(0, dst, el[src] * a[:, :, None])
    if residual:
        rst = rst + (_lin64(x, p, "res_fc") if "res_fc.weight" in p else x).view(n, -1, out)
    return rst, a


def conv_case(dev, fin, fout, H, residual, share, bias, self_loop=True, seed=47):
    from dgl.nn.pytorch import GATv2Conv

    src, dst, g, rng = gc.shim_case(dev, seed=seed, self_loop=self_loop)
    torch.manual_seed(11)
    conv = GATv2Conv(fin, fout, H, residual=residual, share_weights=share, bias=bias,
                     allow_zero_in_degree=not self_loop).to(dev)
    with torch.no_grad():  # biases start at zero: give them values so their gradients matter
        for k, v in conv.named_parameters():
            if k.endswith(".bias"):
                v.copy_(gc._randn(rng, *v.shape) * 0.1)
    return src, dst, g, rng, conv


def check_gatv2conv(dev, fin, fout, H, residual=False, share=False, bias=True, self_loop=True):
    """GATv2Conv against a pure-torch float64 GATv2 with the same parameters: output, attention
    (edge-id order), every parameter's and the input's gradient, the state_dict keys."""
    src, dst, g, rng, conv = conv_case(dev, fin, fout, H, residual, share, bias, self_loop)
    E, n = len(src), g.num_nodes()
    lin = lambda name: [name + ".weight"] + ([name + ".bias"] if bias else [])  # noqa: E731
    keys = lin("fc_src") + lin("fc_dst") + ["attn"] + (lin("res_fc") if residual and fin != H * fout else [])
    assert sorted(conv.state_dict().keys()) == sorted(keys)
    assert conv.attn.shape == (1, H, fout) and conv.fc_src.weight.shape == (H * fout, fin)
    assert (conv.fc_dst is conv.fc_src) == share
    x, dZ, dA = gc._randn(rng, n, fin), gc._randn(rng, n, H, fout), gc._randn(rng, E, H, 1)
    xd = _leaf(x, dev)
    y, att = conv(g, xd, get_attention=True)
    assert tuple(y.shape) == (n, H, fout) and tuple(att.shape) == (E, H, 1)
    assert tuple(conv(g, xd).shape) == (n, H, fout)
    ((y * dZ.to(dev)).sum() + (att * dA.to(dev)).sum()).backward()
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    x64 = _leaf(x, dtype=torch.float64)
    y64, a64 = gatv2_64(src, dst, n, x64, p64, H, fout, 0.2, residual, share)
    ((y64 * dZ.double()).sum() + (a64 * dA.reshape(E, H).double()).sum()).backward()
    close(y, y64, 1e-5, "out")
    close(att.reshape(E, H), a64, 1e-5, "attention")
    tot = torch.zeros(n, H, dtype=torch.float64).index_add_(0, dst, att.detach().cpu().double().reshape(E, H))
    live = torch.bincount(dst, minlength=n) > 0
    assert bool(((tot[live] - 1).abs() < 1e-5).all()), "attention sums to 1 per destination and head"
    close(xd.grad, x64.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(v.grad, p64[k].grad, 1e-5, "d " + k)


def check_gatv2conv_frozen_attn(dev, monkeypatch):
    src, dst, g, rng, conv = conv_case(dev, 12, 8, 2, False, False, True)
    conv.attn.requires_grad_(False)
    calls = count_dattn_passes(monkeypatch)
    conv(g, gc._randn(rng, g.num_nodes(), 12).to(dev)).sum().backward()
    assert calls == {"passes": 2, "dattn": 0} and conv.attn.grad is None
    assert conv.fc_src.weight.grad is not None and conv.fc_dst.weight.grad is not None


def check_fused_vs_unfused(dev, fin=10, fout=6, H=3):
    """GATv2Conv equals the same layer written on the shim's own primitives."""
    import dgl.function as fn
    from dgl.nn.functional import edge_softmax

    src, dst, g, rng, conv = conv_case(dev, fin, fout, H, True, False, True, seed=49)
    n = g.num_nodes()
    x, dZ = gc._randn(rng, n, fin), gc._randn(rng, n, H, fout).to(dev)
    xd = _leaf(x, dev)
    y, att = conv(g, xd, get_attention=True)
    (y * dZ).sum().backward()
    grads = {k: v.grad.clone() for k, v in conv.named_parameters()}
    conv.zero_grad()

    xu = _leaf(x, dev)
    with g.local_scope():
        el = conv.fc_src(xu).view(n, H, fout)
        er = conv.fc_dst(xu).view(n, H, fout)
        g.srcdata["el"], g.dstdata["er"] = el, er
        g.apply_edges(fn.u_add_v("el", "er", "e"))
        e = torch.nn.functional.leaky_relu(g.edata.pop("e"), 0.2)
        a = edge_softmax(g, (e * conv.attn).sum(-1, keepdim=True))
        g.edata["a"] = a
        g.update_all(fn.u_mul_e("el", "a", "m"), fn.sum("m", "ft"))
        yu = g.dstdata["ft"] + conv.res_fc(xu).view(n, -1, fout)
    (yu * dZ).sum().backward()
    close(y, yu, 1e-5, "out")
    close(att, a, 1e-5, "attention")
    close(xd.grad, xu.grad, 1e-5, "d feat")
    for k, v in conv.named_parameters():
        close(grads[k], v.grad, 1e-5, "d " + k)


def check_module_surface(dev):
    import pytest
    import dgl
    import plagnn
    from dgl.nn.pytorch import GATv2Conv

    assert dgl.nn.pytorch.GATv2Conv is GATv2Conv and dgl.nn.GATv2Conv is GATv2Conv
    assert "GATv2Conv" in dgl.nn.pytorch.__all__
    src, dst, g, rng = gc.shim_case(dev, seed=41, self_loop=False)
    n = g.num_nodes()
    assert int((g.in_degrees() == 0).sum()) > 0
    conv = GATv2Conv(6, 4, 2).to(dev)
    assert not conv.fc_src.bias.any() and not conv.fc_dst.bias.any(), "biases start at zero"
    with pytest.raises(plagnn.PlagnnError, match="0-in-degree"):
        conv(g, torch.zeros(n, 6, device=dev))
    conv.set_allow_zero_in_degree(True)
    y, att = conv(g, gc._randn(rng, n, 6).to(dev), get_attention=True)
    assert tuple(y.shape) == (n, 2, 4) and tuple(att.shape) == (len(src), 2, 1)
    zero = torch.from_numpy(np.bincount(dst.numpy(), minlength=n) == 0)
    assert not y.detach().cpu()[zero].any(), "a node without in-edges aggregates nothing"
    with pytest.raises(NotImplementedError):
        GATv2Conv((6, 6), 4, 2)
    with pytest.raises(NotImplementedError):
        x = torch.zeros(n, 6, device=dev)
        conv(g, (x, x))
    # an identity residual needs no parameters
    assert isinstance(GATv2Conv(8, 4, 2, residual=True).res_fc, torch.nn.Identity)
    assert GATv2Conv(8, 4, 2).res_fc is None
