"""Shared by test_gspmm_cpu.py and test_gpu_gspmm.py: float64 numpy references for pg_gspmm and
pg_gsddmm (vector edge features), computed from the CSR entry lists of the graph (never by the
code under test), and the checks both files run (on the CPU device and on the GPU).

Two input families.
  Grid: operands on which every operator is exact in float32, so the results must equal the
    float64 reference bit for bit (sum, max, min, every pg_gsddmm form; mean within one ulp).
    Node values are multiples of 0.25 in [-2, 2], edge values are in {+-0.5, +-1, +-2, +-4}:
    every message is a multiple of 1/16 of magnitude <= 8, and a sum over hub64's ~2 100-entry
    row stays far below 2^24 units of 1/16, so it is exact in any order. A divisor is always
    drawn from the power-of-two set, also where pg_gsddmm's right operand sits at a node
    (a quotient by 0.75 is not exact, one by 0 not finite). Ties are frequent, which pins the
    first-wins rule of max / min across the pieces of split rows.
  Gaussian, u = 2^-24, m_k the float64 messages of a row:
    sum   |got - ref| <= (deg + 3) u sum_k |m_k| + 1e-30 (deg - 1 additions, one rounding per
          message, spare), mean: that over deg plus u |ref| for the division;
    max / min  |got - ref| <= 2 u |ref| (one rounding of the winning message), and the record
          names an entry whose float64 message is within that of the extremum;
    pg_gsddmm  |got - ref| <= 2 u |ref|.
Autograd through the shim: 1e-5 of each tensor's magnitude (sddmm_common.close) against a
float64 torch composition that routes a max / min gradient to the explicit first winner.
"""
import re

import numpy as np
import torch

import gat_common as gc
import sddmm_common as sc
from sddmm_common import U, _leaf, close

OPS = ["add", "sub", "mul", "div", "copy_lhs", "copy_rhs"]
BINARY = ["add", "sub", "mul", "div"]
REDUCERS = ["sum", "max", "min"]
WIDTHS = [1, 5, 8, 64, 100, 256, 300]
GRAPHS = gc.GRAPHS
TRIO = [("mul", "sum"), ("add", "max"), ("copy_rhs", "min")]
TARGET_PAIRS = [("u", "v"), ("v", "u"), ("u", "e"), ("e", "u"), ("v", "e"), ("e", "v")]
SENT = 7.0
ARG_SENT = 77
NEW_SYMBOLS = ["pg_gspmm", "pg_gspmm_workspace", "pg_gsddmm", "pg_gspmm_cpu", "pg_gsddmm_cpu"]


# ------------------------------------------------------------------ graph entry lists
def entries(g, transpose, eidx="eid", seed=0):
    """(row, gathered row, in-row position, edge row, eidx argument) of every entry of the
    in-CSR (transpose: of the out-CSR). eidx: 'eid' = edge-id order (the wrapper's cached
    map), None = the in-CSR slot order, 'perm' = an explicit non-identity permutation."""
    h = g.bwd if transpose else g.fwd
    ptr = h.ptr.astype(np.int64)
    row = np.repeat(np.arange(g.num_nodes), np.diff(ptr))
    pos = np.arange(h.nnz) - ptr[row]
    slot = h.eslot.astype(np.int64) if h.eslot is not None else np.arange(h.nnz)
    if eidx == "eid":
        erow, arg = g.eid.astype(np.int64)[slot], "eid"
    elif eidx is None:
        erow, arg = slot, None
    else:
        erow = np.random.default_rng(seed + 99).permutation(h.nnz).astype(np.int64)
        assert h.nnz < 2 or (erow != np.arange(h.nnz)).any()
        arg = erow.astype(np.int32)
    return row, h.col.astype(np.int64), pos, erow, arg, ptr


def operand_rows(t, target, row, colr, erow):
    return t[colr] if target == "u" else t[row] if target == "v" else t[erow]


def messages(op, L, lt, R, rt, row, colr, erow):
    """float64 messages (one row per CSR entry) of float32 operands."""
    l = operand_rows(L.astype(np.float64), lt, row, colr, erow) if op != "copy_rhs" else None
    r = operand_rows(R.astype(np.float64), rt, row, colr, erow) if op != "copy_lhs" else None
    with np.errstate(all="ignore"):
        return {"add": lambda: l + r, "sub": lambda: l - r, "mul": lambda: l * r, "div": lambda: l / r,
                "copy_lhs": lambda: l, "copy_rhs": lambda: r}[op]()


def reduce_ref(m, row, ptr, n, reduce):
    """(ref, bar, records) of a reduce over the float64 messages m. Records: the first
    extremal entry's in-row position, -1 for a row without entries; +-inf is stored as 0."""
    F = m.shape[1]
    deg = np.diff(ptr).astype(np.float64)[:, None]
    if reduce in ("sum", "mean"):
        ref, ab = np.zeros((n, F)), np.zeros((n, F))
        np.add.at(ref, row, m)
        np.add.at(ab, row, np.abs(m))
        bar = (deg + 3) * U * ab + 1e-30
        if reduce == "mean":
            d = np.maximum(deg, 1.0)
            ref, bar = ref / d, bar / d + U * np.abs(ref / d)
        return ref, bar, None
    ref, arg = np.zeros((n, F)), np.full((n, F), -1, np.int64)
    for v in range(n):
        b, e = ptr[v], ptr[v + 1]
        if e > b:
            a = np.argmax(m[b:e], axis=0) if reduce == "max" else np.argmin(m[b:e], axis=0)  # the first
            arg[v] = a
            ref[v] = m[b + a, np.arange(F)]
    ref[np.isinf(ref)] = 0.0
    return ref, 2 * U * np.abs(ref) + 1e-300, arg


# ------------------------------------------------------------------ inputs
def grid_nodes(rng, n, F):
    return (rng.integers(-8, 9, (n, F)) / 4.0).astype(np.float32)


def grid_edges(rng, E, F):
    return rng.choice(np.array([-4, -2, -1, -0.5, 0.5, 1, 2, 4], np.float32), (E, F))


def operands(g, op, lt, rt, F, family, seed):
    """(L, R) float32 for the targets; grid: a divisor comes from the power-of-two set."""
    rng = np.random.default_rng(seed)
    out = []
    for side, tgt in (("l", lt), ("r", rt)):
        rows = g.num_edges if tgt == "e" else g.num_nodes
        if family == "gauss":
            out.append(rng.standard_normal((rows, F)).astype(np.float32))
        elif tgt == "e" or (side == "r" and op == "div"):
            out.append(grid_edges(rng, rows, F))
        else:
            out.append(grid_nodes(rng, rows, F))
    return out


def padded(values, dev, pad, sent=SENT):
    """Device tensor holding `values`; pad > 0: a view of a buffer `pad` columns wider whose
    other columns hold a sentinel. Returns (view, buffer or None)."""
    t = sc.to_dev(values, dev)
    if pad == 0:
        return t, None
    buf = torch.full((t.shape[0], t.shape[1] + pad), sent, dtype=t.dtype, device=dev)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]], buf


def untouched(buf, F, sent=SENT):
    return buf is None or bool((buf[:, F:] == sent).all())


def arg_dtype(kind):
    return torch.int16 if kind == 16 else torch.int32


def records_to_dev(arg, kind, dev, pad=0):
    """int64 records (-1 = none) as the u16 / i32 device tensor the entry points read."""
    a = arg.copy()
    if kind == 16:
        a[a < 0] = 0xFFFF
        a = a.astype(np.uint16).view(np.int16)
    else:
        a = a.astype(np.int32)
    return padded(a, dev, pad, ARG_SENT)


# ------------------------------------------------------------------ kernel-level runs
def run_gspmm(dev, g, op, reduce, L, R, lt="u", rt="e", transpose=False, pad=0, eidx="eid", kind=None):
    """ops.gspmm on `dev` -> (out, records as int64 or None, float64 messages, entry lists)."""
    from plagnn import ops

    ent = entries(g, transpose, eidx)
    row, colr, pos, erow, earg, ptr = ent
    n, F = g.num_nodes, (L if op != "copy_rhs" else R).shape[1]
    Lt = padded(L, dev, pad)[0] if op != "copy_rhs" else None
    Rt = padded(R, dev, pad)[0] if op != "copy_lhs" else None
    if isinstance(earg, np.ndarray):
        earg = sc.to_dev(earg, dev)
    out, obuf = padded(np.full((n, F), SENT, np.float32), dev, pad)
    cmp_ = reduce in ("max", "min")
    h = g.bwd if transpose else g.fwd
    k = kind if kind is not None else (16 if h.max_deg < 0xFFFF else 32)
    argpos, abuf = padded(np.full((n, F), ARG_SENT, np.int16 if k == 16 else np.int32), dev, pad, ARG_SENT) \
        if cmp_ else (None, None)
    res = ops.gspmm(g.on(dev), op, reduce, Lt, Rt, lt, rt, transpose=transpose, eidx=earg, out=out,
                    argpos=argpos, arg_kind=kind)
    got, rec = (res if cmp_ else (res, None))
    assert got.data_ptr() == out.data_ptr() and untouched(obuf, F), "output padding written"
    if cmp_:
        assert rec.dtype == arg_dtype(k) and untouched(abuf, F, ARG_SENT), "record padding written"
        rec = sc.argpos_np(rec)
    m = messages(op, L, lt, R, rt, row, colr, erow) if h.nnz else np.zeros((0, F))
    return got, rec, m, ent


def check_gspmm(dev, gname, op, reduce, F, family, transpose=False, pad=0, eidx="eid", kind=None, seed=3):
    """One pg_gspmm call against the float64 reference: grid bitwise (mean: one ulp), records
    equal to numpy's first argmax / argmin; gauss within the bars. Returns (out, records)."""
    g = gc.graph(gname)
    L, R = operands(g, op, "u", "e", F, family, seed)
    got, rec, m, (row, colr, pos, erow, earg, ptr) = run_gspmm(dev, g, op, reduce, L, R, transpose=transpose,
                                                              pad=pad, eidx=eidx, kind=kind)
    ref, bar, arg = reduce_ref(m, row, ptr, g.num_nodes, reduce)
    name = f"gspmm {gname} {op}/{reduce} F={F} {family} T={transpose} pad={pad} eidx={eidx}"
    gn = got.detach().cpu().numpy().astype(np.float64)
    empty = np.diff(ptr) == 0
    if empty.any():
        assert not gn[empty].any(), f"{name}: rows without entries are not 0"
        assert rec is None or (rec[empty] == -1).all(), f"{name}: rows without entries have records"
    if family == "grid":
        if reduce == "mean":
            gc.within(got, ref, 2.0 ** -23 * np.abs(ref) + 1e-300, name)
        else:
            assert np.array_equal(gn, ref), f"{name}: not bitwise the float64 reference " \
                                            f"(max diff {np.abs(gn - ref).max():.3e})"
        if rec is not None:
            assert np.array_equal(rec, arg), f"{name}: {int((rec != arg).sum())} records differ from the first winner"
    else:
        gc.within(got, ref, bar, name)
        if rec is not None:
            assert ((rec >= 0) == (arg >= 0)).all()
            k = np.minimum(ptr[:-1, None] + np.maximum(rec, 0), max(len(m) - 1, 0))
            won = np.where(rec >= 0, m[k, np.arange(F)[None, :]] if len(m) else 0.0, 0.0)
            won[np.isinf(won)] = 0.0
            assert (np.abs(won - ref) <= bar).all(), f"{name}: a record names an entry off the extremum"
    return got, rec


def random_records(g, F, seed=5):
    """Records that name a random entry of each row per feature, none with probability ~1/8."""
    rng = np.random.default_rng(seed)
    deg = np.diff(g.fwd.ptr.astype(np.int64))[:, None]
    a = (rng.random((g.num_nodes, F)) * deg).astype(np.int64)
    a[(deg == 0) | (rng.random((g.num_nodes, F)) < 0.125)] = -1
    return a


def check_gsddmm(dev, gname, op, lt, rt, F, family, masked=False, pad=0, eidx="eid", kind=None, seed=4):
    from plagnn import ops

    g = gc.graph(gname)
    L, R = operands(g, op, lt, rt, F, family, seed)
    row, colr, pos, erow, earg, ptr = entries(g, False, eidx)
    Lt = padded(L, dev, pad)[0] if op != "copy_rhs" else None
    Rt = padded(R, dev, pad)[0] if op != "copy_lhs" else None
    if isinstance(earg, np.ndarray):
        earg = sc.to_dev(earg, dev)
    out, obuf = padded(np.full((g.num_edges, F), SENT, np.float32), dev, pad)
    k = kind if kind is not None else 16
    rec = random_records(g, F) if masked else None
    argpos = records_to_dev(rec, k, dev, pad)[0] if masked else None
    got = ops.gsddmm(g.on(dev), op, Lt, Rt, lt, rt, eidx=earg, out=out, argpos=argpos, arg_kind=kind)
    assert got.data_ptr() == out.data_ptr() and untouched(obuf, F), "output padding written"
    m = messages(op, L, lt, R, rt, row, colr, erow)
    if masked:
        m = np.where(rec[row] == pos[:, None], m, 0.0)
    ref = np.zeros_like(m)
    ref[erow] = m
    name = f"gsddmm {gname} {lt}_{op}_{rt} F={F} {family} masked={masked} pad={pad} eidx={eidx}"
    if family == "grid":
        gn = got.detach().cpu().numpy().astype(np.float64)
        assert np.array_equal(gn, ref), f"{name}: not bitwise the float64 reference"
    else:
        gc.within(got, ref, 2 * U * np.abs(ref) + 1e-300, name)
    return got


def check_devices_agree(dev, gname, op, reduce, F, transpose=False):
    """`dev` against the CPU device: bitwise on grid inputs (values and records); on Gaussian
    inputs within twice the bars (each side is within one bar of the reference), twice in a
    row on `dev` bitwise the same."""
    g = gc.graph(gname)
    for family in ("grid", "gauss"):
        L, R = operands(g, op, "u", "e", F, family, 8)
        a, ra, m, (row, _, _, _, _, ptr) = run_gspmm(dev, g, op, reduce, L, R, transpose=transpose)
        a2, ra2, _, _ = run_gspmm(dev, g, op, reduce, L, R, transpose=transpose)
        b, rb, _, _ = run_gspmm("cpu", g, op, reduce, L, R, transpose=transpose)
        assert torch.equal(a, a2) and (ra is None or np.array_equal(ra, ra2)), "repeated calls differ"
        if family == "grid":
            assert torch.equal(a.cpu(), b) and (ra is None or np.array_equal(ra, rb)), \
                f"{gname} {op}/{reduce} F={F}: {dev} and cpu differ on grid inputs"
        else:
            bar = reduce_ref(m, row, ptr, g.num_nodes, reduce)[1]
            gc.within(a, b.numpy().astype(np.float64), bar, f"{dev} vs cpu {gname} {op}/{reduce} F={F}", factor=2.0)


def check_devices_agree_gsddmm(dev, gname, op, lt, rt, F, masked):
    for family in ("grid", "gauss"):
        a = check_gsddmm(dev, gname, op, lt, rt, F, family, masked=masked)
        a2 = check_gsddmm(dev, gname, op, lt, rt, F, family, masked=masked)
        b = check_gsddmm("cpu", gname, op, lt, rt, F, family, masked=masked)
        assert torch.equal(a, a2), "repeated calls differ"
        if family == "grid":
            assert torch.equal(a.cpu(), b), f"gsddmm {gname} {lt}_{op}_{rt} F={F}: {dev} and cpu differ"
        else:
            b64 = b.numpy().astype(np.float64)
            gc.within(a, b64, 2 * U * np.abs(b64) + 1e-300, f"gsddmm {dev} vs cpu {lt}_{op}_{rt}", factor=2.0)


def check_inf_edge(dev, reduce="max"):
    """One +inf edge value under add / max: that row's maximum is +inf, stored as 0 (DGL's
    replace_inf_with_zero); its record still names the edge."""
    g = gc.graph("hub")
    L, R = operands(g, "add", "u", "e", 8, "grid", 6)
    row, colr, pos, erow, earg, ptr = entries(g, False)
    k = int(ptr[3])  # the first entry of row 3
    assert row[k] == 3
    R[erow[k], 2] = np.inf
    got, rec, m, _ = run_gspmm(dev, g, "add", reduce, L, R)
    ref, bar, arg = reduce_ref(m, row, ptr, g.num_nodes, reduce)
    assert ref[3, 2] == 0.0 and arg[3, 2] == 0
    assert np.array_equal(got.cpu().numpy().astype(np.float64), ref) and np.array_equal(rec, arg)


def check_empty_shapes(dev):
    """nnz == 0, n_rows == 0 and F == 0 succeed; a graph without edges gives zeros and none."""
    import plagnn
    from plagnn import ops

    z = np.zeros(0, np.int64)
    dg = plagnn.CSRGraph(z, z, 5).on(dev)
    x, e = torch.ones(5, 8, device=dev), torch.zeros(0, 8, device=dev)
    for red in ("sum", "mean"):
        out = ops.gspmm(dg, "mul", red, x, e)
        assert out.shape == (5, 8) and not out.any()
    out, rec = ops.gspmm(dg, "add", "max", x, e)
    assert not out.any() and (sc.argpos_np(rec) == -1).all()
    assert ops.gsddmm(dg, "sub", x, x, "u", "v").shape == (0, 8)
    dg0 = plagnn.CSRGraph(z, z, 0).on(dev)
    x0 = torch.zeros(0, 8, device=dev)
    assert ops.gspmm(dg0, "mul", "sum", x0, e).shape == (0, 8)
    assert ops.gspmm(dg0, "copy_rhs", "min", None, e)[0].shape == (0, 8)
    assert ops.gsddmm(dg0, "add", x0, e, "u", "e").shape == (0, 8)
    g = gc.graph("hub")
    dg = g.on(dev)
    xf, ef = torch.zeros(g.num_nodes, 0, device=dev), torch.zeros(g.num_edges, 0, device=dev)
    assert ops.gspmm(dg, "mul", "sum", xf, ef).shape == (g.num_nodes, 0)
    assert ops.gspmm(dg, "mul", "max", xf, ef)[0].shape == (g.num_nodes, 0)
    assert ops.gsddmm(dg, "mul", xf, ef, "v", "e").shape == (g.num_edges, 0)


def check_abi_rejections(dev):
    """Argument errors come back as PlagnnError with the library's message."""
    import pytest
    from plagnn import _lib, ops
    from plagnn._lib import ptr

    g = gc.graph("hub")
    dg = g.on(dev)
    n, E = g.num_nodes, g.num_edges
    x, e, out = torch.zeros(n, 8, device=dev), torch.zeros(E, 8, device=dev), torch.zeros(n, 8, device=dev)
    s = dg.fwd.struct(None)
    cpu = dev == "cpu"
    tail = () if cpu else (0, 0, 0)
    name = "pg_gspmm_cpu" if cpu else "pg_gspmm"
    with pytest.raises(_lib.PlagnnError, match="bad op"):
        _lib.call(name, s, 9, 0, ptr(x), 8, 0, ptr(e), 8, 2, 0, 8, 0, ptr(out), 8, 0, 0, 16, *tail)
    with pytest.raises(_lib.PlagnnError, match="target"):  # V is a pg_gsddmm target only
        _lib.call(name, s, 0, 0, ptr(x), 8, 1, ptr(e), 8, 2, 0, 8, 0, ptr(out), 8, 0, 0, 16, *tail)
    with pytest.raises(_lib.PlagnnError, match="leading"):
        _lib.call(name, s, 0, 0, ptr(x), 4, 0, ptr(e), 8, 2, 0, 8, 0, ptr(out), 8, 0, 0, 16, *tail)
    with pytest.raises(_lib.PlagnnError, match="norm_mode"):  # mean belongs to sum
        _lib.call(name, s, 0, 1, ptr(x), 8, 0, ptr(e), 8, 2, 0, 8, 1, ptr(out), 8, 0, 0, 16, *tail)
    with pytest.raises(_lib.PlagnnError, match="alias"):
        ops.gsddmm(dg, "add", e, x, "e", "v", out=e)
    with pytest.raises(ValueError):
        ops.gspmm(dg, "mul", "sum", x, torch.zeros(E, 4, device=dev))
    with pytest.raises(ValueError):
        ops.gspmm(dg, "pow", "sum", x, e)


def check_exports():
    """pg_version() stays 13 and every symbol the header newly declares is exported."""
    import os
    from plagnn import _lib

    assert _lib.lib().pg_version() == 13 and _lib.ABI_VERSION == 13
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "plagnn.h")) as f:
        declared = set(re.findall(r"\b(pg_gs(?:pmm|ddmm)\w*)\s*\(", f.read()))
    assert declared == set(NEW_SYMBOLS), declared
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name


# ------------------------------------------------------------------ autograd through the shim
def first_winner(m, dst, n, reduce):
    """(E-index of the first extremal in-edge per (node, feature), none mask) of float64
    messages m (E, F) in edge-id order: rows list their in-edges in ascending edge id."""
    mn = m.detach().numpy()
    order = np.argsort(dst.numpy(), kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(dst.numpy(), minlength=n))])
    F = mn.shape[1]
    idx, none = np.zeros((n, F), np.int64), np.ones((n, F), bool)
    for v in range(n):
        ids = order[ptr[v]:ptr[v + 1]]
        if len(ids):
            a = np.argmax(mn[ids], axis=0) if reduce == "max" else np.argmin(mn[ids], axis=0)
            idx[v], none[v] = ids[a], False
    return torch.from_numpy(idx), torch.from_numpy(none)


def reduce64(m, dst, n, reduce):
    """The reduce of float64 torch messages (E, F), differentiable; max / min gather the
    explicit first winner, so a tie sends the whole gradient there (scatter_reduce splits it)."""
    if reduce in ("sum", "mean"):
        out = torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, dst, m)
        if reduce == "mean":
            out = out / torch.bincount(dst, minlength=n).clamp(min=1).double()[:, None]
        return out
    idx, none = first_winner(m, dst, n, reduce)
    return torch.gather(m, 0, idx).masked_fill(none, 0.0)


def op64(op, l, r):
    return {"add": lambda: l + r, "sub": lambda: l - r, "mul": lambda: l * r, "div": lambda: l / r,
            "dot": lambda: (l * r).sum(-1, keepdim=True)}[op]()


def _case(dev, shape, seed):
    src, dst, g, rng = gc.shim_case(dev, seed=seed)
    n, E = g.num_nodes(), len(src)
    return src, dst, g, rng, n, E, gc._randn(rng, n, *shape), gc._randn(rng, n, *shape), gc._randn(rng, E, *shape)


def _compare(out, ref, leaves, leaves64, rng, name, scales=None):
    """Output and gradients within 1e-5 of each tensor's magnitude. scales: {operand index:
    callable giving the magnitude to use after the float64 backward}, for a gradient that is
    identically zero in exact arithmetic (its own magnitude is no scale)."""
    close(out, ref, 1e-5, name + " out")
    w = torch.from_numpy(rng.standard_normal(tuple(ref.shape)))
    (out.double() * w.to(out.device)).sum().backward()
    (ref * w).sum().backward()
    for k, (a, b) in enumerate(zip(leaves, leaves64)):
        assert a.grad is not None, f"{name}: operand {k} has no gradient"
        if scales and k in scales:
            err, scale = (a.grad.detach().cpu().double() - b.grad).abs().max().item(), scales[k]()
            print(f"{name} d operand {k}: max err {err:.3e}, scale of its terms {scale:.3e}")
            assert err <= 1e-5 * scale, f"{name} d operand {k}: max err {err:.3e} vs scale {scale:.3e}"
        else:
            close(a.grad, b.grad, 1e-5, f"{name} d operand {k}")


def check_update_all(dev, msg, reduce, shape=(6,), seed=51):
    """update_all(msg, reduce) for msg = u_<op>_e | e_<op>_u | copy_e | copy_u, gradients in
    every operand."""
    import dgl.function as fn

    src, dst, g, rng, n, E, x, _, y = _case(dev, shape, seed)
    xd, yd, x64, y64 = _leaf(x, dev), _leaf(y, dev), _leaf(x, dtype=torch.float64), _leaf(y, dtype=torch.float64)
    g.ndata["h"], g.edata["w"] = xd, yd
    if msg == "copy_u":
        mf, m64, leaves = fn.copy_u("h", "m"), x64[src], ((xd,), (x64,))
    elif msg == "copy_e":
        mf, m64, leaves = fn.copy_e("w", "m"), y64 * 1.0, ((yd,), (y64,))
    else:
        lt, op, rt = msg.split("_")
        names = {"u": "h", "e": "w"}
        mf = getattr(fn, msg)(names[lt], names[rt], "m")
        vals = {"u": x64[src], "e": y64}
        m64, leaves = op64(op, vals[lt], vals[rt]), ((xd, yd), (x64, y64))
    g.update_all(mf, getattr(fn, reduce)("m", "o"))
    out = g.ndata["o"]
    assert tuple(out.shape) == (n,) + tuple(shape)
    F = int(np.prod(shape))
    ref = reduce64(m64.reshape(E, F), dst, n, reduce).reshape((n,) + tuple(shape))
    _compare(out, ref, leaves[0], leaves[1], rng, f"update_all {msg}/{reduce}")


def check_apply_edges(dev, msg, shape=(2, 4), seed=53):
    import dgl.function as fn

    src, dst, g, rng, n, E, a, b, y = _case(dev, shape, seed)
    lt, op, rt = msg.split("_")
    host = {"u": a, "v": b, "e": y}
    dl, dr = _leaf(host[lt], dev), _leaf(host[rt], dev)
    l64, r64 = _leaf(host[lt], dtype=torch.float64), _leaf(host[rt], dtype=torch.float64)
    frames = {"u": g.ndata, "v": g.ndata, "e": g.edata}
    frames[lt]["l"], frames[rt]["r"] = dl, dr
    g.apply_edges(getattr(fn, msg)("l", "r", "z"))
    at = {"u": lambda t: t[src], "v": lambda t: t[dst], "e": lambda t: t}
    ref = op64(op, at[lt](l64), at[rt](r64))
    assert tuple(g.edata["z"].shape) == tuple(ref.shape)
    _compare(g.edata["z"], ref, (dl, dr), (l64, r64), rng, f"apply_edges {msg}")


def check_dgl_ops(dev, seed=55):
    """dgl.ops.gspmm / gsddmm with DGL's signatures and three generated names."""
    import dgl

    src, dst, g, rng, n, E, x, b, y = _case(dev, (2, 4), seed)

    def run(name, call, ref_fn, hosts):
        ds = [_leaf(t, dev) for t in hosts]
        d64 = [_leaf(t, dtype=torch.float64) for t in hosts]
        _compare(call(*ds), ref_fn(*d64), ds, d64, rng, name)

    def red(m, reduce):
        return reduce64(m.reshape(E, -1), dst, n, reduce).reshape((n,) + tuple(m.shape[1:]))

    run("ops.gspmm mul/sum", lambda p, q: dgl.ops.gspmm(g, "mul", "sum", p, q), lambda p, q: red(p[src] * q, "sum"), (x, y))
    run("ops.gspmm div/mean", lambda p, q: dgl.ops.gspmm(g, "div", "mean", p, q), lambda p, q: red(p[src] / q, "mean"), (x, y))
    run("ops.gspmm copy_rhs/min", lambda q: dgl.ops.gspmm(g, "copy_rhs", "min", None, q), lambda q: red(q * 1.0, "min"), (y,))
    run("ops.gsddmm sub u v", lambda p, q: dgl.ops.gsddmm(g, "sub", p, q), lambda p, q: p[src] - q[dst], (x, b))
    run("ops.gsddmm dot e v", lambda q, p: dgl.ops.gsddmm(g, "dot", q, p, "e", "v"),
        lambda q, p: (q * p[dst]).sum(-1, keepdim=True), (y, b))
    run("ops.u_mul_e_sum", lambda p, q: dgl.ops.u_mul_e_sum(g, p, q), lambda p, q: red(p[src] * q, "sum"), (x, y))
    run("ops.copy_e_max", lambda q: dgl.ops.copy_e_max(g, q), lambda q: red(q * 1.0, "max"), (y,))
    run("ops.u_sub_v", lambda p, q: dgl.ops.u_sub_v(g, p, q), lambda p, q: p[src] - q[dst], (x, b))
    run("ops.e_sub_u_max", lambda q, p: dgl.ops.e_sub_u_max(g, q, p), lambda q, p: red(q - p[src], "max"), (y, x))


def check_edgeconv(dev, batch_norm, fin=6, fout=8, seed=57):
    """EdgeConv's output, input gradient and every parameter gradient against its float64
    composition (the module's own double copy for theta / phi / bn). With batch norm the
    gradients of theta.bias and phi.bias are identically zero (the norm removes any constant
    added to a column), so their error is measured against the magnitude of the terms they
    sum, sum_e |d loss / d e[e, j]| at the norm's input, not against their own."""
    import copy

    from dgl.nn.pytorch import EdgeConv

    src, dst, g, rng, n, E, x, _, _ = _case(dev, (fin,), seed)
    torch.manual_seed(seed)
    conv = EdgeConv(fin, fout, batch_norm=batch_norm)
    assert sorted(k.split(".")[0] for k, _ in conv.named_parameters()) == \
        sorted(["theta", "theta", "phi", "phi"] + (["bn", "bn"] if batch_norm else []))
    conv64 = copy.deepcopy(conv).double()
    conv = conv.to(dev)
    xd, x64 = _leaf(x, dev), _leaf(x, dtype=torch.float64)
    out = conv(g, xd)
    pre = conv64.theta(x64[dst] - x64[src]) + conv64.phi(x64)[dst]
    pre.retain_grad()
    e64 = conv64.bn(pre) if batch_norm else pre
    ref = reduce64(e64, dst, n, "max")
    p, p64 = dict(conv.named_parameters()), dict(conv64.named_parameters())
    keys = sorted(p)
    scales = {1 + i: (lambda: pre.grad.abs().sum(0).max().item()) for i, k in enumerate(keys)
              if batch_norm and k in ("theta.bias", "phi.bias")}
    _compare(out, ref, [xd] + [p[k] for k in keys], [x64] + [p64[k] for k in keys], rng,
             f"EdgeConv bn={batch_norm}", scales)
    assert "theta" not in g.edata and "x" not in g.ndata  # local_scope


def check_tie_gradient(dev):
    """Grid inputs with ties under copy_e / max: the whole gradient lands on the first winner."""
    import dgl.function as fn

    src, dst, g, rng = gc.shim_case(dev, seed=59)
    n, E = g.num_nodes(), len(src)
    y = torch.from_numpy(grid_edges(rng, E, 4))
    yd, y64 = _leaf(y, dev), _leaf(y, dtype=torch.float64)
    g.edata["w"] = yd
    g.update_all(fn.copy_e("w", "m"), fn.max("m", "o"))
    out = g.ndata["o"]
    idx, none = first_winner(y64, dst, n, "max")
    ties = (y64[:, None, :] == torch.gather(y64, 0, idx)[dst][:, None, :]).squeeze(1)
    assert int(torch.zeros(n, 4).index_add_(0, dst, ties.float()).max()) > 1, "the case has no ties"
    ref = torch.gather(y64, 0, idx).masked_fill(none, 0.0)
    assert torch.equal(out.detach().cpu().double(), ref.detach())
    w = torch.from_numpy(rng.integers(1, 5, (n, 4)).astype(np.float64))
    (out.double() * w.to(dev)).sum().backward()
    (ref * w).sum().backward()
    assert torch.equal(yd.grad.cpu().double(), y64.grad), "a tie's gradient is not all on the first winner"


def check_shim_rejections(dev):
    """The rejections the earlier suites pin stay NotImplementedError, and the new forms reject
    what they do not cover the same way."""
    import pytest
    import dgl
    import dgl.function as fn

    src, dst, g, rng = gc.shim_case(dev, seed=61)
    E, n = len(src), g.num_nodes()
    g.ndata["h"], g.edata["w"] = torch.zeros(n, 4, 8, device=dev), torch.zeros(E, 4, 1, device=dev)
    for red in ("max", "mean"):
        with pytest.raises(NotImplementedError):
            g.update_all(fn.u_mul_e("h", "w", "m"), getattr(fn, red)("m", "o"))
    g.ndata["h2"], g.edata["w2"] = torch.zeros(n, 32, device=dev), torch.zeros(E, 4, device=dev)
    for red in ("sum", "min"):
        with pytest.raises(NotImplementedError):
            g.update_all(fn.u_mul_e("h2", "w2", "m"), getattr(fn, red)("m", "o"))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.u_add_e("h2", "w2", "m"), fn.sum("m", "o"))
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.copy_u("h", "m"))
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.u_sub_v("h", "h", "e"), edges=torch.arange(3))
    with pytest.raises(NotImplementedError):
        g.apply_edges(lambda edges: {"s": edges.src["h"]})
    with pytest.raises(NotImplementedError):
        g.apply_edges(fn.u_mul_e("h2", "w2", "e"))
    for mf in (fn.u_add_v("h", "h", "m"), fn.u_dot_v("h", "h", "m"), fn.u_dot_e("h", "w", "m"),
               fn.v_mul_e("h", "w", "m")):
        with pytest.raises(NotImplementedError):
            g.update_all(mf, fn.sum("m", "o"))
    with pytest.raises(NotImplementedError):
        dgl.ops.gspmm(g, "mul", "sum", g.ndata["h2"], g.edata["w2"])
    assert fn.copy_edge is fn.copy_e


def check_scalar_forms_unchanged(dev, monkeypatch):
    """copy_u and one-weight-per-edge u_mul_e with sum / mean / max still call spmm_sum /
    spmm_max, never pg_gspmm; the vector form and min go to pg_gspmm."""
    import dgl.function as fn
    from plagnn import ops

    calls = {"sum": 0, "max": 0, "gspmm": 0}
    real = {"sum": ops.spmm_sum, "max": ops.spmm_max, "gspmm": ops.gspmm}

    def wrap(key):
        def f(*a, **k):
            calls[key] += 1
            return real[key](*a, **k)
        return f

    monkeypatch.setattr(ops, "spmm_sum", wrap("sum"))
    monkeypatch.setattr(ops, "spmm_max", wrap("max"))
    monkeypatch.setattr(ops, "gspmm", wrap("gspmm"))
    src, dst, g, rng = gc.shim_case(dev, seed=63)
    E, n = len(src), g.num_nodes()
    g.ndata["h"], g.edata["w"], g.edata["w1"] = gc._randn(rng, n, 8).to(dev), gc._randn(rng, E).to(dev), \
        gc._randn(rng, E, 1).to(dev)
    for w in ("w", "w1"):
        for red in ("sum", "mean", "max"):
            g.update_all(fn.u_mul_e("h", w, "m"), getattr(fn, red)("m", "o"))
            g.update_all(fn.copy_u("h", "m"), getattr(fn, red)("m", "o"))
    assert calls == {"sum": 8, "max": 4, "gspmm": 0}
    g.edata["wv"] = gc._randn(rng, E, 8).to(dev)
    g.update_all(fn.u_mul_e("h", "wv", "m"), fn.sum("m", "o"))
    g.update_all(fn.copy_u("h", "m"), fn.min("m", "o"))
    assert calls == {"sum": 8, "max": 4, "gspmm": 2}
