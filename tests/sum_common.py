"""Shared by test_spmm_sum_cpu.py and test_gpu_spmm_sum.py: references for pg_spmm_sum (the
sum / mean / edge-weighted aggregation and its transposed mean form), computed here with
numpy on the CPU from the CSR arrays (the oracle is not involved), the ladder graph both
files run on, and the checks themselves (on the CPU device and on the GPU).

Two statements are checked for every case.

The float64 bar (sum_ref64), valid for any summation order. With t_k = coef_k * X[col[k]]
(divided by the entry count of col[k] in the transposed mean form) the deg - 1 additions of
a row give at most (deg - 1) * u * sum_k |t_k| to first order (u = 2^-24), every term carries
at most two roundings (the product, the mode-2 division), the mean's division adds one and
one rounding is kept spare:
    |got - ref64| <= (deg + 3) * 2^-24 * sum_k |t_k| + 1e-30
both sides divided by the row's entry count in the mean form. A lost tile, a slot added
twice or a clamped gather row counted once too often is off by orders of magnitude.

The bitwise statement (sum_piecewise32). The library is built with -ffp-contract=off, every
schedule item sums its entries in order from +0 and every merge adds its slots in order from
+0, so the result is one fixed float32 expression, restated here from csr.items and
csr.merges with one numpy float32 operation per step. With split=False every row is one
item: pg_spmm_sum_cpu's order. Bit patterns are compared as int32.

Autograd bar: 1e-5 of each tensor's magnitude (sddmm_common.close).
"""
import functools

import numpy as np
import pytest
import torch

import sddmm_common as sc

U = 2.0 ** -24

# one lane; the scalar NC ladder (1, 2, 4, 8 with 8 edges in flight, 16 with 4); one vector
# tile, exactly one, one plus a last tile of width 4, two, two plus a partial scalar tile; the
# scalar tiling's full first launch and its second launch (1025; 1100 with an odd stride)
WIDTHS = [1, 3, 4, 63, 64, 65, 252, 256, 260, 503, 512, 513, 1023, 1024, 1025, 1100]
ALL_FORM_WIDTHS = [3, 64, 260, 503, 1100]
FORMS = {"plain": (False, False), "mean": (True, False), "weighted": (False, True), "weighted_mean": (True, True)}
# every width in the weighted mean form, every form at ALL_FORM_WIDTHS
WIDTH_CASES = [(F, "weighted_mean") for F in WIDTHS] + [(F, form) for F in ALL_FORM_WIDTHS for form in FORMS
                                                        if form != "weighted_mean"]
TRANSPOSED_WIDTHS = [3, 64, 260, 503, 1100]


def check_width_list():
    """The sweep has a width below, at and above every tile boundary of both paths."""
    for below, b, above in ((63, 64, 65), (252, 256, 260), (503, 512, 513), (1023, 1024, 1025)):
        assert below < b < above and {below, b, above} <= set(WIDTHS), b
    assert 260 in WIDTHS, "one vector tile plus a last tile of width 4"
    assert any(F % 4 == 0 and F > 1024 for F in WIDTHS), "past the widest single vector launch"
    assert any(F % 4 and F > 1024 for F in WIDTHS), "the scalar tiling's second launch"
    for F in WIDTHS:
        assert (F, "weighted_mean") in WIDTH_CASES
    for F in ALL_FORM_WIDTHS:
        assert all((F, form) in WIDTH_CASES for form in FORMS)


# ------------------------------------------------------------------ references
def _coef_index(csr):
    return np.arange(csr.nnz) if csr.eslot is None else csr.eslot.astype(np.int64)


def sum_ref64(csr, X, ew_slots, norm_mode, norm_ptr):
    """(float64 reference, error bar) of pg_spmm_sum over the HostCsr `csr` (g.fwd, or g.bwd
    with its eslot); X numpy float32, ew_slots numpy float32 in in-CSR slot order or None."""
    ptr, col = csr.ptr.astype(np.int64), csr.col.astype(np.int64)
    deg = np.diff(ptr)
    F = X.shape[1]
    ref = np.zeros((csr.n_rows, F))
    mag = np.zeros((csr.n_rows, F))
    if csr.nnz:
        with np.errstate(invalid="ignore", over="ignore"):
            T = X.astype(np.float64)[col]
            if ew_slots is not None:
                T *= ew_slots.astype(np.float64)[_coef_index(csr)][:, None]
            if norm_mode == 2:
                T /= np.diff(norm_ptr.astype(np.int64)).astype(np.float64)[col][:, None]
            nz = deg > 0
            ref[nz] = np.add.reduceat(T, ptr[:-1][nz], axis=0)
            mag[nz] = np.add.reduceat(np.abs(T), ptr[:-1][nz], axis=0)
    bar = (deg + 3.0)[:, None] * U * mag + 1e-30
    if norm_mode == 1:
        d = np.maximum(deg, 1).astype(np.float64)[:, None]
        ref, bar = ref / d, bar / d
    return ref, bar


def sum_piecewise32(csr, X, ew_slots, norm_mode, norm_ptr, split):
    """pg_spmm_sum's own summation order in numpy float32 (see the module docstring): the
    schedule's items and merges with split=True, one item per row with split=False."""
    ptr, col = csr.ptr.astype(np.int64), csr.col.astype(np.int64)
    deg = np.diff(ptr)
    F = X.shape[1]
    n = csr.n_rows
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.ascontiguousarray(X, dtype=np.float32)[col] if csr.nnz else np.zeros((0, F), np.float32)
        if ew_slots is not None and csr.nnz:
            T = T * ew_slots.astype(np.float32)[_coef_index(csr)][:, None]
        if norm_mode == 2 and csr.nnz:
            T = T / np.diff(norm_ptr.astype(np.int64)).astype(np.float32)[col][:, None]
        assert T.dtype == np.float32
        if split:
            items = csr.items.reshape(-1, 4)[:csr.n_items].astype(np.int64)
            merges = csr.merges.reshape(-1, 4)[:csr.n_merges].astype(np.int64)
        else:
            items = np.stack([np.arange(n), ptr[:-1], ptr[1:], np.full(n, -1)], 1).astype(np.int64)
            merges = np.zeros((0, 4), np.int64)
        length = items[:, 2] - items[:, 1]
        order = np.argsort(-length, kind="stable")  # longest first: the live items are a prefix
        items, length = items[order], length[order]
        acc = np.zeros((len(items), F), np.float32)  # +0
        for j in range(int(length.max()) if len(items) else 0):
            na = int(np.searchsorted(-length, -j, side="left"))  # items with length > j
            acc[:na] += T[items[:na, 1] + j]
        out = np.full((n, F), np.nan, np.float32)
        written = np.zeros(n, bool)
        whole = items[:, 3] < 0
        rows = items[whole, 0]
        val = acc[whole]
        if norm_mode == 1:
            d = deg[rows]
            val[d > 0] = val[d > 0] / d[d > 0].astype(np.float32)[:, None]
        out[rows] = val
        written[rows] = True
        part = np.zeros((int(csr.n_slots) if split else 0, F), np.float32)
        part[items[~whole, 3]] = acc[~whole]
        for row, s0, ns, _ in merges:
            a = np.zeros(F, np.float32)
            for s in range(s0, s0 + ns):
                a = a + part[s]
            if norm_mode == 1:
                a = a / np.float32(deg[row])
            assert not written[row]
            out[row] = a
            written[row] = True
        assert written.all() and out.dtype == np.float32
    return out


def bits_equal(a, b, nan_equal=False):
    """Element-wise equality of the float32 bit patterns; nan_equal: any NaN equals any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, f"shape {a.shape} vs {b.shape}"
    eq = a.view(np.int32) == b.view(np.int32)
    if nan_equal:
        eq |= np.isnan(a) & np.isnan(b)
    return eq


def assert_bits(got, want, name, nan_equal=False):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    eq = bits_equal(got, want, nan_equal)
    if not eq.all():
        r, f = np.argwhere(~eq)[0]
        raise AssertionError(f"{name}: {int((~eq).sum())} of {eq.size} elements differ bitwise, first at "
                             f"[{r}, {f}]: {got[r, f]!r} vs {want[r, f]!r}")


# ------------------------------------------------------------------ graphs
def _default_chunk():
    from plagnn import graph

    return graph.DEFAULT_CHUNK


@functools.lru_cache(maxsize=None)
def ladder_coo(c, seed=0, n=150):
    """(src, dst) of the ladder graph for a forward chunk of c: see ladder_graph."""
    rng = np.random.default_rng(seed)
    degs = [0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129,
            c - 1, c, c + 1, 2 * c + 1, 8 * c, 8 * c + 1, 20 * c + 3]
    degs = np.array(degs + list(rng.integers(0, 12, n - len(degs))), np.int64)
    rng.shuffle(degs)  # long and short rows interleave
    dst = np.repeat(np.arange(n), degs)
    # random sources from three quarters of the nodes, some of them much more often than others:
    # out-degrees from 0 to well past any backward chunk
    pool = rng.choice(n, 3 * n // 4, replace=False)
    p = 1.0 / (1.0 + np.arange(len(pool))) ** 0.8
    src = rng.choice(pool, len(dst), p=p / p.sum())
    order = rng.permutation(len(dst))
    return src[order].astype(np.int64), dst[order].astype(np.int64), degs


@functools.lru_cache(maxsize=None)
def ladder_graph(chunk=None, chunk_bwd=None, seed=0):
    """About 150 nodes whose in-degrees cover every boundary of the sum kernel by construction:
    0, 1, 2, 3, 5, 7, 8, 9 (the U = 4 / 8 edge gather), 15 to 17, 63 to 65 and 127 to 129 (the
    64-edge window), c - 1, c, c + 1 and 2c + 1 (whole and barely split rows) and 8c, 8c + 1,
    20c + 3 (merges of 8, 9 and 21 slots) for the forward chunk c. Sources are random, so some
    nodes have no out-edge. The builder asserts all of it."""
    import plagnn

    c = _default_chunk() if chunk is None else chunk
    src, dst, degs = ladder_coo(c, seed)
    n = len(degs)
    g = plagnn.CSRGraph(src, dst, n, chunk=c, chunk_bwd=chunk_bwd)
    assert (g.in_degrees() == degs).all() and g.fwd.chunk == c
    assert (g.out_degrees() == 0).any(), "the out-CSR must have empty rows"
    for d in (0, 1, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, c - 1, c, c + 1):
        assert (degs == d).any(), d
    ns = g.fwd.merges.reshape(-1, 4)[:g.fwd.n_merges, 2]
    assert g.fwd.n_merges >= 3
    assert (ns < 8).any() and (ns == 8).any() and (ns == 9).any() and (ns >= 20).any(), sorted(ns)
    assert n <= 160 and degs.max() == max(129, 20 * c + 3)
    return g


@functools.lru_cache(maxsize=None)
def rect_graph():
    """90 sources, 40 destinations (CSRGraph.from_in_csr), chunks 8 / 4 so both directions
    split rows; some sources have no out-edge and some destinations no in-edge."""
    import plagnn

    rng = np.random.default_rng(5)
    deg = rng.integers(0, 30, 40)
    deg[[3, 17]] = 0
    ptr = np.concatenate([[0], np.cumsum(deg)])
    col = rng.choice(rng.choice(90, 60, replace=False), int(ptr[-1]))
    g = plagnn.CSRGraph.from_in_csr(ptr, col, 90, chunk=8, chunk_bwd=4)
    assert (g.num_src, g.num_dst) == (90, 40)
    assert (g.out_degrees() == 0).any() and (g.in_degrees() == 0).any()
    assert g.fwd.n_merges > 0 and g.bwd.n_merges > 0
    return g


# ------------------------------------------------------------------ one case
def operands(csr, F, seed=0):
    """(X, w): normal features for the rows `csr` gathers, weights of mixed sign in slot order."""
    rng = np.random.default_rng(1000 * seed + F)
    X = rng.standard_normal((csr.n_cols, F)).astype(np.float32)
    w = rng.uniform(-1.0, 2.0, csr.nnz).astype(np.float32)
    return X, w


_refs = {}


def references(g, transpose, X, w, norm_mode, split, key=None):
    """(ref64, bar, piecewise32) of one case, computed once per `key` and never modified."""
    if key is not None and key in _refs:
        return _refs[key]
    csr = g.bwd if transpose else g.fwd
    norm_ptr = g.fwd.ptr if norm_mode == 2 else None
    ref, bar = sum_ref64(csr, X, w, norm_mode, norm_ptr)
    want = sum_piecewise32(csr, X, w, norm_mode, norm_ptr, split)
    for a in (ref, bar, want):
        a.setflags(write=False)
    if key is not None:
        _refs[key] = (ref, bar, want)
    return ref, bar, want


def run_case(dev, g, F, name, mean=False, weighted=False, transpose=False, seed=0, X=None, w=None,
             finite=True):
    """ops.spmm_sum on `dev`: (a) within the float64 bar, (b) bitwise the restated order (the
    schedule's on the GPU, whole rows on the CPU), (c) a second call gives the same bits.
    Returns (result tensor on the CPU, X, w). finite=False: the inputs hold inf / NaN; (a) is
    skipped and every NaN equals every NaN in (b) and (c)."""
    from plagnn import ops

    csr = g.bwd if transpose else g.fwd
    key = None
    if X is None:
        X, w0 = operands(csr, F, seed)
        w = w0 if weighted else None
        key = (id(g), transpose, F, seed, mean, weighted, dev != "cpu")
    norm_mode = (2 if transpose else 1) if mean else 0
    dg = g.on(dev)
    Xt = sc.to_dev(X, dev)
    wt = None if w is None else sc.to_dev(w, dev)
    got = ops.spmm_sum(dg, Xt, mean=mean, ew_slots=wt, transpose=transpose)
    again = ops.spmm_sum(dg, Xt, mean=mean, ew_slots=wt, transpose=transpose)
    assert tuple(got.shape) == (csr.n_rows, F) and got.dtype == torch.float32
    ref, bar, want = references(g, transpose, X, w, norm_mode, dev != "cpu", key)
    if finite:
        sc.assert_within(got, ref, bar, name)
    assert_bits(got, want, name + ": against the restated order", nan_equal=not finite)
    assert_bits(again, got, name + ": second call", nan_equal=not finite)
    return got.cpu(), X, w


# ------------------------------------------------------------------ the checks
def check_width(dev, F, form):
    mean, weighted = FORMS[form]
    run_case(dev, ladder_graph(), F, f"{form} F={F}", mean=mean, weighted=weighted)


def check_transposed(dev, F, mean, weighted, chunk_bwd):
    g = ladder_graph() if chunk_bwd is None else ladder_graph(chunk_bwd=chunk_bwd)
    if chunk_bwd == 4:  # nearly every source row splits
        assert g.bwd.n_merges >= g.num_src / 4, (g.bwd.n_merges, g.num_src)
    assert g.bwd.n_merges > 0
    run_case(dev, g, F, f"transposed mean={mean} weighted={weighted} chunk_bwd={chunk_bwd} F={F}",
             mean=mean, weighted=weighted, transpose=True, seed=1)


def check_item_lengths(dev, chunk, F):
    """CSRGraph(chunk=4): item lengths 1 to 4, all below the U-edge gather; chunk=64: items of
    exactly one 64-edge window."""
    g = ladder_graph(chunk=chunk)
    length = np.diff(g.fwd.items.reshape(-1, 4)[:g.fwd.n_items, 1:3], axis=1).ravel()
    assert length.max() == chunk and ({1, 2, 3, 4} if chunk == 4 else {chunk}) <= set(length.tolist())
    assert ((length == chunk) & (g.fwd.items.reshape(-1, 4)[:g.fwd.n_items, 3] >= 0)).any()
    run_case(dev, g, F, f"chunk {chunk} plain F={F}", seed=2)
    run_case(dev, g, F, f"chunk {chunk} weighted mean F={F}", mean=True, weighted=True, seed=2)


def _strided(t, extra, dev, fill=0.0):
    """A copy of the 2-D tensor t in a buffer with a row stride of t.shape[1] + extra."""
    n, F = t.shape
    buf = torch.full((n, F + extra), fill, device=dev)
    buf[:, :F] = t
    return buf[:, :F]


def _offset4(t, dev, fill=0.0):
    """A contiguous copy of t whose base pointer is 4 bytes past a 16-byte boundary."""
    n, F = t.shape
    flat = torch.full((n * F + 1,), fill, device=dev)
    v = flat[1:].view(n, F)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def check_unaligned(dev, F, transpose):
    """A row stride of F + 1 (X, out, both) and a base pointer 4 bytes off (X, out) take the
    scalar path; the per-feature order does not depend on the path, so the bits stay."""
    from plagnn import ops

    g = ladder_graph()
    base, X, w = run_case(dev, g, F, f"aligned F={F} transpose={transpose}", mean=True, weighted=True,
                          transpose=transpose, seed=3)
    dg = g.on(dev)
    Xt, wt = sc.to_dev(X, dev), sc.to_dev(w, dev)
    n_out = base.shape[0]
    nan = float("nan")
    fresh = lambda: torch.full((n_out, F), nan, device=dev)  # noqa: E731
    variants = {
        "X stride F+1": (_strided(Xt, 1, dev), fresh()),
        "out stride F+1": (Xt, _strided(fresh(), 1, dev, nan)),
        "both strides F+1": (_strided(Xt, 1, dev), _strided(fresh(), 1, dev, nan)),
        "X base + 4 B": (_offset4(Xt, dev), fresh()),
        "out base + 4 B": (Xt, _offset4(fresh(), dev, nan)),
    }
    for name, (Xv, outv) in variants.items():
        r = ops.spmm_sum(dg, Xv, mean=True, ew_slots=wt, transpose=transpose, out=outv)
        assert r.data_ptr() == outv.data_ptr()
        assert_bits(outv, base, f"{name}, F={F} transpose={transpose}")


SENTINEL = -7.25


def check_strided_guards(dev, F, off, transpose):
    """`out` as a column window of a buffer full of a sentinel, X as a column window of a buffer
    full of NaN: nothing outside the window is written or read, everything inside is written."""
    from plagnn import ops

    g = ladder_graph(chunk=64)
    csr = g.bwd if transpose else g.fwd
    base, X, w = run_case(dev, g, F, f"plain call F={F} transpose={transpose}", mean=True, weighted=True,
                          transpose=transpose, seed=4)
    assert np.isfinite(base.numpy()).all()
    dg = g.on(dev)
    wt = sc.to_dev(w, dev)
    width = off + F + 3
    if off % 4 == 0:
        width = (width + 3) // 4 * 4  # ld a multiple of 4: a window of F % 4 == 0 columns stays 16-byte aligned
    else:
        width += (width + 1) % 2  # an odd ld
    Xbuf = torch.full((csr.n_cols, width), float("nan"), device=dev)
    Xbuf[:, off:off + F] = sc.to_dev(X, dev)
    obuf = torch.full((csr.n_rows, width), SENTINEL, device=dev)
    obuf[:, off:off + F] = float("nan")  # rows without entries included: they must read +0
    ops.spmm_sum(dg, Xbuf[:, off:off + F], mean=True, ew_slots=wt, transpose=transpose, out=obuf[:, off:off + F])
    o = obuf.cpu().numpy()
    name = f"window at {off} of {width}, F={F} transpose={transpose}"
    assert (o[:, :off] == SENTINEL).all() and (o[:, off + F:] == SENTINEL).all(), name + ": a guard column was written"
    inside = o[:, off:off + F]
    assert np.isfinite(inside).all(), name + ": an element was not written, or a guard column was read"
    assert_bits(inside, base, name)
    empty = np.diff(csr.ptr) == 0
    assert empty.any() and (np.ascontiguousarray(inside[empty]).view(np.int32) == 0).all(), name + ": empty rows read +0"


def check_rect(dev, F):
    g = rect_graph()
    for transpose in (False, True):
        for mean in (False, True):
            run_case(dev, g, F, f"rect transpose={transpose} mean={mean} F={F}", mean=mean, weighted=True,
                     transpose=transpose, seed=5)


def check_empty_shapes(dev):
    import plagnn
    from plagnn import ops

    g0 = plagnn.CSRGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    for transpose in (False, True):
        for mean in (False, True):
            out = torch.full((5, 8), float("nan"), device=dev)
            ops.spmm_sum(g0.on(dev), torch.ones(5, 8, device=dev), mean=mean, transpose=transpose, out=out)
            assert (out.cpu().numpy().view(np.int32) == 0).all(), "an edgeless graph gives +0"
    g = ladder_graph(chunk=64)
    out = ops.spmm_sum(g.on(dev), torch.ones(g.num_nodes, 0, device=dev), mean=True)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert tuple(out.shape) == (g.num_nodes, 0)
    # every edge enters row 0 (two slots at the default chunk); every other row is empty
    rng = np.random.default_rng(6)
    g1 = plagnn.CSRGraph(rng.integers(0, 20, 300), np.zeros(300, np.int64), 20)
    assert g1.fwd.n_merges == 1 and (g1.in_degrees()[1:] == 0).all()
    for transpose in (False, True):
        run_case(dev, g1, 12, f"one row, transpose={transpose}", mean=True, weighted=True, transpose=transpose, seed=6)


def check_nonfinite(dev, F, transpose):
    """One input row +inf, one NaN, one weight 0 on an entry that gathers the +inf row (inf * 0
    = NaN): bitwise the restated order up to NaN payloads, and only the rows that aggregate
    those inputs are touched."""
    g = ladder_graph(chunk=64)
    csr = g.bwd if transpose else g.fwd
    X, w = operands(csr, F, seed=7)
    X, w = X.copy(), w.copy()
    cnt = np.bincount(csr.col, minlength=csr.n_cols)
    used = [int(i) for i in np.argsort(cnt, kind="stable") if cnt[i] > 0]  # gathered by the fewest rows
    a, b = used[0], used[1]
    X[a], X[b] = np.inf, np.nan
    k = int(np.flatnonzero(csr.col == a)[0])
    w[_coef_index(csr)[k]] = 0.0
    row_of = np.repeat(np.arange(csr.n_rows), np.diff(csr.ptr))
    hit = np.zeros(csr.n_rows, bool)
    hit[row_of[(csr.col == a) | (csr.col == b)]] = True
    assert hit.any() and not hit.all()
    for mean in (False, True):
        got, _, _ = run_case(dev, g, F, f"non-finite F={F} transpose={transpose} mean={mean}", mean=mean,
                             transpose=transpose, X=X, w=w, finite=False)
        fin = np.isfinite(got.numpy()).all(1)
        assert (fin == ~hit).all(), "non-finite values reach exactly the rows that aggregate them"
        assert np.isnan(got.numpy()[row_of[k]]).all(), "inf * 0 is NaN"


def check_autograd(dev, F, mean):
    """ops.SumAggregate with a weight that requires grad against float64 autograd on the
    edge list: the layers' path at the widths of the kernel-level sweep."""
    from plagnn import ops

    g = ladder_graph()
    src, dst, _ = ladder_coo(g.fwd.chunk)
    n = g.num_nodes
    dg = g.on(dev)
    rng = np.random.default_rng(F)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(-1.0, 2.0, len(src)).astype(np.float32))
    dZ = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    xd, wd = sc._leaf(x, dev), sc._leaf(w, dev)
    y = ops.SumAggregate.apply(xd, dg, dg.edge_weight_slots(wd), mean)
    y.backward(dZ.to(dev))
    x64, w64 = sc._leaf(x, dtype=torch.float64), sc._leaf(w, dtype=torch.float64)
    y64 = sc.agg_sum64(torch.from_numpy(src), torch.from_numpy(dst), n, x64, w64, mean)
    y64.backward(dZ.double())
    sc.close(y, y64, 1e-5, "out")
    sc.close(xd.grad, x64.grad, 1e-5, "d feat")
    sc.close(wd.grad, w64.grad, 1e-5, "d edge weight")


def check_error_returns(dev):
    """The C-ABI's argument checks (nothing is launched) and the wrapper's row check."""
    from plagnn import _lib, ops
    from plagnn._lib import ptr

    g = ladder_graph(chunk=64)
    dg = g.on(dev)
    s = dg.fwd.struct(None)
    n, F = g.num_nodes, 8
    X, out = torch.zeros(n, F, device=dev), torch.zeros(n, F, device=dev)
    gpu = dev != "cpu"
    name = "pg_spmm_sum" if gpu else "pg_spmm_sum_cpu"
    if gpu:
        ws_n = _lib.lib().pg_spmm_sum_workspace(s, F)
        assert g.fwd.n_slots > 0 and ws_n > 0
        ws = torch.zeros(ws_n, dtype=torch.uint8, device=dev)
        tail = lambda nbytes=ws_n: (ptr(ws), nbytes, None)  # noqa: E731
    else:
        tail = lambda: ()  # noqa: E731
    invalid, workspace = r"\(code -1\)", r"\(code -3\)"
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*leading"):
        _lib.call(name, s, ptr(X), F - 1, F, 0, None, ptr(out), F, *tail())
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*leading"):
        _lib.call(name, s, ptr(X), F, F, 0, None, ptr(out), F - 1, *tail())
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*norm_mode"):
        _lib.call(name, s, ptr(X), F, F, 3, None, ptr(out), F, *tail())
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*norm_mode"):
        _lib.call(name, s, ptr(X), F, F, 2, None, ptr(out), F, *tail())
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*NULL"):
        _lib.call(name, s, None, F, F, 0, None, ptr(out), F, *tail())
    with pytest.raises(_lib.PlagnnError, match=invalid + ".*NULL"):
        _lib.call(name, s, ptr(X), F, F, 0, None, None, F, *tail())
    _lib.call(name, s, None, F, 0, 0, None, None, F, *tail())  # F = 0: no buffer is touched
    if gpu:
        with pytest.raises(_lib.PlagnnError, match=workspace + ".*workspace"):
            _lib.call(name, s, ptr(X), F, F, 0, None, ptr(out), F, *tail(ws_n - 1))
    with pytest.raises(ValueError, match="rows"):
        ops.spmm_sum(dg, torch.zeros(n + 1, F, device=dev))
    with pytest.raises(ValueError, match="rows"):
        ops.spmm_sum(dg, torch.zeros(n - 1, F, device=dev), transpose=True)
