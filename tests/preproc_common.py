"""References and input builders for the preprocessing kernels' ABI tests (pg_perturb_*,
pg_ecc, pg_csr_spmm_f64). Plain numpy float64 restatements of the contract in
include/plagnn.h, built so that the comparison can be bitwise.

Perturbation. The ABI takes centred rows, so the builder hands it xc = S x - rowsum(x) for
integer x in [-3, 3] (a multiple of the centred row; Pearson's r does not care). Every entry
is an integer of magnitude <= 12 S, every dot product an integer below 2^17: exact in any
summation order, fused or not, so `xc @ xc.T` is the kernel's fma chain bit for bit whatever
BLAS does. Each later step (* inv_fact, / sd_i, / sd_j, sqrt, the subtraction) is one
correctly rounded operation in numpy and in the kernel alike.

Sums. math.fsum of the reference's own terms (correctly rounded); `neumaier_bar` is the bound
a compensated sum of those terms must meet, derived in tests/test_gpu_perturb_abi.py.

f64 SpMM. (a) integer val / X / u / v: every partial sum is an integer, a dense product is
exact. (b) val, X, u, v drawn as float32 and widened: each product w x has a 48-bit
significand and is exact in float64, so fma(w, x, acc) = fl(acc + w x) and numpy's
`acc + w * x` is the same single rounding; the reference adds a row's entries in CSR order.

ECC. The reference is oracle.edge_clustering_coefficients (oracle/ecc_oracle.c), pinned to
the reference's own outputs by tests/golden/ecc.npz and ecc_weighted.npz.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53  # unit roundoff of float64

PG_ERR_INVALID = -1
PG_ERR_UNSUPPORTED = -2
PG_ERR_WORKSPACE = -3


# ---------------------------------------------------------------- perturbation
def inv_fact(S):
    return float(np.true_divide(1, S - 1))  # np.cov: c *= np.true_divide(1, fact)


def pcc_ref(xc, S):
    """(sd [n], pcc [n][n], number of off-diagonal entries with |c| > 1 before the clip)."""
    f = inv_fact(S)
    dot = xc @ xc.T  # small integers: exact
    sd = np.sqrt(np.diag(dot) * f)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = dot * f
        c = c / sd[:, None]
        c = c / sd[None, :]
        over = np.abs(c) > 1.0  # False where NaN
    np.fill_diagonal(over, False)
    c = np.clip(c, -1.0, 1.0)  # NaN kept
    np.fill_diagonal(c, 0.0)
    c[np.isnan(c)] = 0.0
    return sd, c, int(over.sum())


def _mode_nonzero(v):
    """(most frequent non-zero value, how often); (0.0, number of zeros) when there is none."""
    nz = v[v != 0]
    if not len(nz):
        return 0.0, int(len(v))
    u, c = np.unique(nz, return_counts=True)
    k = int(np.argmax(c))
    return float(u[k]), int(c[k])


def perturb_new(a, diff, lo, hi):
    """include/plagnn.h: v' = 0 if v == 1 and diff < lo; 1 if v == 0 and diff > hi; else v."""
    out = a.copy()
    out[(a == 1) & (diff < lo)] = 0
    out[(a == 0) & (diff > hi)] = 1
    return out


def coo_of(dense):
    """(counts per row, columns, values) of the non-zeros, row-major, ascending columns."""
    nz = dense != 0
    return nz.sum(axis=1).astype(np.int32), np.nonzero(nz)[1].astype(np.int32), dense[nz].astype(np.int64)


def _perturb_try(n, S, seed, val, full_row, empty_rows, attempt):
    rng = np.random.default_rng([seed, n, S, int(val), attempt])
    xs = []
    for _ in range(2):
        x = rng.integers(-3, 4, (n, S)).astype(np.float64)
        x[rng.random(n) < 0.15] = 0.0
        # collinear clusters (a row, a copy and a negated copy): r = +-1 up to rounding, the
        # only place where the value before the clip can exceed 1 once S is large
        for _ in range(n // 12):
            b, p, q = rng.choice(n, 3, replace=False)
            x[p], x[q] = x[b], -x[b]
        xs.append(x)
    if n >= 10:
        xs[1][5], xs[1][7], xs[1][9] = xs[1][4], 2.0 * xs[1][6], -xs[1][8]
    xn, xi = (np.ascontiguousarray(S * x - x.sum(axis=1, keepdims=True)) for x in xs)
    sdn, cn, over_n = pcc_ref(xn, S)
    sdi, ci, over_i = pcc_ref(xi, S)
    diff = ci - cn

    m = np.triu(rng.random((n, n)) < 0.2, 1)
    m = m | m.T | np.diag(rng.random(n) < 0.1)
    if full_row >= 0:
        m[full_row] = True
        m[full_row, full_row] = False
    for r in empty_rows:
        m[r] = False
    a = m.astype(np.int64)
    if val:
        a[m] = rng.choice(np.array([0, 1, 2, -1], np.int64), size=int(m.sum()), p=[0.15, 0.55, 0.15, 0.15])
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(m.sum(axis=1), out=ptr[1:])
    col = np.nonzero(m)[1].astype(np.int32)
    vals = a[m].astype(np.int64) if val else None

    lo, tie_lo = _mode_nonzero(diff[a == 1])
    hi, tie_hi = _mode_nonzero(diff[a == 0])
    new = perturb_new(a, diff, lo, hi)
    removed = int(((a == 1) & (new == 0)).sum())
    added = int(((a == 0) & (new == 1)).sum())
    good = (tie_lo >= 3 and tie_hi >= 3 and lo != 0.0 and hi != 0.0 and removed >= 1 and added >= 1 and
            over_n >= 1 and over_i >= 1 and (not val or {0, 1, 2, -1} <= set(vals.tolist())))
    return good, dict(n=n, S=S, xn=xn, xi=xi, sdn=sdn, sdi=sdi, diff=diff, ptr=ptr, col=col, val=vals, a=a,
                      lo=lo, hi=hi, tie_lo=tie_lo, tie_hi=tie_hi, removed=removed, added=added,
                      over=(over_n, over_i), attempt=attempt)


@functools.lru_cache(maxsize=None)
def perturb_case(n, S, seed, val=False, full_row=-1, empty_rows=(), strict=True):
    """One input of the perturbation entry points with its reference, as a dict:
      xn, xi [n][S]   centred integer rows (about 15 % all-zero: NaN -> 0; n // 12 collinear
                      triples per state); in the intervention state also row 5 = row 4,
                      row 7 = 2 row 6, row 9 = -row 8
      sdn, sdi, diff  the reference's standard deviations and pcc_inter - pcc_normal
      ptr, col, val   CSR of a symmetric adjacency at about 20 % density with some diagonal
                      entries; val None (all ones) or int64 in {0 (stored), 1, 2, -1};
                      a [n][n] its dense values
      lo, hi          thresholds ON the data: the most frequent non-zero diff among the pairs
                      with v = 1 (lo) and with v = 0 (hi), so both comparisons' strictness is
                      decided by many pairs (0.0, the diagonal's diff, where there is none)
    strict: the first of up to 64 draws that meets, on the reference alone: >= 3 pairs tied at
    each threshold, >= 1 removed and >= 1 added entry, >= 1 value with |c| > 1 before the clip
    in each state (and all four stored values present); asserts that one does. Not strict
    (sizes too small for these): the first draw. Treat the arrays as read-only."""
    for attempt in range(64 if strict else 1):
        good, c = _perturb_try(n, S, seed, val, full_row, empty_rows, attempt)
        if good or not strict:
            return c
    raise AssertionError(f"perturb_case({n}, {S}, {seed}): no draw meets the conditions")


def sum_terms(diff, squared, mean):
    d = diff.ravel()
    if squared:
        d = d - mean
        d = d * d
    return d


def sum_ref(diff, squared, mean):
    return math.fsum(sum_terms(diff, squared, mean))


def neumaier_bar(diff, squared, mean, n):
    """|compensated sum - fsum| allowed for pg_perturb_sum's reduction over these n^2 terms
    (derivation: tests/test_gpu_perturb_abi.py): the rounding of the final t + tc and the
    reference's own rounding (u |sum| each, taken at the reference with a (1 + 2u) margin for
    where the ulp is measured), plus K D u^2 sum|term| for the D-deep rounded accumulation of
    the K exact two-sum errors."""
    t = sum_terms(diff, squared, mean)
    per = (n + 255) // 256
    K = n * n + 255 * n + n + 256
    D = per + 16 + 2 * per + 512
    return 2.0 * U * (1.0 + 2.0 * U) * abs(math.fsum(t)) + K * D * U * U * math.fsum(np.abs(t))


# ---------------------------------------------------------------- f64 SpMM
SPMM_ROW_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 67, 128, 130, 200)
SPMM_SMALL_LENGTHS = (67, 0, 5, 64, 1, 130, 3, 65, 4)  # its first 1, 3, 4, 5, 9 rows


@functools.lru_cache(maxsize=None)
def spmm_case(lengths, n_src, k, kind, seed=0):
    """CSR rows of the given lengths over n_src source rows (sorted unique columns), X
    [n_src][k], u [n_rows], v [k]. kind "int": integers in [-4, 4]; "f32": float32 normals
    widened to float64 (no zeros). Read-only."""
    rng = np.random.default_rng([seed, len(lengths), n_src, k, kind == "int"])
    ptr = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=ptr[1:])
    col = np.concatenate([np.sort(rng.choice(n_src, L, replace=False)) for L in lengths] +
                         [np.zeros(0, np.int64)]).astype(np.int32)

    def draw(shape):
        if kind == "int":
            return rng.integers(-4, 5, shape).astype(np.float64)
        return rng.standard_normal(shape).astype(np.float32).astype(np.float64)

    return dict(ptr=ptr, col=col, val=draw(len(col)), X=draw((n_src, k)), u=draw(len(lengths)), v=draw(k),
                n_rows=len(lengths), n_src=n_src, k=k)


def _spmm_seq(c, reverse=False):
    ptr, col, val, X = c["ptr"], c["col"], c["val"], c["X"]
    lens = np.diff(ptr)
    acc = np.zeros((c["n_rows"], c["k"]))
    for p in range(int(lens.max()) if len(lens) else 0):
        rows = np.nonzero(lens > p)[0]
        e = ptr[rows] + (lens[rows] - 1 - p if reverse else p)
        acc[rows] = acc[rows] + val[e][:, None] * X[col[e]]  # exact product, one rounding
    return acc


def spmm_ref(c, use_u, use_v, kind):
    """Y = A X - (u or 1) v^T (v None: no term). "int": the dense product (exact); "f32": the
    sum in CSR order, then fl(acc - fl(ur v)) with fl(ur v) exact."""
    if kind == "int":
        A = sp.csr_matrix((c["val"], c["col"], c["ptr"]), shape=(c["n_rows"], c["n_src"])).toarray()
        acc = A @ c["X"]
    else:
        acc = _spmm_seq(c)
    if not use_v:
        return acc
    ur = c["u"] if use_u else np.ones(c["n_rows"])
    return acc - ur[:, None] * c["v"][None, :]


def spmm_order_matters(c):
    """Share of the outputs of rows with >= 8 entries whose CSR-order sum differs from the
    reversed-order sum: the reference pins the order only if this is large."""
    long_rows = np.diff(c["ptr"]) >= 8
    if not long_rows.any():
        return None
    return float((_spmm_seq(c)[long_rows] != _spmm_seq(c, reverse=True)[long_rows]).mean())


# ---------------------------------------------------------------- ECC
def sym_csr(n, r, c, w=None, loops=()):
    """Symmetric float64 CSR with sorted unique columns from undirected pairs (r, c): pairs
    with r == c are dropped, duplicates collapse to one edge of weight w (default 1) stored in
    both directions; loops: node ids that get a diagonal entry of weight 1."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    key, first = np.unique(lo * n + hi, return_index=True)
    lo, hi = key // n, key % n
    wv = np.ones(len(key)) if w is None else np.asarray(w, np.float64)[keep][first]
    loops = np.asarray(loops, np.int64)
    rows = np.concatenate([lo, hi, loops])
    cols = np.concatenate([hi, lo, loops])
    data = np.concatenate([wv, wv, np.ones(len(loops))])
    m = sp.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsr()
    m.sort_indices()
    return m


def ecc_inputs(csr):
    """pg_ecc's arrays from a symmetric CSR: ptr, col, mirror (int32), deg (f64 row sums),
    rows (the row of every entry)."""
    n = csr.shape[0]
    ptr = csr.indptr.astype(np.int32)
    col = csr.indices.astype(np.int32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    key = rows * n + col
    mkey = col.astype(np.int64) * n + rows
    mirror = np.searchsorted(key, mkey)
    assert np.array_equal(key[mirror], mkey), "not symmetric"
    deg = np.bincount(rows, weights=csr.data, minlength=n).astype(np.float64)
    return dict(ptr=ptr, col=col, mirror=mirror.astype(np.int32), deg=deg, rows=rows, n=n, nnz=len(col))


def ecc_expected(oracle_mod, csr, inp, epsilon):
    """The oracle's value at every stored entry, in CSR order; 0.0 on the diagonal. Asserts
    that the oracle emitted each off-diagonal entry exactly once."""
    n = inp["n"]
    ref = oracle_mod.edge_clustering_coefficients(csr, epsilon=epsilon)
    key = inp["rows"] * n + inp["col"]
    pos = np.searchsorted(key, ref.row.astype(np.int64) * n + ref.col)
    exp = np.zeros(inp["nnz"])
    hits = np.zeros(inp["nnz"], np.int64)
    np.add.at(hits, pos, 1)
    offdiag = inp["rows"] != inp["col"]
    assert np.array_equal(hits, offdiag.astype(np.int64))
    exp[pos] = ref.data
    return exp


def powerlaw_graph(n, m, seed, loop_share=0.0):
    """tests/test_gpu_ecc.py's power-law graph, plus self-loops on a share of the nodes."""
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.1, n) + 1.0
    p = w / w.sum()
    s, d = rng.choice(n, m, p=p), rng.choice(n, m, p=p)
    loops = np.nonzero(rng.random(n) < loop_share)[0]
    return sym_csr(n, s, d, loops=loops)


def weighted_graph(n=72, seed=21):
    """ecc_weighted.npz's input: symmetric weights in {1, 2, 3} at about 8 % density, diagonal
    entries (weight 1, 2 or 3) on about 30 % of the nodes. COO (row, col, val)."""
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((n, n)) < 0.08, 1)
    w = np.where(up, rng.integers(1, 4, (n, n)), 0)
    w = w + w.T + np.diag(np.where(rng.random(n) < 0.3, rng.integers(1, 4, n), 0))
    r, c = np.nonzero(w)
    return r.astype(np.int64), c.astype(np.int64), w[r, c].astype(np.float64), n
