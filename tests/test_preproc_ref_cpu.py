"""Pins tests/preproc_common.py's references before the GPU tests rely on them.

* oracle.edge_clustering_coefficients equals the reference's own output on weighted graphs
  with diagonal entries (tests/golden/ecc_weighted.npz, epsilon = 0.25), entry for entry in
  the reference's order, bit for bit.
* The numpy perturbation reference equals the streaming C oracle (oracle_perturb_sd,
  oracle_perturb_rows; pinned to the reference by tests/golden/perturb.npz) bit for bit for
  S = 2..8, with and without stored values (stored zeros, 2, -1), at the tie thresholds and
  at both infinite pairs; the C oracle's compensated sums sit inside the Neumaier bound of
  math.fsum.
* oracle_perturb_sd equals sqrt(diag(np.cov(x))) bit for bit for S = 2..8: the fma-chain
  statement of numpy's order holds for every sample count the kernels are built for.
* SpMM reference (a) equals scipy's product exactly, (b) within float64 rounding, and (b)
  really depends on the order.
"""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp

import preproc_common as P
from conftest import ROOT

_f64p = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def test_oracle_ecc_matches_reference_on_weighted_graphs(oracle_mod):
    import os

    z = np.load(os.path.join(ROOT, "tests", "golden", "ecc_weighted.npz"))
    r, c, w, n = P.weighted_graph()
    np.testing.assert_array_equal(r, z["row"])
    np.testing.assert_array_equal(c, z["col"])
    assert n == int(z["n"]) <= 80
    assert 0.2 <= (r == c).sum() / n <= 0.4  # diagonal entries on about 30 % of the nodes
    for name, scale in (("w", 1.0), ("half", 0.5)):
        np.testing.assert_array_equal(w * scale, z[f"{name}_val"])
        got = oracle_mod.edge_clustering_coefficients(sp.coo_matrix((w * scale, (r, c)), shape=(n, n)),
                                                      epsilon=float(z["epsilon"]))
        np.testing.assert_array_equal(got.row, z[f"{name}_ecc_row"])
        np.testing.assert_array_equal(got.col, z[f"{name}_ecc_col"])
        np.testing.assert_array_equal(got.data, z[f"{name}_ecc_val"])
        assert (got.data == float(z["epsilon"])).any()  # possible == 0 occurs


def _oracle_rows(L, c, lo, hi):
    n, S = c["n"], c["S"]
    f = P.inv_fact(S)
    ptr, col = c["ptr"].astype(np.int64), c["col"].astype(np.int64)
    cap = n * n
    rr, cc, vv = (np.empty(max(cap, 1), np.int64) for _ in range(3))
    m = L.oracle_perturb_rows(_p(c["xn"], _f64p), _p(c["xi"], _f64p), _p(c["sdn"], _f64p), _p(c["sdi"], _f64p),
                              n, S, f, _p(ptr, _i64p), _p(col, _i64p), _p(c["val"], _i64p), lo, hi, 0, n,
                              _p(rr, _i64p), _p(cc, _i64p), _p(vv, _i64p), cap)
    assert m >= 0
    return rr[:m], cc[:m], vv[:m]


@pytest.mark.parametrize("val", [False, True])
@pytest.mark.parametrize("S", range(2, 9))
def test_perturb_ref_equals_stream_oracle(oracle_mod, S, val):
    L = oracle_mod.lib()
    n = 97
    c = P.perturb_case(n, S, S, val=val)
    f = P.inv_fact(S)
    for x, sd in ((c["xn"], c["sdn"]), (c["xi"], c["sdi"])):
        got = np.empty(n)
        L.oracle_perturb_sd(_p(x, _f64p), n, S, f, _p(got, _f64p))
        np.testing.assert_array_equal(got, sd)  # NaN-free: sd of a zero row is 0.0
    inf = float("inf")
    for lo, hi in ((c["lo"], c["hi"]), (-inf, inf), (inf, -inf)):
        cnt, cols, vals = P.coo_of(P.perturb_new(c["a"], c["diff"], lo, hi))
        rr, cc, vv = _oracle_rows(L, c, lo, hi)
        np.testing.assert_array_equal(rr, np.repeat(np.arange(n), cnt))
        np.testing.assert_array_equal(cc, cols)
        np.testing.assert_array_equal(vv, vals)
    # the C oracle's sequential compensated sums against fsum of the reference's terms
    base = (_p(c["xn"], _f64p), _p(c["xi"], _f64p), _p(c["sdn"], _f64p), _p(c["sdi"], _f64p), n, S, f)
    tot = L.oracle_perturb_sum(*base, 0, 0.0, 0, n)
    mean = tot / (float(n) * n)
    tot2 = L.oracle_perturb_sum(*base, 1, mean, 0, n)
    for got, sq in ((tot, 0), (tot2, 1)):
        t = P.sum_terms(c["diff"], sq, mean)
        ref = math.fsum(t)
        # one chain of n^2 exact two-sums whose errors (each <= u sum|t|) are added n^2 deep
        bar = 2 * P.U * (1 + 2 * P.U) * abs(ref) + float(n) ** 4 * P.U ** 2 * math.fsum(np.abs(t))
        assert abs(got - ref) <= bar, (S, sq, got, ref)


@pytest.mark.parametrize("S", range(2, 9))
def test_oracle_sd_equals_numpy_cov_diagonal(oracle_mod, S):
    L = oracle_mod.lib()
    rng = np.random.default_rng(S)
    n = 400
    x = rng.lognormal(1.0, 1.0, (n, S))
    x[rng.random(n) < 0.3] = 0.0
    xc = np.ascontiguousarray(x - x.mean(axis=1)[:, None])
    got = np.empty(n)
    L.oracle_perturb_sd(_p(xc, _f64p), n, S, P.inv_fact(S), _p(got, _f64p))
    np.testing.assert_array_equal(got, np.sqrt(np.diag(np.cov(x))))


@pytest.mark.parametrize("k", [1, 3, 128, 257])
def test_spmm_refs_against_scipy(k):
    for kind in ("int", "f32"):
        c = P.spmm_case(P.SPMM_ROW_LENGTHS, 211, k, kind)
        A = sp.csr_matrix((c["val"], c["col"], c["ptr"]), shape=(c["n_rows"], c["n_src"]))
        prod = A @ c["X"]
        lens = np.diff(c["ptr"])
        assert tuple(lens) == P.SPMM_ROW_LENGTHS
        for use_u, use_v in ((0, 0), (0, 1), (1, 1), (1, 0)):
            ref = P.spmm_ref(c, use_u, use_v, kind)
            full = prod - ((c["u"] if use_u else 1.0) * np.ones(c["n_rows"]))[:, None] * c["v"][None, :] \
                if use_v else prod
            if kind == "int":
                np.testing.assert_array_equal(ref, full)
            else:
                mag = abs(A) @ np.abs(c["X"]) + (np.abs(c["u"])[:, None] + 1.0) * np.abs(c["v"])[None, :]
                assert (np.abs(ref - full) <= 2 * (lens[:, None] + 2) * P.U * mag).all()
        if kind == "f32":
            assert P.spmm_order_matters(c) >= 0.5
            assert not (c["val"] == 0).any() and not (c["X"] == 0).any()
