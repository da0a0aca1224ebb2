"""pg_csr_spmm_f64 at its entry point, bitwise against tests/preproc_common.py's two references:
(a) integer data, where a dense product is exact, and (b) float32-valued data, where every
product is exact in float64 and the reference adds a row's entries in CSR order, so the
header's "sum in CSR order" is held to the bit (the reversed order gives other bits in more
than half of the outputs of the longer rows; asserted).

Every k at a chunk edge (NCH = 1..4, odd and even, k = 1) runs on the double2 path (X on a
16-byte boundary, even ldx; for odd k that makes ldx > k and the last column a lone one) and on
the scalar path reached three ways: an odd contiguous ldx, X eight bytes past a 16-byte
boundary, and an even k in rows of odd length k + 1. X's padding columns hold NaN, Y has
ldy = k + 3 and must keep its sentinel there. The matrix is rectangular with rows of 0 to 200
entries (window edges at 64 and 128, the 4-row unroll's remainders). All four (u, v)
combinations run; (u, NULL) means no rank-1 term.

The front end runs once with an odd column count (components = 61: 71 columns), which puts
every product of the randomized SVD on the scalar path.

Measured on an MI355X: the file (49 tests, about 750 launches) takes about 3.2 s of wall
time, 2 s of it start-up; the front-end test is the slowest on the GPU side at 0.4 s, plus the
CPU oracle's dense randomized SVD.

Tried against deliberately wrong kernels (scratch builds, this file only): subtracting v[f + i]
without ur, and adding each group of four window entries in reverse order: 47 of 49 tests
fail either way. The two that pass are the one that launches nothing and the front end, which
cannot see either: its bar is 1e-7, and its only product with a u (Xc^T Q) multiplies it by
1^T Q, which is zero up to rounding for any Q in the range of the column-centred matrix. Only
the ABI cases hold the rank-1 term.
"""
import numpy as np
import pytest
import torch

import preproc_common as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -768.25
KS = [1, 2, 3, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512]
UV = [(0, 0), (0, 1), (1, 1), (1, 0)]


def _layout(k, path):
    """(ldx, offset of X in doubles from a 16-byte boundary), None where the path needs the
    other parity of k."""
    if path == "vec":
        return k + (k & 1), 0
    if path == "odd_ld":
        return (k, 0) if k & 1 else None
    if path == "off8":
        return k + (k & 1), 1
    return (k + 1, 0) if not k & 1 else None  # "even_k_odd_ld"


LAYOUTS = [(k, p) for k in KS for p in ("vec", "odd_ld", "off8", "even_k_odd_ld") if _layout(k, p)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Dev:
    """A preproc_common.spmm_case on the device with X laid out as asked."""

    def __init__(self, c, ldx, off):
        self.c = c
        self.ptr, self.col, self.val = _dev(c["ptr"]), _dev(c["col"]), _dev(c["val"])
        self.u, self.v = _dev(c["u"]), _dev(c["v"])
        host = np.full(c["n_src"] * ldx + 2, np.nan)
        host[off:off + c["n_src"] * ldx].reshape(c["n_src"], ldx)[:, :c["k"]] = c["X"]
        self.xbuf = _dev(host)
        assert self.xbuf.data_ptr() % 16 == 0
        self.x_ptr = self.xbuf.data_ptr() + 8 * off
        self.ldx = ldx
        self.vec = self.x_ptr % 16 == 0 and ldx % 2 == 0

    def run(self, use_u, use_v):
        from plagnn import _lib

        c = self.c
        n_rows, k = c["n_rows"], c["k"]
        ldy = k + 3
        Y = torch.full((n_rows + 1, ldy), SENT, dtype=torch.float64, device=DEV)
        _lib.call("pg_csr_spmm_f64", n_rows, self.ptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(),
                  self.x_ptr, self.ldx, k, self.u.data_ptr() if use_u else None,
                  self.v.data_ptr() if use_v else None, Y.data_ptr(), ldy, _lib.stream_handle(Y.device))
        h = Y.cpu().numpy()
        assert (h[:, k:] == SENT).all() and (h[n_rows] == SENT).all(), "written outside Y[:, :k]"
        return h[:n_rows, :k]


def _check(lengths, n_src, k, ldx, off, want_vec, uvs=UV):
    for kind in ("int", "f32"):
        c = P.spmm_case(lengths, n_src, k, kind)
        d = _Dev(c, ldx, off)
        assert d.vec == want_vec
        for use_u, use_v in uvs:
            got = d.run(use_u, use_v)
            ref = P.spmm_ref(c, use_u, use_v, kind)
            np.testing.assert_array_equal(got, ref, err_msg=f"{kind} k={k} ldx={ldx} off={off} u={use_u} v={use_v}")
            if kind == "f32":  # the sequential reference also fixes the sign of a zero (empty rows)
                assert np.array_equal(np.signbit(got), np.signbit(ref))
        if kind == "f32":
            assert P.spmm_order_matters(c) >= 0.5


@pytest.mark.parametrize("k,path", LAYOUTS)
def test_all_widths_and_paths(k, path):
    ldx, off = _layout(k, path)
    _check(P.SPMM_ROW_LENGTHS, 211, k, ldx, off, want_vec=path == "vec")


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 9])
def test_row_counts_around_the_block(n_rows):
    """Four rows per workgroup: a lone row, a part block, a whole one, one row into the next."""
    for k, (ldx, off) in ((3, (4, 0)), (130, (130, 1)), (257, (257, 0))):
        _check(P.SPMM_SMALL_LENGTHS[:n_rows], 150, k, ldx, off, want_vec=(k == 3), uvs=[(1, 1), (0, 0)])


def _raw(n_rows, k, ldx, ldy, Y):
    from plagnn import _lib

    c = P.spmm_case(P.SPMM_SMALL_LENGTHS[:4], 150, 8, "int")
    d = _Dev(c, 8, 0)
    rc = _lib.lib().pg_csr_spmm_f64(n_rows, d.ptr.data_ptr(), d.col.data_ptr(), d.val.data_ptr(), d.x_ptr, ldx, k,
                                    d.u.data_ptr(), d.v.data_ptr(), Y.data_ptr(), ldy, _lib.stream_handle(Y.device))
    torch.cuda.synchronize()
    return rc


def test_empty_products_and_rejections():
    Y = torch.full((4, 16), SENT, dtype=torch.float64, device=DEV)
    assert _raw(4, 0, 8, 16, Y) == 0 and _raw(0, 8, 8, 16, Y) == 0
    assert _raw(4, 513, 520, 520, Y) == P.PG_ERR_INVALID  # one past four chunks of 128
    assert _raw(4, 8, 7, 16, Y) == P.PG_ERR_INVALID       # ldx < k
    assert _raw(4, 8, 8, 7, Y) == P.PG_ERR_INVALID        # ldy < k
    assert _raw(-1, 8, 8, 16, Y) == P.PG_ERR_INVALID
    assert (Y.cpu().numpy() == SENT).all()


def test_pca_front_end_on_the_scalar_path(oracle_mod):
    """components = 61 on a 700 x 700 sparse matrix: 71 columns, an odd leading dimension in
    every product. tests/test_gpu_pca.py's bars for a general sparse matrix."""
    from scipy.sparse import diags, random as sprandom

    from plagnn.pca import pca

    n, nc = 700, 61
    m = sprandom(n, n, density=0.01, random_state=4, format="csr",
                 data_rvs=np.random.default_rng(4).standard_normal)
    m = (diags(np.r_[np.zeros(5), np.ones(n - 5)]) @ m).tocsr()  # empty rows
    m.eliminate_zeros()
    got = pca(m, nc)
    ora = oracle_mod.pca_randomized(m, nc)
    sv = np.linalg.norm(ora, axis=0)
    gap = np.minimum(np.abs(np.diff(np.r_[np.inf, sv])), np.abs(np.diff(np.r_[sv, 0.0]))) / sv[0]
    sep = gap > 1e-4
    assert sep[:5].all()
    scale = np.abs(ora).max(axis=0)
    assert np.all((np.abs(got - ora).max(axis=0) <= 1e-7 * scale)[sep])
    qa, _ = np.linalg.qr(got)
    qb, _ = np.linalg.qr(ora)
    assert np.linalg.norm(qa @ (qa.T @ qb) - qb) <= 1e-6 * np.sqrt(nc)
