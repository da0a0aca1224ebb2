"""pg_ecc at its entry point, bitwise against oracle.edge_clustering_coefficients (pinned to the
reference on these input classes by tests/golden/ecc.npz and ecc_weighted.npz). The output is
pre-filled with NaN, so an entry that no row wrote fails; diagonal entries must read 0.0.

Covered here and nowhere else: diagonal entries; weights other than 1 (deg is not the row
length), deg = NULL; order = NULL and an arbitrary order; rows of equal length everywhere (the
id rule alone decides which row owns a pair); epsilon with mostly `possible == 0` pairs; a
700-entry row (three rounds of the 256-stride loops); persistent workgroups that walk many
rows (clearing only their own bits); and the bitmap above 64 KB of LDS up to the largest the
entry point accepts, n = 1 310 720 (160 KB).

n = 1 310 720 launches and is right, so that is the documented limit (include/plagnn.h said
2^22, which the entry point answers with PG_ERR_UNSUPPORTED above 1 310 720).

Measured on an MI355X: the file (15 tests) takes about 2.7 s of wall time, 2 s of it start-up;
the slowest tests are the 600 000-node graph and the power-law graph at under 0.2 s each
(host reference included).

Tried against deliberately wrong kernels (scratch builds, this file only):
  no owner on a length tie (`lj == li` skips)      12 tests fail (NaN left in the output)
  the clearing loop removed                        3 fail (power-law, 600 000, 1 310 720)
  the tie rule turned round (`j < i`)              passes, and must: the pair then belongs to
      the smaller id, which computes the same symmetric count and writes both entries.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import preproc_common as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_MAX = 1310720  # 160 KB of LDS hold one bit per node


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(inp, epsilon, deg=True, order=None):
    from plagnn import _lib

    t = {k: _dev(inp[k]) for k in ("ptr", "col", "mirror", "deg")}
    od = None if order is None else _dev(np.asarray(order, np.int32))
    out = torch.full((inp["nnz"] + 4,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("pg_ecc", t["ptr"].data_ptr(), t["col"].data_ptr(), t["mirror"].data_ptr(),
              t["deg"].data_ptr() if deg else None, None if od is None else od.data_ptr(), inp["n"], inp["nnz"],
              float(epsilon), out.data_ptr(), _lib.stream_handle(out.device))
    h = out.cpu().numpy()
    assert np.isnan(h[inp["nnz"]:]).all(), "written past nnz"
    return h[:inp["nnz"]]


def _longest_first(inp):
    return np.argsort(-np.diff(inp["ptr"]), kind="stable").astype(np.int32)


def _check(oracle_mod, csr, epsilon, orders=("longest",), deg=True):
    inp = P.ecc_inputs(csr)
    exp = P.ecc_expected(oracle_mod, csr, inp, epsilon)
    first = None
    for o in orders:
        order = {"longest": _longest_first(inp), "none": None,
                 "random": np.random.default_rng(5).permutation(inp["n"]).astype(np.int32)}[o]
        got = _run(inp, epsilon, deg=deg, order=order)
        np.testing.assert_array_equal(got, exp)  # NaN (unwritten) != anything: fails
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()
    return inp, exp


@pytest.mark.parametrize("name,scale", [("w", 1.0), ("half", 0.5)])
def test_weighted_with_diagonal_golden(oracle_mod, name, scale):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ecc_weighted.npz"))
    n = int(z["n"])
    csr = sp.coo_matrix((z[f"{name}_val"], (z["row"], z["col"])), shape=(n, n)).tocsr()
    csr.sort_indices()
    inp, exp = _check(oracle_mod, csr, float(z["epsilon"]), orders=("longest", "none"))
    diag = inp["rows"] == inp["col"]
    assert diag.sum() >= 10 and (exp[diag] == 0.0).all()
    assert not np.array_equal(inp["deg"], np.diff(inp["ptr"]))  # the degree is not the length
    # and against the reference's own numbers directly
    key = inp["rows"] * n + inp["col"]
    pos = np.searchsorted(key, z[f"{name}_ecc_row"] * n + z[f"{name}_ecc_col"])
    np.testing.assert_array_equal(exp[pos], z[f"{name}_ecc_val"])


def test_deg_null_is_row_length(oracle_mod):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ecc_weighted.npz"))
    n = int(z["n"])
    csr = sp.coo_matrix((np.ones(len(z["row"])), (z["row"], z["col"])), shape=(n, n)).tocsr()
    csr.sort_indices()
    _check(oracle_mod, csr, 0.25, orders=("longest", "none"), deg=False)


def test_powerlaw_with_loops_any_order(oracle_mod):
    """10 000 rows on at most 2048 persistent workgroups: each walks several rows and must
    leave its bitmap clean; the order of the walk must not show in the result."""
    csr = P.powerlaw_graph(10000, 160000, seed=10000, loop_share=0.1)  # about 61 000 distinct edges
    inp, exp = _check(oracle_mod, csr, 0.0, orders=("longest", "none", "random"))
    assert 110000 < inp["nnz"] < 135000
    assert (inp["rows"] == inp["col"]).sum() > 500 and np.diff(inp["ptr"]).max() > 256
    assert (exp > 0).sum() > 1000


def test_ring_lattice_id_rule(oracle_mod):
    n = 65
    i = np.repeat(np.arange(n), 4)
    j = (i + np.tile(np.arange(1, 5), n)) % n
    csr = P.sym_csr(n, i, j)
    assert (np.diff(csr.indptr) == 8).all()
    _check(oracle_mod, csr, 0.0, orders=("longest", "none", "random"))


def test_star_and_path_epsilon(oracle_mod):
    leaves = np.arange(1, 41)
    path = np.arange(41, 52)
    csr = P.sym_csr(52, np.concatenate([np.zeros(40, np.int64), path[:-1]]), np.concatenate([leaves, path[1:]]))
    inp, exp = _check(oracle_mod, csr, 0.5, orders=("longest", "none"))
    possible = np.minimum(inp["deg"][inp["rows"]], inp["deg"][inp["col"]]) - 1.0
    assert (possible == 0).mean() > 0.5
    np.testing.assert_array_equal(exp[possible == 0], 0.5)


def test_hub_of_700(oracle_mod):
    rng = np.random.default_rng(3)
    n = 800
    r = np.concatenate([np.zeros(700, np.int64), rng.integers(0, n, 3000)])
    c = np.concatenate([np.arange(1, 701), rng.integers(0, n, 3000)])
    csr = P.sym_csr(n, r, c, loops=[0, 5, 799])
    assert np.diff(csr.indptr).max() >= 700
    _check(oracle_mod, csr, 0.0, orders=("longest", "none"))


@pytest.mark.parametrize("n", [2, 33, 64, 65])
def test_small_sizes(oracle_mod, n):
    rng = np.random.default_rng(n)
    m = max(1, n * 3)
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    if n == 2:
        r, c = np.array([0]), np.array([1])
    csr = P.sym_csr(n, r, c, loops=[n - 1])
    _check(oracle_mod, csr, 0.25, orders=("longest", "none"))


def test_single_node_without_entries_touches_nothing():
    inp = dict(ptr=np.zeros(2, np.int32), col=np.zeros(1, np.int32), mirror=np.zeros(1, np.int32),
               deg=np.zeros(1), n=1, nnz=0)
    assert len(_run(inp, 0.5)) == 0  # _run asserts that the whole buffer still holds NaN


def _spread_graph(n, m, seed):
    """About m edges over all ids, node n - 1 included: half of them random pairs, half the
    sides of random triangles (or every value would be 0); a loop on node n - 1."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, n, (m // 6, 3))
    t[0] = (n - 1, n - 2, 0)
    r = np.concatenate([rng.integers(0, n, m // 2), t[:, 0], t[:, 1], t[:, 2], [n - 1]])
    c = np.concatenate([rng.integers(0, n, m // 2), t[:, 1], t[:, 2], t[:, 0], [n // 2]])
    return P.sym_csr(n, r, c, loops=[n - 1])


def test_bitmap_above_64k_lds(oracle_mod):
    """n = 600 000: a 75 000-byte bitmap, two workgroups per CU (512 in all)."""
    n = 600000
    csr = _spread_graph(n, 200000, seed=6)
    inp, exp = _check(oracle_mod, csr, 0.0, orders=("longest", "none"))
    assert inp["col"].max() == n - 1 and (exp > 0).sum() > 1000


def test_largest_accepted_n(oracle_mod):
    """n = 1 310 720: the bitmap is all 160 KB of a CU's LDS."""
    n = N_MAX
    csr = _spread_graph(n, 3000, seed=7)
    inp, exp = _check(oracle_mod, csr, 0.0, orders=("longest", "none"))
    assert inp["col"].max() == n - 1 and (exp > 0).sum() > 100


def test_rejections_before_launch():
    from plagnn import _lib

    ptr = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    st = _lib.stream_handle(out.device)

    def rc(n, nnz=1, p=ptr.data_ptr()):
        return _lib.lib().pg_ecc(p, ptr.data_ptr(), ptr.data_ptr(), None, None, n, nnz, 0.0, out.data_ptr(), st)

    assert rc(N_MAX + 1) == P.PG_ERR_UNSUPPORTED
    assert rc((1 << 22) + 1) == P.PG_ERR_INVALID
    assert rc(-1) == P.PG_ERR_INVALID and rc(4, nnz=-1) == P.PG_ERR_INVALID
    assert rc(4, p=None) == P.PG_ERR_INVALID
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()
