"""The topology perturbation at its entry points: pg_perturb_prepare, pg_perturb_sum,
pg_perturb_count and pg_perturb_fill called through the C ABI on tests/preproc_common.py's
integer-valued inputs, whose numpy reference is exact to the bit (see that module), into
sentinel-filled buffers. Every instantiation S = 2..8 runs; the thresholds sit ON the data
(many pairs have diff == lo_thr or == hi_thr exactly), values before the clip exceed 1 in
both states, the adjacency holds diagonal entries and, in the `val` variant, stored zeros, 2
and -1.

pg_perturb_sum's bar (preproc_common.neumaier_bar). kadd(s, c, x) forms t = fl(s + x) and the
error e of that addition with the larger operand first (Fast2Sum: e is exact in binary
round-to-nearest), then c = fl(c + e). So at every point of the reduction the s registers plus
ALL e produced so far add up to the consumed terms exactly; the only roundings that count are
the additions into the c registers and the final t + tc.
  K = n^2 + 255 n + n + 256 two-sums happen (one per term; 255 per row in sum_kernel's LDS
      tree; one per row and 256 more in final_sum_kernel), each |e| <= u |t| <= u A up to
      higher order, A = sum |term|;
  D = ceil(n/256) + 2*8 + 2*ceil(n/256) + 2*256 bounds the rounded additions any e passes
      through on its way into tc (a thread's column loop; two per tree level; two per row of
      a final thread's run; two per step of the last loop), so
      |tc - sum e| <= D u sum|e| <= K D u^2 A   (terms in u^3: below 1e-10 of this one);
  out = fl(t + tc) adds u |sum|, and math.fsum is itself within u |sum| of the exact sum.
bar = 2 u |sum| + K D u^2 A. At n = 513: K D u^2 = 2.1e-24, so the bar is two roundings of
the result unless the terms cancel to below 1e-8 of their magnitude.

Measured on an MI355X: all 18 sums (S in {2, 3, 8} x n in {33, 257, 513} x both passes) equal
math.fsum bit for bit (error 0, ratio 0 to a bar between 1.2e-15 and 6.1e-11), so the bar's two
roundings are never used up. The file (85 tests) takes about 3 s of wall time, 2 s of it
start-up; no test above 0.2 s.

Tried against deliberately wrong kernels (scratch builds, this file only):
  `d <= lo_thr` in new_value                       39 tests fail
  no clip in pcc                                   16 fail (count/fill, and the sums)
  `w <= wave` in fill_kernel's prefix              46 fail
  kadd without its compensation                    6 of the 9 sum cases fail
  stored zeros read as ones (bitmap and lookup)    23 fail (each `val` case with n > 1, the front end)
  build_bitmap not skipping stored zeros           passes, and must: ppi_value then finds the
      stored 0 by its binary search and returns it, the same v = 0 as for an absent entry. The
      skip saves the search; it is not what makes stored zeros behave.
"""
import numpy as np
import pytest
import torch

import preproc_common as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
SENT_I32 = -77
SENT_I64 = -7777
SENT_F64 = -768.25
TAIL = 512  # sentinel entries kept after the last row of a fill


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Inputs:
    """A preproc_common.perturb_case on the device (standard deviations: the reference's)."""

    def __init__(self, c):
        from plagnn import _lib

        self.c, self.n, self.S = c, c["n"], c["S"]
        self.xn, self.xi, self.sdn, self.sdi = (_dev(c[k]) for k in ("xn", "xi", "sdn", "sdi"))
        self.ptr, self.col = _dev(c["ptr"]), _dev(c["col"]) if len(c["col"]) else torch.zeros(1, dtype=torch.int32,
                                                                                               device=DEV)
        self.val = None if c["val"] is None else (_dev(c["val"]) if len(c["val"]) else
                                                  torch.zeros(1, dtype=torch.int64, device=DEV))
        self.st = _lib.stream_handle(self.xn.device)
        self.base = (self.xn.data_ptr(), self.xi.data_ptr(), self.sdn.data_ptr(), self.sdi.data_ptr(), self.n,
                     self.S, P.inv_fact(self.S))
        self.csr = (self.ptr.data_ptr(), self.col.data_ptr(), _ptr(self.val))


def _count(inp, lo, hi):
    from plagnn import _lib

    counts = torch.full((inp.n + 3,), SENT_I32, dtype=torch.int32, device=DEV)
    _lib.call("pg_perturb_count", *inp.base, *inp.csr, lo, hi, counts.data_ptr(), inp.st)
    h = counts.cpu().numpy()
    assert (h[inp.n:] == SENT_I32).all(), "counts written past n"
    return h[:inp.n]


def _fill(inp, lo, hi, offs, total):
    from plagnn import _lib

    oc = torch.full((total + TAIL,), SENT_I32, dtype=torch.int32, device=DEV)
    ov = torch.full((total + TAIL,), SENT_I64, dtype=torch.int64, device=DEV)
    _lib.call("pg_perturb_fill", *inp.base, *inp.csr, lo, hi, _dev(offs).data_ptr(), oc.data_ptr(),
              ov.data_ptr(), inp.st)
    return oc.cpu().numpy(), ov.cpu().numpy()


def _check_fill(inp, lo, hi, gap):
    """count, then fill at offsets with `gap` unused entries before every row: counts, columns,
    values, order, untouched gaps and tail, and a second call's bits."""
    c, n = inp.c, inp.n
    cnt, cols, vals = P.coo_of(P.perturb_new(c["a"], c["diff"], lo, hi))
    # fill trusts the caller's offsets to leave room for what count reported: compare first
    np.testing.assert_array_equal(_count(inp, lo, hi), cnt)
    start = np.zeros(n + 1, np.int64)
    np.cumsum(cnt.astype(np.int64) + gap, out=start[1:])
    offs = start[:n] + gap
    total = int(start[n])
    exp_c = np.full(total + TAIL, SENT_I32, np.int32)
    exp_v = np.full(total + TAIL, SENT_I64, np.int64)
    where = np.repeat(offs, cnt) + (np.arange(len(cols)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    exp_c[where], exp_v[where] = cols, vals
    got_c, got_v = _fill(inp, lo, hi, offs, total)
    np.testing.assert_array_equal(got_c, exp_c)
    np.testing.assert_array_equal(got_v, exp_v)
    again_c, again_v = _fill(inp, lo, hi, offs, total)
    np.testing.assert_array_equal(again_c, got_c)
    np.testing.assert_array_equal(again_v, got_v)
    return cnt


def _case(n, S, val):
    kw = dict(full_row=100, empty_rows=(0, 200, 201, 202, 512)) if n == 513 else {}
    return P.perturb_case(n, S, S, val=val, strict=n >= 31, **kw)


# ---- pg_perturb_prepare ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("S", range(2, 9))
def test_prepare_sd_bitwise(S, n):
    from plagnn import _lib

    c = P.perturb_case(n, S, S, strict=False)
    xn, xi = _dev(c["xn"]), _dev(c["xi"])
    sdn = torch.full((n + 5,), SENT_F64, dtype=torch.float64, device=DEV)
    sdi = torch.full((n + 5,), SENT_F64, dtype=torch.float64, device=DEV)
    _lib.call("pg_perturb_prepare", xn.data_ptr(), xi.data_ptr(), n, S, P.inv_fact(S), sdn.data_ptr(),
              sdi.data_ptr(), _lib.stream_handle(xn.device))
    for got, ref in ((sdn, c["sdn"]), (sdi, c["sdi"])):
        h = got.cpu().numpy()
        assert (h[n:] == SENT_F64).all()
        np.testing.assert_array_equal(h[:n], ref)
    if n > 1:
        assert (c["sdn"] == 0).any() and (c["sdi"] == 0).any()  # zero rows are there


# ---- pg_perturb_count + pg_perturb_fill ------------------------------------------------
CASES = [(97, S) for S in range(2, 9)] + [(n, S) for n in (1, 31, 32, 33, 256, 257, 513) for S in (3, 8)]


@pytest.mark.parametrize("val", [False, True], ids=["ones", "val"])
@pytest.mark.parametrize("n,S", CASES)
def test_count_fill_bitwise(n, S, val):
    c = _case(n, S, val)
    inp = _Inputs(c)
    a = c["a"]
    if n == 513:
        lens = np.diff(c["ptr"])
        assert lens[100] == 512 and (lens[[0, 200, 201, 202, 512]] == 0).all()
    # thresholds on the data: ties decide `<` against `<=` and `>` against `>=`
    _check_fill(inp, c["lo"], c["hi"], 0)
    _check_fill(inp, c["lo"], c["hi"], 3)
    # nothing fires: the adjacency comes back as stored (explicit zeros dropped)
    cnt = _check_fill(inp, -INF, INF, 0)
    np.testing.assert_array_equal(cnt, (a != 0).sum(axis=1))
    # everything fires: every 1 removed, every 0 set (stored zeros and the diagonal too)
    cnt = _check_fill(inp, INF, -INF, 3)
    np.testing.assert_array_equal(cnt, (a != 1).sum(axis=1))


# ---- pg_perturb_sum --------------------------------------------------------------------
def _sum(inp, squared, mean):
    from plagnn import _lib

    nws = int(_lib.lib().pg_perturb_workspace(inp.n))
    assert nws > 0
    guard = 64
    ws = torch.full((nws + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    tot = torch.full((3,), SENT_F64, dtype=torch.float64, device=DEV)
    _lib.call("pg_perturb_sum", *inp.base, squared, mean, tot[1:2].data_ptr(), ws.data_ptr(), nws, inp.st)
    h = tot.cpu().numpy()
    assert h[0] == SENT_F64 and h[2] == SENT_F64
    assert (ws[nws:].cpu().numpy() == 0xA5).all(), "workspace overrun"
    return float(h[1])


@pytest.mark.parametrize("n", [33, 257, 513])
@pytest.mark.parametrize("S", [2, 3, 8])
def test_sum_within_neumaier_bound(S, n):
    c = P.perturb_case(n, S, S, strict=False)
    inp = _Inputs(c)
    tot = _sum(inp, 0, 0.0)
    mean = tot / (float(n) * float(n))
    for squared, got in ((0, tot), (1, _sum(inp, 1, mean))):
        ref = P.sum_ref(c["diff"], squared, mean)
        bar = P.neumaier_bar(c["diff"], squared, mean, n)
        err = abs(got - ref)
        print(f"pg_perturb_sum S={S} n={n} squared={squared}: sum {ref:.17g} err {err:.3g} "
              f"bar {bar:.3g} ratio {err / bar:.3f}")
        assert err <= bar, (got, ref, bar)
        assert _sum(inp, squared, mean) == got  # deterministic


# ---- the front end on the instantiations it never ran ----------------------------------
@pytest.mark.parametrize("S", [4, 6, 7, 8])
def test_front_end_other_sample_counts(oracle_mod, S):
    """modify_network_topology_expr at n = 150 on lognormal expression rows against the dense
    numpy oracle (tests/test_gpu_perturb.py's bars: adjacency exact, mean / std to 1e-13), with
    a PPI that stores explicit zeros and a duplicated edge (value 2)."""
    from scipy.sparse import coo_matrix

    from plagnn import perturb

    n, thr = 150, 0.9
    rng = np.random.default_rng(40 + S)
    en = rng.lognormal(1.0, 1.0, (n, S))
    ei = en * rng.lognormal(0.0, 0.5, (n, S))
    en[rng.random(n) < 0.2] = 0.0
    ei[rng.random(n) < 0.2] = 0.0
    ei[5] = ei[4]
    up = np.triu(rng.random((n, n)) < 0.05, 1)
    r, c = np.nonzero(up | up.T)
    data = np.ones(len(r), np.int64)
    data[rng.random(len(r)) < 0.1] = 0                       # stored explicit zeros
    data[:3] = 1                                             # ... and three entries stored twice
    r, c, data = np.append(r, r[:3]), np.append(c, c[:3]), np.append(data, [1, 1, 1])
    ppi = coo_matrix((data, (r, c)), shape=(n, n))
    dense = ppi.toarray()
    assert (dense == 2).any() and (data == 0).sum() > 10
    ref, (mean, std) = oracle_mod.modify_network_topology(ppi, oracle_mod.pcc_matrix(en),
                                                          oracle_mod.pcc_matrix(ei), thr)
    got, st = perturb.modify_network_topology_expr(ppi, en, ei, thr, return_stats=True)
    np.testing.assert_allclose([st.mean, st.std], [mean, std], rtol=1e-13, atol=1e-16)
    np.testing.assert_array_equal(got.row, ref.row)
    np.testing.assert_array_equal(got.col, ref.col)
    np.testing.assert_array_equal(got.data, ref.data)
    assert got.data.dtype == np.int64 and (got.data == 2).any()
    assert st.removed > 0 and st.added > 0


# ---- n = 0 and the rejections (all return before any launch) ---------------------------
def _dummies():
    from plagnn import _lib

    d = dict(x=torch.zeros(64, dtype=torch.float64, device=DEV),
             sd=torch.full((8,), SENT_F64, dtype=torch.float64, device=DEV),
             i32=torch.full((8,), SENT_I32, dtype=torch.int32, device=DEV),
             i64=torch.full((8,), SENT_I64, dtype=torch.int64, device=DEV),
             offs=torch.zeros(8, dtype=torch.int64, device=DEV),
             ptr=torch.zeros(8, dtype=torch.int32, device=DEV),
             ws=torch.zeros(4096, dtype=torch.uint8, device=DEV))
    d["st"] = _lib.stream_handle(d["x"].device)
    return d


def _calls(d, n, S, x=True, ws_bytes=4096, total=True, ws=True):
    """name -> argument tuple of the four entry points on the dummy buffers."""
    xp = d["x"].data_ptr() if x else None
    f = 1.0 / max(S - 1, 1)
    base = (xp, d["x"].data_ptr(), d["sd"].data_ptr(), d["sd"].data_ptr(), n, S, f)
    csr = (d["ptr"].data_ptr(), d["ptr"].data_ptr(), None)
    return {
        "pg_perturb_prepare": (xp, d["x"].data_ptr(), n, S, f, d["sd"].data_ptr(), d["sd"].data_ptr(), d["st"]),
        "pg_perturb_sum": (*base, 0, 0.0, d["sd"][0:1].data_ptr() if total else None,
                           d["ws"].data_ptr() if ws else None, ws_bytes, d["st"]),
        "pg_perturb_count": (*base, *csr, -INF, INF, d["i32"].data_ptr(), d["st"]),
        "pg_perturb_fill": (*base, *csr, -INF, INF, d["offs"].data_ptr(), d["i32"].data_ptr(),
                            d["i64"].data_ptr(), d["st"]),
    }


def _rc(name, args):
    from plagnn import _lib

    return getattr(_lib.lib(), name)(*args)


def _untouched(d, sd=True):
    torch.cuda.synchronize()
    assert (d["i32"].cpu().numpy() == SENT_I32).all() and (d["i64"].cpu().numpy() == SENT_I64).all()
    if sd:
        assert (d["sd"].cpu().numpy() == SENT_F64).all()


def test_n_zero():
    d = _dummies()
    for name, args in _calls(d, 0, 3).items():
        if name != "pg_perturb_sum":
            assert _rc(name, args) == 0
    _untouched(d)
    assert _rc("pg_perturb_sum", _calls(d, 0, 3)["pg_perturb_sum"]) == 0
    torch.cuda.synchronize()
    h = d["sd"].cpu().numpy()
    assert h[0] == 0.0 and np.signbit(h[0]) == 0 and (h[1:] == SENT_F64).all()
    from plagnn import _lib

    assert int(_lib.lib().pg_perturb_workspace(0)) == 0


def test_rejections_before_launch():
    from plagnn import _lib

    d = _dummies()
    for n, S in ((4, 1), (4, 9), (-1, 3)):
        for name, args in _calls(d, n, S).items():
            assert _rc(name, args) == P.PG_ERR_INVALID, (name, n, S)
    for name, args in _calls(d, 4, 3, x=False).items():  # a NULL input with n > 0
        assert _rc(name, args) == P.PG_ERR_INVALID, name
    assert _rc("pg_perturb_sum", _calls(d, 4, 3, total=False)["pg_perturb_sum"]) == P.PG_ERR_INVALID
    need = int(_lib.lib().pg_perturb_workspace(4))
    assert 0 < need <= 4096
    assert _rc("pg_perturb_sum", _calls(d, 4, 3, ws_bytes=need - 1)["pg_perturb_sum"]) == P.PG_ERR_WORKSPACE
    assert _rc("pg_perturb_sum", _calls(d, 4, 3, ws=False)["pg_perturb_sum"]) == P.PG_ERR_WORKSPACE
    big = _calls(d, 1310721, 3)  # one past the largest row bitmap (160 KB of LDS)
    assert _rc("pg_perturb_count", big["pg_perturb_count"]) == P.PG_ERR_INVALID
    assert _rc("pg_perturb_fill", big["pg_perturb_fill"]) == P.PG_ERR_INVALID
    assert b"pg_perturb_fill" in _lib.lib().pg_last_error_string()
    _untouched(d)
