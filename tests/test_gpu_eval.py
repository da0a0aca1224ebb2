"""§8f rank 3: per-epoch evaluation on the GPU vs the reference's own outputs
(tests/golden/eval.npz, made by running code/train.py:19-86) and vs the oracle at the
full S0 size (N = 24,041 rows)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import eval_common as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(ROOT, "tests", "golden", "eval.npz")


@pytest.mark.parametrize("alpha", [0.1, 0.3])
def test_eval_matches_reference_golden(alpha):
    from plagnn import loc_eval

    d = np.load(GOLD)
    pred = loc_eval.protein_loc_correction(torch.from_numpy(d["proba"]).to(DEV), alpha)
    np.testing.assert_array_equal(pred.cpu().numpy(), d[f"pred_{alpha}"])
    perf = np.array(loc_eval.performances_record(torch.from_numpy(d["true"]).to(DEV), pred), np.float64)
    np.testing.assert_array_equal(perf, d[f"perf_{alpha}"])


@pytest.mark.parametrize("alpha", [0.0, 0.2, 0.5])
def test_eval_matches_oracle_full_size(oracle_mod, alpha):
    from plagnn import loc_eval

    rng = np.random.default_rng(5)
    n, C = 24041, 12
    proba = torch.from_numpy(rng.random((n, C)).astype(np.float32))
    true = torch.from_numpy((rng.random((n, C)) < 0.2).astype(np.float32))
    true[true.sum(1) == 0, 3] = 1.0
    pred = loc_eval.protein_loc_correction(proba.to(DEV), alpha)
    ref = oracle_mod.protein_loc_correction(proba, alpha)
    np.testing.assert_array_equal(pred.cpu().numpy(), ref.numpy())
    got = loc_eval.performances_record(true.to(DEV), pred)
    exp = oracle_mod.performances_record(true, ref)
    np.testing.assert_array_equal(np.array(got), np.array(exp))


# ---- through the ABI: both pg_loc_correction kernels (<12> and the generic one), padded
# leading dimensions, n below one 256-row part and at loc_perf_sum_kernel's 2048-row chunk
# boundaries (tests/eval_common.py: the exact float32 restatement, pinned to the oracle by
# tests/test_eval_ref_cpu.py)
SENT = -768.0


def _padded(a, dtype):
    """a [n][C] as the leading columns of a sentinel-filled [n][C + 3] device buffer."""
    buf = torch.full((a.shape[0], a.shape[1] + 3), SENT, dtype=dtype)
    buf[:, :a.shape[1]] = torch.from_numpy(np.asarray(a)).to(dtype)
    return buf.to(DEV)


def _unpad(buf, C):
    h = buf.cpu()
    assert (h[:, C:] == SENT).all(), "padding overwritten"
    return h[:, :C].contiguous().numpy()


def _abi_correction(p, alpha):
    from plagnn import _lib

    n, C = p.shape
    pd = _padded(p, torch.float32)
    pred = torch.full((n, C + 3), SENT, dtype=torch.float64, device=DEV)
    nws = int(_lib.lib().pg_loc_eval_workspace(n, C))
    ws = torch.full((nws,), 255, dtype=torch.uint8, device=DEV)
    _lib.call("pg_loc_correction", pd.data_ptr(), C + 3, n, C, float(alpha), pred.data_ptr(), C + 3,
              ws.data_ptr(), nws, _lib.stream_handle(pd.device))
    torch.cuda.synchronize()
    return _unpad(pred, C)


def _abi_performance(true, pred):
    from plagnn import _lib

    n, C = true.shape
    td, prd = _padded(true, torch.float32), _padded(pred, torch.float64)
    out = torch.full((4,), SENT, dtype=torch.float64, device=DEV)
    nws = int(_lib.lib().pg_loc_eval_workspace(n, C))
    ws = torch.full((nws,), 255, dtype=torch.uint8, device=DEV)
    _lib.call("pg_loc_performance", td.data_ptr(), C + 3, prd.data_ptr(), C + 3, n, C, out.data_ptr(),
              ws.data_ptr(), nws, _lib.stream_handle(td.device))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out[3] == SENT
    return out[:3]


def _perf_equal(oracle_mod, true, pred):
    got = _abi_performance(true, pred)
    exp = np.array(oracle_mod.performances_record(torch.from_numpy(true), torch.from_numpy(pred)), np.float64)
    assert np.array_equal(got, exp, equal_nan=True), (got, exp)
    return exp


@pytest.mark.parametrize("C,n,alpha,seed", E.CASES)
def test_loc_eval_abi_padded_every_class_count(oracle_mod, C, n, alpha, seed):
    p = E.make_proba(C, n, seed)
    pred = _abi_correction(p, alpha)
    np.testing.assert_array_equal(pred, E.loc_correction_f32(p, alpha))       # bit-exact
    ok, share = E.comparable(p, alpha)
    ref = oracle_mod.protein_loc_correction(torch.from_numpy(p), alpha).numpy()
    assert np.array_equal(pred[ok], ref[ok]) and share <= 1e-3
    # performances_record on the kernel's own predictions: every row labelled, no NaN
    true = E.make_true(C, n, seed)
    exp = _perf_equal(oracle_mod, true, pred)
    assert np.isfinite(exp).all()
    # special rows: one with no true label (coverage 0 / 0: the NaN reaches the result as in
    # the oracle), one with no prediction (aim takes no term)
    t2, p2 = true.copy(), pred.copy()
    t2[n // 2] = 0.0
    p2[n // 2] = 1.0
    p2[n // 3] = 0.0
    exp = _perf_equal(oracle_mod, t2, p2)
    assert np.isnan(exp[1]) and np.isfinite(exp[0])


def test_loc_correction_constant_column(oracle_mod):
    """max == min down one column: 0 / 0, a NaN row sum, no prediction anywhere."""
    p = E.make_proba(3, 257, 20, const_col=1)
    pred = _abi_correction(p, 0.2)
    np.testing.assert_array_equal(pred, E.loc_correction_f32(p, 0.2))
    np.testing.assert_array_equal(pred, oracle_mod.protein_loc_correction(torch.from_numpy(p), 0.2).numpy())
    assert not pred.any()
