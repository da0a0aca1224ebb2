"""Pins tests/eval_common.py's float32 restatement of pg_loc_correction to the reference's own
function on the CPU, for the cases and seeds tests/test_gpu_eval.py runs: equal to
oracle.protein_loc_correction on every entry outside the rounding margin, with at most 1e-3
of the entries left out (eval_common's margin rule)."""
import numpy as np
import pytest
import torch

import eval_common as E


def _against_oracle(p, alpha):
    import oracle

    got = E.loc_correction_f32(p, alpha)
    ref = oracle.protein_loc_correction(torch.from_numpy(p), alpha).numpy()
    ok, share = E.comparable(p, alpha)
    print(f"left out {share:.2e}, compared {ok.mean():.3f}, all-entry mismatches {int((got != ref).sum())}")
    assert np.array_equal(got[ok], ref[ok])
    assert share <= 1e-3
    return got


@pytest.mark.parametrize("C,n,alpha,seed", E.CASES)
def test_loc_correction_restatement_matches_oracle(C, n, alpha, seed):
    got = _against_oracle(E.make_proba(C, n, seed), alpha)
    if 0.0 < alpha < 1.0 and C > 1 and n > 1:
        assert 0 < got.sum() < got.size          # the case decides something


def test_loc_correction_constant_column_predicts_nothing():
    """max == min in one column: 0 / 0 there, a NaN row sum, every comparison false."""
    got = _against_oracle(E.make_proba(3, 257, 20, const_col=1), 0.2)
    assert not got.any()
