"""pg_gemm_f32_rows (the three-piece product on a list of rows) against pg_gemm_f32 on the
whole matrix: listed rows of C bitwise equal, every other row still the NaN written before.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 300
UNSUPPORTED = -2


def _rows_call(A, B, C, rows, transb, n_rows=None):
    from plagnn import _lib
    from plagnn._lib import ptr

    K = A.shape[1]
    N = B.shape[0] if transb else B.shape[1]
    rc = _lib.lib().pg_gemm_f32_rows(int(transb), A.shape[0], N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C),
                                     C.stride(0), ptr(rows), len(rows) if n_rows is None else n_rows,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _operands(K, N, transb, seed):
    rng = np.random.default_rng(seed)
    A = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.standard_normal((N, K) if transb else (K, N)).astype(np.float32)).to(DEV)
    return A, B


def _listed(seed):
    """131 of the 300 rows, sorted, with row 0 and row 299 (the ragged last row tile)."""
    rng = np.random.default_rng(seed)
    inner = rng.choice(np.arange(1, M - 1), 129, replace=False)
    rows = np.sort(np.concatenate([[0, M - 1], inner])).astype(np.int32)
    assert len(rows) == 131 and len(np.unique(rows)) == 131
    return rows


@pytest.mark.parametrize("K", [256, 40])
@pytest.mark.parametrize("N", [256, 72])
@pytest.mark.parametrize("transb", [False, True])
def test_gemm_rows_bitwise(K, N, transb):
    from plagnn import ops

    A, B = _operands(K, N, transb, K + N + transb)
    full = ops.gemm(A, B, transb=transb, split_k=1)
    rows = _listed(K + N)
    rows_d = torch.from_numpy(rows).to(DEV)
    C = torch.full((M, N), float("nan"), device=DEV)
    assert _rows_call(A, B, C, rows_d, transb) == 0
    listed = torch.zeros(M, dtype=torch.bool, device=DEV)
    listed[rows_d.long()] = True
    assert torch.equal(C[listed].view(torch.int32), full[listed].view(torch.int32))
    assert torch.isnan(C[~listed]).all()
    # the list of all rows is the full product
    every = torch.arange(M, dtype=torch.int32, device=DEV)
    C2 = torch.full((M, N), float("nan"), device=DEV)
    assert _rows_call(A, B, C2, every, transb) == 0
    assert torch.equal(C2.view(torch.int32), full.view(torch.int32))


def test_gemm_rows_empty_and_unaligned():
    A, B = _operands(40, 72, False, 5)
    rows_d = torch.from_numpy(_listed(5)).to(DEV)
    C = torch.full((M, 72), float("nan"), device=DEV)
    assert _rows_call(A, B, C, rows_d, False, n_rows=0) == 0  # the empty list writes nothing
    assert torch.isnan(C).all()
    # an operand the three-piece kernel does not take: A 4 bytes off a 16-byte boundary
    flat = torch.zeros(M * 40 + 4, device=DEV)
    A_off = flat[1:1 + M * 40].view(M, 40)
    assert A_off.data_ptr() % 16 != 0
    assert _rows_call(A_off, B, C, rows_d, False) == UNSUPPORTED
    assert torch.isnan(C).all()
