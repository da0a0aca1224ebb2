"""pg_spmm_sum_cpu on the CPU device: the whole matrix of test_gpu_spmm_sum.py, within the
float64 bar and bitwise against the row-by-row float32 order (sum_piecewise32 with
split=False); tests/sum_common.py holds the references, the ladder graph and the checks."""
import pytest

import sum_common as su

DEV = "cpu"


def test_width_list_straddles_the_tile_boundaries():
    su.check_width_list()


@pytest.mark.parametrize("F,form", su.WIDTH_CASES)
def test_width_sweep(F, form):
    su.check_width(DEV, F, form)


@pytest.mark.parametrize("chunk_bwd", [4, None], ids=["chunk4", "default_chunk"])
@pytest.mark.parametrize("weighted", [False, True], ids=["copy_u", "u_mul_e"])
@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("F", su.TRANSPOSED_WIDTHS)
def test_transposed_forms(F, mean, weighted, chunk_bwd):
    su.check_transposed(DEV, F, mean, weighted, chunk_bwd)


@pytest.mark.parametrize("chunk", [4, 64])
@pytest.mark.parametrize("F", [3, 40, 260])
def test_tiny_and_exact_items(F, chunk):
    su.check_item_lengths(DEV, chunk, F)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("F", [40, 260, 1100])
def test_unaligned_operands_give_the_same_bits(F, transpose):
    su.check_unaligned(DEV, F, transpose)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("off", [4, 1])
@pytest.mark.parametrize("F", [5, 64, 260])
def test_strided_views_with_guards(F, off, transpose):
    su.check_strided_guards(DEV, F, off, transpose)


@pytest.mark.parametrize("F", [3, 260])
def test_rectangular_graph(F):
    su.check_rect(DEV, F)


def test_empty_shapes():
    su.check_empty_shapes(DEV)


@pytest.mark.parametrize("transpose", [False, True], ids=["in_csr", "out_csr"])
@pytest.mark.parametrize("F", [64, 65])
def test_nonfinite_inputs(F, transpose):
    su.check_nonfinite(DEV, F, transpose)


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("F", [260, 503])
def test_autograd_at_width(F, mean):
    su.check_autograd(DEV, F, mean)


def test_error_returns():
    su.check_error_returns(DEV)
