"""A sampled block's transpose and schedules built on the GPU (pg_csr_transpose_dev,
pg_schedule_count_dev, pg_schedule_build_dev) and the sampler's block path on them: the checks of
tests/devgraph_common.py with DEV = cuda. Every comparison is exact."""
import pytest

import devgraph_common as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("chunks", dc.CHUNK_PAIRS, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("name", list(dc.CASES))
def test_kernels_equal_host_functions(name, chunks):
    dc.check_kernels(DEV, name, *chunks)


@pytest.mark.parametrize("which", list(dc.BAD_INPUTS))
def test_bad_input_sets_status(which):
    dc.check_bad_input(DEV, which)


def test_capture_and_replay():
    dc.check_capture(DEV)


def test_arg_kind_from_max_deg():
    dc.check_arg_kind(DEV)


@pytest.mark.parametrize("name", ["rect_37x11", "rect_11x37", "nothing", "no_src", "empty_tail", "hub_column",
                                  "digits_65537"])
def test_device_graph_from_in_csr(name):
    dc.check_from_in_csr(DEV, name)
    dc.check_from_in_csr(DEV, name, 4, 2)


def test_has_zero_in_degree_from_min_deg():
    dc.check_zero_in_degree_device(DEV)


@pytest.mark.parametrize("which", ["parent", "hubs"])
def test_host_path_equals_device_path(which):
    dc.check_paths_equal(DEV, which)


def test_no_host_graph_after_forward_backward():
    dc.check_no_host_graph(DEV)


def test_empty_seeds():
    dc.check_empty_seeds(DEV)
