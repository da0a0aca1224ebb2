"""A sampled block's transpose and schedules on the device, the parts that need no GPU: the
exports, the numpy restatement of the host functions on every case of tests/devgraph_common.py,
DeviceGraph.from_in_csr on the CPU device and has_zero_in_degree()."""
import pytest

import devgraph_common as dc


def test_exports():
    dc.check_exports()


@pytest.mark.parametrize("chunks", dc.CHUNK_PAIRS, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("name", list(dc.CASES))
def test_numpy_restatement_equals_host_functions(name, chunks):
    dc.check_restatement(name, *chunks)


@pytest.mark.parametrize("name", ["rect_37x11", "rect_11x37", "nothing", "no_src", "empty_tail", "hub_column"])
def test_device_graph_from_in_csr_on_cpu(name):
    dc.check_from_in_csr("cpu", name)


def test_has_zero_in_degree():
    dc.check_zero_in_degree_host()
