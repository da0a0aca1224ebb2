"""Link-prediction mini-batches on the GPU (pg_edge_bits_update, pg_sample_count_excl /
pg_sample_fill_excl, pg_edge_lookup, pg_negative_sample and the dgl shim on them): the checks of
tests/linkpred_common.py with DEV = cuda. Every kernel must equal its CPU twin bit for bit; the
sampler with exclusion must also equal the existing pg_sample_*_cpu on the filtered graph."""
import pytest

import linkpred_common as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("fanout", lc.FANOUTS)
def test_exclusion_equals_deletion(fanout):
    lc.check_exclusion(DEV, fanout)


def test_exclusion_empty_inputs():
    lc.check_exclusion_empty(DEV)


def test_edge_bits():
    lc.check_bits(DEV)


def test_edge_lookup_equals_dictionary_and_twin():
    lc.check_lookup(DEV)


def test_negative_sample_equals_cpu_twin():
    lc.check_negatives(DEV)


def test_shim_edge_queries():
    lc.check_shim_queries(DEV)


def test_shim_sampling():
    lc.check_shim_sampling(DEV)


def test_negative_samplers():
    lc.check_negative_samplers(DEV)


def test_edge_loader():
    lc.check_edge_loader(DEV)


def test_edge_loader_equals_cpu_device():
    lc.check_edge_loader_equals_cpu(DEV)


def test_link_prediction_end_to_end_equals_cpu_device():
    lc.check_end_to_end(DEV)
