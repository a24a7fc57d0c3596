"""sgpu_frames_scan_dense and sgpu_frames_recv_dense on the MI355X: the cases of
test_dense_cpu.py (dense_cases.py) through the device library, where k_walkd
reads the rows, k_rowsum sums their counts and k_compact places the records.
Every expectation is built from sgpu_frames_scan_packed's output (k_walk) on the
same rows."""
import pytest

import dense_cases as K
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("count", K.EDGE_COUNTS)
def test_row_count_edges(amd, count):
    K.check_row_counts(amd, count)


def test_degenerate_mixes(amd):
    K.check_degenerate(amd)


def test_rows_are_all_or_nothing_at_the_cut(amd):
    K.check_cut(amd)


def test_flags_survive(amd):
    K.check_flags(amd)


def test_record_content(amd):
    K.check_record_content(amd)


def test_routing_agrees_with_the_packed_scan(amd):
    K.check_routing(amd)


def test_argument_checks(amd):
    K.check_arguments(amd, gpu=True)
