"""sgpu_frames_scan_rows and sgpu_frames_recv_rows on the MI355X: the cases of
test_scan_cpu.py (scan_cases.py) through the device library, where k_scan
reads the rows."""
import pytest

import scan_cases as K
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_header_edges(amd):
    K.check_header_edges(amd)


def test_tail_alignment_and_a_full_last_row(amd):
    K.check_tail_alignment(amd)


def test_empty_and_stale_rows(amd):
    K.check_empty_and_stale(amd)


def test_malformed_rows_among_good_neighbours(amd):
    K.check_malformed(amd)


def test_parity_with_frames_recv(amd):
    K.check_parity(amd)


def test_many_flows_in_one_scan(amd):
    K.check_many_flows(amd, gpu=True)


def test_argument_checks(amd):
    K.check_arguments(amd)
