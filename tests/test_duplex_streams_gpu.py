"""sgpu_frames_scan_duplex_streams and sgpu_frames_recv_duplex_streams on the
MI355X: the cases of test_duplex_streams_cpu.py (duplex_streams_cases.py) through
the device library, where k_ackstreamwalk walks the rows a lane each and
k_rowsum2, k_compact and k_slots place records and slots.  Every expectation is
built from sgpu_frames_scan_duplex_dense's output on a zeroed copy of the rows
and from the frame lists the cases laid out."""
import pytest

import duplex_streams_cases as K
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_starts_and_ends(amd):
    K.check_starts_and_ends(amd)


def test_partial_and_never_valid_cuts(amd):
    K.check_partial_frames(amd)


def test_acks_slots_and_flags(amd):
    K.check_acks(amd)


def test_row_end_edges_and_max_frames(amd):
    K.check_row_end(amd)


@pytest.mark.parametrize("count", K.ROW_COUNTS)
def test_row_counts(amd, count):
    K.check_row_counts(amd, count)


def test_equals_the_dense_duplex_scan_from_start_zero(amd):
    K.check_dense_equivalence(amd)


def test_rows_are_all_or_nothing_at_the_cut(amd):
    K.check_cut(amd)


def test_resume_from_the_consumed_words(amd):
    K.check_resume(amd)


def test_argument_checks(amd):
    K.check_arguments(amd, gpu=True)
