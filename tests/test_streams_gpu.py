"""sgpu_frames_scan_streams and sgpu_frames_recv_streams on the MI355X: the cases
of test_streams_cpu.py (streams_cases.py) through the device library, where
k_streamwalk walks the rows a wave each and k_rowsum and k_compact place the
records.  Every expectation is built from sgpu_frames_scan_dense's output on a
zeroed copy of the rows and from the frame lists the cases laid out."""
import pytest

import scenario_lib as S
import streams_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_chunk_edges(amd):
    K.check_chunk_edges(amd)


def test_dense_small_frames_and_max_frames(amd):
    K.check_small_frames(amd)


def test_starts_and_ends(amd):
    K.check_starts_and_ends(amd)


@pytest.mark.parametrize("count", K.ROW_COUNTS)
def test_row_counts(amd, count):
    K.check_row_counts(amd, count)


def test_partial_and_malformed_frames(amd):
    K.check_partial_frames(amd)


def test_resume_from_the_next_words(amd):
    K.check_resume(amd)


def test_rows_are_all_or_nothing_at_the_cut(amd):
    K.check_cut(amd)


def test_argument_checks(amd):
    K.check_arguments(amd, gpu=True)
