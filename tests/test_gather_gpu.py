"""sgpu_gather, sgpu_gather_completed, sgpu_gather_async and sgpu_frames_send on
the MI355X: the cases of test_gather_cpu.py (gather_cases.py) through the
device library, where k_ingest's table-less path makes the copies."""
import pytest

import gather_cases as G
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_calls_that_move_nothing(amd):
    G.check_nothing_to_move(amd)


@pytest.mark.parametrize("way", ["gather", "completed", "async"])
def test_alignments_and_edge_lengths(amd, way):
    G.check_alignment_lengths(amd, way, gpu=True)   # (with the path check on sgpu_gather's run)


def test_grid_counts(amd):
    G.check_grid_counts(amd)


@pytest.mark.parametrize("count,way", [(2048, "gather"), (2049, "gather"), (4097, "gather"), (4097, "completed")])
def test_many_short_ranges(amd, count, way):
    G.check_many_ranges(amd, count, way)


def test_nine_gathers_in_flight(amd):
    G.check_slot_ring(amd)


def test_staging_growth(amd):
    G.check_staging_growth(amd)


def test_framed_alignments_and_header_lengths(amd):
    G.check_framed(amd)


def test_gather_ordered_before_the_next_submission(amd):
    G.check_ordering(amd)
