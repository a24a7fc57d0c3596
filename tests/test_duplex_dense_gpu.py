"""sgpu_frames_scan_duplex_dense and sgpu_frames_recv_duplex_dense on the MI355X:
the cases of test_duplex_dense_cpu.py (duplex_dense_cases.py) through the device
library, where k_ackwalkd reads the rows, k_rowsum2 sums both counts, k_compact
places the records and k_slots the slots.  Every expectation is built from
sgpu_frames_scan_duplex's output (k_ackwalk) on the same rows."""
import pytest

import duplex_dense_cases as K
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


def test_ack_free_rows_give_the_dense_scan(amd):
    K.check_ack_free(amd)


def test_rows_are_all_or_nothing_under_both_budgets(amd):
    K.check_cut(amd)


def test_the_cut_behind_the_first_wave_and_pass(amd):
    K.check_cut_far(amd)


def test_flags_and_truncation_survive(amd):
    K.check_flags(amd)


def test_slot_content(amd):
    K.check_slot_content(amd)


def test_routing_agrees_with_the_duplex_scan(amd):
    K.check_routing(amd)


def test_one_round_of_the_loop(amd):
    K.check_loop(amd)


def test_argument_checks(amd):
    K.check_arguments(amd, gpu=True)
