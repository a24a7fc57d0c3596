"""sgpu_decoder_deliver_stream on the MI355X: the cases of test_stream_cpu.py
(stream_cases.py) through the device library, where k_offsets sums the lengths
and k_concat copies to byte-granular destinations."""
import pytest

import scenario_lib as S
import stream_cases as ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_every_shift_short_packets(amd):
    ST.check_every_shift(amd, ST.SHIFT_SHORT, range(16))


def test_every_shift_two_byte_prefix(amd):
    ST.check_every_shift(amd, ST.SHIFT_HS2, range(16))


def test_shifts_three_byte_prefix(amd):
    ST.check_every_shift(amd, ST.SHIFT_HS3, (0, 1, 7, 15))


def test_chunk_and_tile_edges_at_odd_destinations(amd):
    ST.check_chunk_edges(amd)


def test_scan_wave_edges_and_stops(amd):
    ST.check_scan_wave_edges(amd)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(amd, device):
    ST.check_recovered(amd, device)


def test_holes_and_appending_at_the_cursor(amd):
    ST.check_holes(amd)


def test_invalid_pending_packet_stops_the_stream(amd):
    ST.check_invalid_pending(amd)


def test_jobs_of_one_submission_and_stream_only(amd):
    ST.check_jobs_one_submission(amd, gpu=True)


def test_argument_checks(amd):
    ST.check_arguments(amd)
