"""sgpu_decoder_deliver_stream against the CPU test double of the backend
(tools/backend_hostsim.cpp): the control plane, the queued job and its place in
a submission, and the byte contract k_offsets and k_concat share with frames.h
concat_plan and concat_copy, which be_launch_concat's plain C++ twin runs.  The
cases live in stream_cases.py; test_stream_gpu.py runs the same ones on the
MI355X."""
import pytest

import scenario_lib as S
import stream_cases as ST


def test_every_shift_short_packets():
    ST.check_every_shift(S.SIM_LIB, ST.SHIFT_SHORT, range(16))


def test_every_shift_two_byte_prefix():
    ST.check_every_shift(S.SIM_LIB, ST.SHIFT_HS2, range(16))


def test_shifts_three_byte_prefix():
    ST.check_every_shift(S.SIM_LIB, ST.SHIFT_HS3, (0, 1, 7, 15))


def test_chunk_and_tile_edges_at_odd_destinations():
    ST.check_chunk_edges(S.SIM_LIB)


def test_scan_wave_edges_and_stops():
    ST.check_scan_wave_edges(S.SIM_LIB)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(device):
    ST.check_recovered(S.SIM_LIB, device)


def test_holes_and_appending_at_the_cursor():
    ST.check_holes(S.SIM_LIB)


def test_invalid_pending_packet_stops_the_stream():
    ST.check_invalid_pending(S.SIM_LIB)


def test_jobs_of_one_submission_and_stream_only():
    ST.check_jobs_one_submission(S.SIM_LIB, gpu=False)


def test_argument_checks():
    ST.check_arguments(S.SIM_LIB)
