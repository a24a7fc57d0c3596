"""sgpu_decoder_pack_frames against the CPU test double of the backend
(tools/backend_hostsim.cpp): the control plane, the queued job and its place in
a submission, and the byte contract k_plan and k_pack share with frames.h
pack_plan and relay_row, which be_launch_pack's plain C++ twin runs.  The cases
live in relaypack_cases.py; test_relaypack_gpu.py runs the same ones on the
MI355X."""
import pytest

import relaypack_cases as RP
import scenario_lib as S


def test_edge_lengths_packed():
    RP.check_edge_lengths(S.SIM_LIB)


def test_exact_fits_and_a_chunk_edge_inside_a_span():
    RP.check_exact_fits(S.SIM_LIB)


def test_plan_wave_edges():
    RP.check_plan_wave_edges(S.SIM_LIB)


def test_jobs_of_one_submission_and_pack_only():
    RP.check_jobs_one_submission(S.SIM_LIB, gpu=False)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(device):
    RP.check_recovered(S.SIM_LIB, device)


def test_byte_identity_with_the_sender():
    RP.check_byte_identity(S.SIM_LIB)


def test_second_hop_scans_and_parses_the_rows():
    RP.check_second_hop(S.SIM_LIB)


def test_absent_packets_and_repacking():
    RP.check_absent(S.SIM_LIB)


def test_pending_packet_that_does_not_fit_is_skipped():
    RP.check_does_not_fit(S.SIM_LIB)


def test_too_few_rows():
    RP.check_too_few_rows(S.SIM_LIB)


def test_argument_checks():
    RP.check_arguments(S.SIM_LIB)
