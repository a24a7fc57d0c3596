"""sgpu_decoder_deliver_frames against the CPU test double of the backend
(tools/backend_hostsim.cpp): the control plane, the queued item and its place
in a submission, and the byte contract k_relay shares with frames.h relay_row,
which be_launch_relay's plain C++ twin runs.  The cases live in relay_cases.py;
test_relay_gpu.py runs the same ones on the MI355X."""
import pytest

import relay_cases as R
import scenario_lib as S


def test_edge_lengths_received():
    R.check_edge_lengths(S.SIM_LIB)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(device):
    R.check_recovered(S.SIM_LIB, device)


def test_byte_identity_with_the_sender():
    R.check_byte_identity(S.SIM_LIB)


def test_second_hop_scans_and_parses_the_rows():
    R.check_second_hop(S.SIM_LIB)


def test_absent_packets_and_redelivery():
    R.check_absent(S.SIM_LIB)


def test_frame_does_not_fit_where_the_payload_does():
    R.check_does_not_fit(S.SIM_LIB)


def test_argument_checks():
    R.check_arguments(S.SIM_LIB)


def test_many_instances_one_launch_and_relay_only():
    R.check_many_instances(S.SIM_LIB, gpu=False)
