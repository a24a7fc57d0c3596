"""sgpu_encoder_deliver_range and sgpu_frames_deliver_recovery against the CPU
test double of the backend (tools/backend_hostsim.cpp): the control plane, the
queued item and its place in a submission, and the byte contract k_frame
shares with be_launch_frame's plain C++ twin.  The cases live in
frame_cases.py; test_frame_gpu.py runs the same ones on the MI355X."""
import pytest

import frame_cases as F
import scenario_lib as S


@pytest.mark.parametrize("framed", [True, False], ids=["framed", "bare"])
def test_original_edge_lengths(framed):
    F.check_original_edges(S.SIM_LIB, framed)


def test_recovery_same_submission_framed():
    F.check_recovery_framed(S.SIM_LIB)


def test_recovery_bare():
    F.check_recovery_bare(S.SIM_LIB)


def test_round_trip_through_the_wire_format():
    F.check_round_trip(S.SIM_LIB)


def test_absent_originals_and_redelivery():
    F.check_absent(S.SIM_LIB)


def test_argument_checks():
    F.check_arguments(S.SIM_LIB)


def test_many_instances_one_launch_and_framing_only():
    F.check_many_instances(S.SIM_LIB, gpu=False)
