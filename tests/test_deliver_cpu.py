"""sgpu_decoder_deliver_range against the CPU test double of the backend
(tests/hostsim): the control plane, the queued item and its place in a
submission, and the byte contract k_deliver shares with be_launch_deliver's
plain C++ twin.  The cases live in deliver_cases.py; test_deliver_gpu.py runs
the same ones on the MI355X."""
import pytest

import deliver_cases as D
import scenario_lib as S


def test_edge_lengths():
    D.check_edge_lengths(S.SIM_LIB)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_same_submission(device):
    D.check_recovered(S.SIM_LIB, device)


def test_absent_packets():
    D.check_absent(S.SIM_LIB)


def test_too_long_for_the_row():
    D.check_too_long(S.SIM_LIB)


def test_argument_checks():
    D.check_arguments(S.SIM_LIB)


def test_many_instances_one_launch():
    D.check_many_instances(S.SIM_LIB)


def test_delivery_only_submission():
    D.check_delivery_only(S.SIM_LIB)
