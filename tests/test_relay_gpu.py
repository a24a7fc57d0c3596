"""sgpu_decoder_deliver_frames on the MI355X: the cases of test_relay_cpu.py
(relay_cases.py) through the device library, where k_relay places the rows."""
import pytest

import relay_cases as R
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_edge_lengths_received(amd):
    R.check_edge_lengths(amd)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(amd, device):
    R.check_recovered(amd, device)


def test_byte_identity_with_the_sender(amd):
    R.check_byte_identity(amd)


def test_second_hop_scans_and_parses_the_rows(amd):
    R.check_second_hop(amd)


def test_absent_packets_and_redelivery(amd):
    R.check_absent(amd)


def test_frame_does_not_fit_where_the_payload_does(amd):
    R.check_does_not_fit(amd)


def test_argument_checks(amd):
    R.check_arguments(amd)


def test_many_instances_one_launch_and_relay_only(amd):
    R.check_many_instances(amd, gpu=True)
