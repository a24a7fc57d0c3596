"""sgpu_encoder_deliver_range and sgpu_frames_deliver_recovery on the MI355X:
the cases of test_frame_cpu.py (frame_cases.py) through the device library,
where k_frame places the rows."""
import pytest

import frame_cases as F
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("framed", [True, False], ids=["framed", "bare"])
def test_original_edge_lengths(amd, framed):
    F.check_original_edges(amd, framed)


def test_recovery_same_submission_framed(amd):
    F.check_recovery_framed(amd)


def test_recovery_bare(amd):
    F.check_recovery_bare(amd)


def test_round_trip_through_the_wire_format(amd):
    F.check_round_trip(amd)


def test_absent_originals_and_redelivery(amd):
    F.check_absent(amd)


def test_argument_checks(amd):
    F.check_arguments(amd)


def test_many_instances_one_launch_and_framing_only(amd):
    F.check_many_instances(amd, gpu=True)
