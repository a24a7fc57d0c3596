"""sgpu_decoder_deliver_range on the MI355X: the cases of test_deliver_cpu.py
(deliver_cases.py) through the device library, where k_deliver places the
rows."""
import pytest

import deliver_cases as D
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_edge_lengths(amd):
    D.check_edge_lengths(amd)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_same_submission(amd, device):
    D.check_recovered(amd, device)


def test_absent_packets(amd):
    D.check_absent(amd)


def test_too_long_for_the_row(amd):
    D.check_too_long(amd)


def test_argument_checks(amd):
    D.check_arguments(amd)


def test_many_instances_one_launch(amd):
    D.check_many_instances(amd)


def test_delivery_only_submission(amd):
    D.check_delivery_only(amd)
