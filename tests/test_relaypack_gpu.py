"""sgpu_decoder_pack_frames on the MI355X: the cases of test_relaypack_cpu.py
(relaypack_cases.py) through the device library, where k_plan lays the frames
out and k_pack places them."""
import pytest

import relaypack_cases as RP
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_edge_lengths_packed(amd):
    RP.check_edge_lengths(amd)


def test_exact_fits_and_a_chunk_edge_inside_a_span(amd):
    RP.check_exact_fits(amd)


def test_plan_wave_edges(amd):
    RP.check_plan_wave_edges(amd)


def test_jobs_of_one_submission_and_pack_only(amd):
    RP.check_jobs_one_submission(amd, gpu=True)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_recovered_in_the_same_submission(amd, device):
    RP.check_recovered(amd, device)


def test_byte_identity_with_the_sender(amd):
    RP.check_byte_identity(amd)


def test_second_hop_scans_and_parses_the_rows(amd):
    RP.check_second_hop(amd)


def test_absent_packets_and_repacking(amd):
    RP.check_absent(amd)


def test_pending_packet_that_does_not_fit_is_skipped(amd):
    RP.check_does_not_fit(amd)


def test_too_few_rows(amd):
    RP.check_too_few_rows(amd)


def test_argument_checks(amd):
    RP.check_arguments(amd)
