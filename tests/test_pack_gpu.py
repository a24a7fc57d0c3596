"""sgpu_frames_scan_packed, sgpu_frames_recv_packed and sgpu_encoder_pack_frames
on the MI355X: the cases of test_pack_cpu.py (pack_cases.py) through the device
library, where k_walk reads the rows and k_frame writes the packed ones."""
import pytest

import pack_cases as K
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


def test_header_at_every_byte_offset(amd):
    K.check_header_offsets(amd)


def test_recovery_head_and_tail(amd):
    K.check_recovery_tails(amd)


def test_gaps_and_empty_rows(amd):
    K.check_gaps(amd)


def test_max_frames_edges(amd):
    K.check_max_frames(amd)


def test_malformed_frames_among_good_neighbours(amd):
    K.check_malformed(amd)


def test_parity_and_routing(amd):
    K.check_parity_routing(amd)


def test_packer_layout(amd):
    K.check_packer(amd)


def test_round_trip(amd):
    K.check_round_trip(amd, device=True)


def test_argument_checks(amd):
    K.check_arguments(amd, gpu=True)
