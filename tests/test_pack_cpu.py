"""sgpu_frames_scan_packed, sgpu_frames_recv_packed and sgpu_encoder_pack_frames
against the CPU test double of the backend (tools/backend_hostsim.cpp): the
control plane, the gather slots and tickets the packed scan shares with the
other gathers, and the record contract k_walk shares with be_walk_rows' plain
C++ twin (frames.h row_walk).  The cases live in pack_cases.py;
test_pack_gpu.py runs the same ones on the MI355X."""
import pytest

import pack_cases as K
import scenario_lib as S


def test_header_at_every_byte_offset():
    K.check_header_offsets(S.SIM_LIB)


def test_recovery_head_and_tail():
    K.check_recovery_tails(S.SIM_LIB)


def test_gaps_and_empty_rows():
    K.check_gaps(S.SIM_LIB)


def test_max_frames_edges():
    K.check_max_frames(S.SIM_LIB)


def test_malformed_frames_among_good_neighbours():
    K.check_malformed(S.SIM_LIB)


def test_parity_and_routing():
    K.check_parity_routing(S.SIM_LIB)


def test_packer_layout():
    K.check_packer(S.SIM_LIB)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_round_trip(device):
    K.check_round_trip(S.SIM_LIB, device)


def test_argument_checks():
    K.check_arguments(S.SIM_LIB, gpu=False)


def test_forged_records_are_refused():
    K.check_forged(S.SIM_LIB)
