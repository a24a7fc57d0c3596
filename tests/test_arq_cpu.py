"""ARQ on the batch ABI against the CPU test double of the backend
(tools/backend_hostsim.cpp): the acknowledgement and retransmission calls
against the reference, ack and retransmission rows, and the duplex scan, whose
twin of k_ackwalk is frames.h ack_walk.  The cases live in arq_cases.py;
test_arq_gpu.py runs the same ones on the MI355X."""
import os

import pytest

import arq_cases as K
import scenario_lib as S


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(S.REF_LIB):
        pytest.skip("oracle/_ref not built")
    return S.REF_LIB


@pytest.mark.parametrize("limit", [16, 32, 64])
def test_acks_and_retransmits_match_reference(ref, limit):
    K.check_parity(S.SIM_LIB, ref, limit)


def test_arq_argument_checks():
    K.check_arq_arguments(S.SIM_LIB)


def test_ack_rows():
    K.check_ack_rows(S.SIM_LIB)


def test_retransmit_rows():
    K.check_retransmit_rows(S.SIM_LIB)


def test_walk_smallest_rows():
    K.check_walk_small(S.SIM_LIB)


def test_walk_slots_and_truncation():
    K.check_walk_slots(S.SIM_LIB)


def test_walk_workgroup_edge_and_rows_without_acks():
    K.check_walk_counts(S.SIM_LIB)


def test_duplex_argument_checks():
    K.check_duplex_arguments(S.SIM_LIB, gpu=False)


def test_recv_duplex_routing_and_forged_records():
    K.check_recv_duplex(S.SIM_LIB)


def test_loop_end_to_end():
    K.check_loop(S.SIM_LIB)
