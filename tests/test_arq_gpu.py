"""ARQ on the batch ABI on the MI355X: the cases of test_arq_cpu.py
(arq_cases.py) through the device library, where k_ackwalk reads the rows of a
bidirectional flow and k_frame writes the ack and retransmission rows."""
import os

import pytest

import arq_cases as K
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("limit", [16, 32, 64])
def test_acks_and_retransmits_match_reference(amd, limit):
    if not os.path.exists(S.REF_LIB):
        pytest.skip("oracle/_ref not built")
    K.check_parity(amd, S.REF_LIB, limit)


def test_ack_rows(amd):
    K.check_ack_rows(amd)


def test_retransmit_rows(amd):
    K.check_retransmit_rows(amd)


def test_walk_smallest_rows(amd):
    K.check_walk_small(amd)


def test_walk_slots_and_truncation(amd):
    K.check_walk_slots(amd)


def test_walk_workgroup_edge_and_rows_without_acks(amd):
    K.check_walk_counts(amd)


def test_duplex_argument_checks(amd):
    K.check_duplex_arguments(amd, gpu=True)


def test_recv_duplex_routing(amd):
    K.check_recv_duplex(amd)


def test_loop_end_to_end(amd):
    K.check_loop(amd)
