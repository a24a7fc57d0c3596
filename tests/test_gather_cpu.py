"""sgpu_gather, sgpu_gather_completed, sgpu_gather_async and sgpu_frames_send
against the CPU test double of the backend (tools/backend_hostsim.cpp): the
descriptors Engine::gather and Engine::gather_async_framed build, the landing
layout, the slot ring and the host-side unpack, and the byte contract k_ingest's
table-less path shares with ingest_one.  The cases live in gather_cases.py;
test_gather_gpu.py runs the same ones on the MI355X."""
import pytest

import gather_cases as G
import scenario_lib as S


def test_calls_that_move_nothing():
    G.check_nothing_to_move(S.SIM_LIB)


@pytest.mark.parametrize("way", ["gather", "completed", "async"])
def test_alignments_and_edge_lengths(way):
    G.check_alignment_lengths(S.SIM_LIB, way)


def test_grid_counts():
    G.check_grid_counts(S.SIM_LIB)


@pytest.mark.parametrize("count,way", [(2048, "gather"), (2049, "gather"), (4097, "gather"), (4097, "completed")])
def test_many_short_ranges(count, way):
    G.check_many_ranges(S.SIM_LIB, count, way)


def test_nine_gathers_in_flight():
    G.check_slot_ring(S.SIM_LIB)


def test_staging_growth():
    G.check_staging_growth(S.SIM_LIB)


def test_framed_alignments_and_header_lengths():
    G.check_framed(S.SIM_LIB)


def test_gather_ordered_before_the_next_submission():
    G.check_ordering(S.SIM_LIB)
