"""The device decode's recovery matrix at its shape, pivot and singular edges
against the CPU test double of the backend (tests/hostsim): be_launch_ge, the
plain C++ twin of k_ge, and the host's half of the outcome (finish_chained,
finish_device_ge, chain_sums_restore), with the reference's packets and decode
results (tests/golden/ge_edges.json).  The cases live in ge_cases.py;
test_ge_edges_gpu.py runs the same ones on the MI355X."""
import pytest

import ge_cases as G
import scenario_lib as S


@pytest.mark.parametrize("name", list(G.CASES))
def test_ge_edges(name):
    G.check(name, S.SIM_LIB)
