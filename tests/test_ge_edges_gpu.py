"""The device decode's recovery matrix at its shape, pivot and singular edges
on the MI355X: the cases of test_ge_edges_cpu.py (ge_cases.py) through the
device library, where k_ge generates and eliminates the matrix, with the
reference's packets and decode results (tests/golden/ge_edges.json)."""
import pytest

import ge_cases as G
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("name", list(G.CASES))
def test_ge_edges(amd, name):
    G.check(name, amd)
