"""The solves on inconsistent recovery data on the MI355X: the cases of
test_solve_inconsistent_cpu.py (solve_cases.py) through the device library,
where k_solve_main's sweeps on both tile sizes, k_solve_prefix, k_solve_pre
and k_solve_tr (whose flagged product k_solve_main must redo by the sweeps)
and the solve gated behind a chained k_ge job do the arithmetic, with the
reference's wrong bytes and result codes
(tests/golden/solve_inconsistent.json)."""
import pytest

import scenario_lib as S
import solve_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("name", list(V.CASES))
def test_solve_inconsistent(amd, name):
    V.check(name, amd)


@pytest.mark.parametrize("name", V.SWEEPS_AGAIN)
def test_solve_inconsistent_two_sweeps(amd, name):
    """SGPU_TR_SOLVE=0 (read once per process, so in a child): the split
    launches as k_solve_prefix + k_solve_main, no product and so no flag."""
    V.check_in_child(name, amd, {"SGPU_TR_SOLVE": "0"})
