"""The solves on inconsistent recovery data against the CPU test double of the
backend (tests/hostsim): one received original reaches the decoder with a
flipped byte or short, and the decode must hand back the reference's wrong
bytes and the reference's result codes (tests/golden/solve_inconsistent.json).
The double has the sweeps only, so no solve is ever flagged here; the cases
live in solve_cases.py, and test_solve_inconsistent_gpu.py runs the same ones
on the MI355X, where the product solve has to notice and step back."""
import pytest

import scenario_lib as S
import solve_cases as V


@pytest.mark.parametrize("name", list(V.CASES))
def test_solve_inconsistent(name):
    V.check(name, S.SIM_LIB)
