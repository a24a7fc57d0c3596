"""Encode -> eliminate -> solve at tile-boundary packet sizes against the CPU
test double of the backend (tests/hostsim): the descriptors the host control
plane lays out for these sizes and the plain C++ twins of the kernels, with
the reference's recovery packets (tests/golden/size_edges.json).  The cases
live in size_cases.py; test_sizes_gpu.py runs the same ones on the MI355X."""
import pytest

import scenario_lib as S
import size_cases as Z


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
@pytest.mark.parametrize("name", list(Z.CASES))
def test_sizes(name, device):
    Z.check(name, S.SIM_LIB, device)


def test_product20_two_sweeps():
    """product20 with SGPU_TR_SOLVE=0 (read once per process, so in a child).
    The test double has one solve and ignores the knob: this pins that the
    case itself passes in a fresh process, as test_sizes_gpu.py runs it."""
    Z.check_in_child("product20", S.SIM_LIB, False, {"SGPU_TR_SOLVE": "0"})
