"""Encode -> eliminate -> solve at tile-boundary packet sizes on the MI355X:
the cases of test_sizes_cpu.py (size_cases.py) through the device library,
where k_ingest, k_exec, k_ldpc, k_ge and the solve kernels do the arithmetic,
with the reference's recovery packets (tests/golden/size_edges.json)."""
import pytest

import scenario_lib as S
import size_cases as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
@pytest.mark.parametrize("name", list(Z.CASES))
def test_sizes(amd, name, device):
    Z.check(name, amd, device)


def test_product20_two_sweeps(amd):
    """SGPU_TR_SOLVE=0 (read once per process, so in a child): the 20-row
    solve as the reference's two sweeps (k_solve_prefix + k_solve_main)
    instead of the product X = T R (k_solve_pre + k_solve_tr)."""
    Z.check_in_child("product20", amd, False, {"SGPU_TR_SOLVE": "0"})
