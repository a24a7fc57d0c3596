"""Chained device decodes of wide windows on the MI355X: the checks of
test_chained_wide_cpu.py through the device library (k_ge, gated k_ldpc,
gated k_exec ranges and solves in one submission per decode)."""
import pytest

import scenario_lib as S
from test_chained_wide_cpu import (BLOCK, check_accounting, check_chained, check_reference,
                                   check_retried)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_matches_reference(amd, name):
    check_reference(amd, name)


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_is_chained(amd, name):
    check_chained(amd, name)


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_accounting(amd, name):
    check_accounting(amd, name)


def test_chained_wide_singular_retry(amd):
    """A wide chained job whose matrix is singular (the gated k_ldpc items,
    row batches and solve are skipped on the device, the host repeats the
    elimination): still the reference's results."""
    check_retried(amd, "wide_retry")
    check_reference(amd, "wide_retry")
