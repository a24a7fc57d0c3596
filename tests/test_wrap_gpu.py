"""Every path at the 22-bit packet-number wrap on the MI355X: the cases of
test_wrap_cpu.py (wrap_cases.py) through the device library, where k_ingest,
k_exec, k_ldpc, k_ge, the solve kernels and the delivery kernels get window
entries, columns and packet numbers that wrap, with the reference's packets,
decodes and acknowledgements (tests/golden/wrap_edges.json).  The walk to the
wrap is made once, by the first test that needs it, for all of them."""
import faulthandler

import pytest

import scenario_lib as S
import wrap_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    yield S.AMD_LIB
    W.release(S.AMD_LIB)     # (the pairs no test took, and the walk's source)


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this module, the walk included, ends its process with a
    traceback if it has not returned after two minutes (a hung device call
    never returns to Python).  That ends the whole pytest process, the GPU
    modules after this one included: after a hang nothing more is to start on
    the device.  The children of this module have limits of 110 s, below
    this one, so none outlives its parent."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("name", list(W.CASES))
def test_wrap(amd, name):
    W.check(name, amd)


def test_ranges_across_the_wrap(amd):
    W.check_ranges(amd)


def test_arq_across_the_wrap(amd):
    W.check_arq(amd)


def test_split_two_sweeps(amd):
    """SGPU_TR_SOLVE=0 (read once per process, so in a child that walks its
    own two pairs): the 16- and 20-row solves across the wrap as the
    reference's two sweeps (k_solve_prefix + k_solve_main) instead of the
    product X = T R (k_solve_pre + k_solve_tr)."""
    W.check_in_child(["split16", "siamese450"], amd, {"SGPU_TR_SOLVE": "0"})


def test_dropin_api(amd):
    """The drop-in siamese.h calls of the device library walked to the wrap
    call by call, then the remove_before case, in a process of its own under
    a time limit."""
    W.check_dropin_in_child(amd, "trim", seconds=110)
