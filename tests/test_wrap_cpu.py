"""Every path at the 22-bit packet-number wrap against the CPU test double of
the backend (tests/hostsim): the host control plane's column arithmetic and
the plain C++ twins of the kernels, with the reference's packets, decodes and
acknowledgements (tests/golden/wrap_edges.json).  The cases live in
wrap_cases.py; test_wrap_gpu.py runs the same ones on the MI355X.  The walk
to the wrap is made once, by the first test that needs it, for all of them."""
import os
import subprocess
import sys

import pytest

import scenario_lib as S
import wrap_cases as W


def test_fixture_is_the_reference(tmp_path):
    """Where the reference is built: its live walk and cases give
    wrap_edges.json byte for byte (tests/golden/make_wrap_golden.py)."""
    if not os.path.exists(S.REF_LIB):
        pytest.skip("oracle/_ref is not built: the fixture's regeneration from the reference was not checked")
    out = str(tmp_path / "wrap_edges.json")
    run = subprocess.run([sys.executable, os.path.join(S.ROOT, "tests", "golden", "make_wrap_golden.py"), "--out", out],
                         capture_output=True, text=True, timeout=300, cwd=S.ROOT)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    with open(out, "rb") as f, open(W.GOLDEN, "rb") as g:
        assert f.read() == g.read(), "wrap_edges.json is stale: run tests/golden/make_wrap_golden.py"


@pytest.fixture(scope="module", autouse=True)
def walk():
    """The pairs no test took and the walk's source are freed with the module."""
    yield
    W.release(S.SIM_LIB)


@pytest.mark.parametrize("name", list(W.CASES))
def test_wrap(name):
    W.check(name, S.SIM_LIB)


def test_ranges_across_the_wrap():
    W.check_ranges(S.SIM_LIB)


def test_arq_across_the_wrap():
    W.check_arq(S.SIM_LIB)


def test_split_two_sweeps():
    """The split solves with SGPU_TR_SOLVE=0 (read once per process, so in a
    child that walks its own two pairs).  The test double has one solve and
    ignores the knob: this pins that the cases pass in a fresh process, as
    test_wrap_gpu.py runs them."""
    W.check_in_child(["split16", "siamese450"], S.SIM_LIB, {"SGPU_TR_SOLVE": "0"})


def test_dropin_api():
    """The drop-in siamese.h calls of the library (the test double's build of
    them) walked to the wrap call by call, 4.19 M adds each way, then the
    remove_before case: the reference's walk hash, packets and decodes."""
    W.check_dropin_in_child(S.SIM_LIB, "trim")
