"""The executor's row-batch modes at window-shape edges on the MI355X: the
cases of test_exec_shapes_cpu.py (exec_shape_cases.py) through the device
library, where k_exec's OP_ROWS path does the arithmetic, with the
reference's recovery packets (tests/golden/exec_shapes.json)."""
import pytest

import exec_shape_cases as X
import scenario_lib as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import siamese_amd
    siamese_amd.require_gpu()
    return S.AMD_LIB


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
@pytest.mark.parametrize("name", list(X.CASES))
def test_exec_shapes(amd, name, device):
    X.check(name, amd, device)


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
def test_stage_edge(amd, device):
    """Windows of cap - 1, cap and cap + 1 elements, cap the stage capacity
    the library reports: the last window that is staged whole, and the first
    whose rows read an element from memory (kPlanGeneral, phase B1b)."""
    cap = X.stage_cap(amd)
    print("stage capacity: %d window elements" % cap)
    assert cap > 0, "the executor has no LDS stage on this device"
    if cap + 1 >= 512:
        # kLdpcSplitMin: a window past the stage would send its picks to
        # k_ldpc, so no executor row ever draws past the stage; window_511 of
        # the sweep is then the largest staged one
        assert cap >= 511
        enc, _ = X.check("window_511", amd, device)
        assert enc["unstaged"] == 0
        return
    for w in (cap - 1, cap, cap + 1):
        name = "window_%d" % w
        assert name in X.CASES, "no case for a window of %d beside a stage of %d: add it to " \
            "exec_shape_cases.STAGE_WINDOWS and run tests/golden/make_exec_shape_golden.py" % (w, cap)
        enc, _ = X.check(name, amd, device)
        assert enc["unstaged"] == (1 if w > cap else 0), "a window of %d, a stage of %d: %r" % (w, cap, enc)
