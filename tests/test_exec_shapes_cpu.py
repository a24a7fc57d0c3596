"""The executor's row-batch modes at window-shape edges against the CPU test
double of the backend (tests/hostsim): the batches the host control plane
makes of each schedule (Program::rows_update, Program::rows_row, counted by
sgpu_engine_stats_ex [30..34]) and the plain C++ twin of k_exec's OP_ROWS
path, with the reference's recovery packets (tests/golden/exec_shapes.json).
The cases live in exec_shape_cases.py; test_exec_shapes_gpu.py runs the same
ones on the MI355X."""
import pytest

import exec_shape_cases as X
import scenario_lib as S


@pytest.mark.parametrize("device", [False, True], ids=["decode", "decode_device"])
@pytest.mark.parametrize("name", list(X.CASES))
def test_exec_shapes(name, device):
    X.check(name, S.SIM_LIB, device)


def test_no_stage():
    """The test double reads every element from memory: it reports no stage,
    and then no batch counts as exceeding one (exec_shape_cases.check asserts
    the latter for every case)."""
    assert X.stage_cap(S.SIM_LIB) == 0


def test_both_sides_of_every_edge():
    """The cases' expected counters name both sides of each edge the host
    decides: versioned or not, a split after kVersionRows rows, a block that
    fits the LDS table or not."""
    enc = {name: case.enc for name, case in X.CASES.items()}
    assert enc["join15"]["versioned_rows"] == 15 and enc["join16"]["versioned_rows"] == 16
    assert enc["join17"]["versioned_rows"] == 16 and enc["join17"]["batches"] == 2
    assert enc["span32"]["versioned"] == 1 and enc["span33"]["versioned"] == 0
    assert enc["fit_edge"]["unfit"] == 0 and enc["fit_edge1"]["unfit"] == 1
    assert enc["rows300"]["unfit"] == 1
    for w in X.SWEEP + X.STAGE_WINDOWS:
        assert "window_%d" % w in X.CASES
