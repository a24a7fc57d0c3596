"""sgpu_frames_scan_rows and sgpu_frames_recv_rows against the CPU test double
of the backend (tools/backend_hostsim.cpp): the control plane, the gather
slots and tickets the scan rides on, and the record contract k_scan shares
with be_scan_rows' plain C++ twin (frames.cpp row_head_scan).  The cases live
in scan_cases.py; test_scan_gpu.py runs the same ones on the MI355X."""
import scan_cases as K
import scenario_lib as S


def test_header_edges():
    K.check_header_edges(S.SIM_LIB)


def test_tail_alignment_and_a_full_last_row():
    K.check_tail_alignment(S.SIM_LIB)


def test_empty_and_stale_rows():
    K.check_empty_and_stale(S.SIM_LIB)


def test_malformed_rows_among_good_neighbours():
    K.check_malformed(S.SIM_LIB)


def test_parity_with_frames_recv():
    K.check_parity(S.SIM_LIB)


def test_many_flows_in_one_scan():
    K.check_many_flows(S.SIM_LIB, gpu=False)


def test_argument_checks():
    K.check_arguments(S.SIM_LIB)


def test_forged_records_are_refused():
    K.check_forged(S.SIM_LIB)
