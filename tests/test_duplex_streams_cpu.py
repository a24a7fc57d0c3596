"""sgpu_frames_scan_duplex_streams and sgpu_frames_recv_duplex_streams against
the CPU test double of the backend (tools/backend_hostsim.cpp): the control
plane, the gather slots and tickets the scan shares with the other gathers, and
the walk's statement (frames.h ack_stream_walk) that k_ackstreamwalk is held to.
The cases live in duplex_streams_cases.py; test_duplex_streams_gpu.py runs the
same ones on the MI355X.  Forged output is also given to a stand-alone host
program built with -fsanitize=address,undefined
(tests/duplex_streams_forged_test.cpp)."""
import os
import shutil
import subprocess

import pytest

import duplex_streams_cases as K
import scenario_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_starts_and_ends():
    K.check_starts_and_ends(S.SIM_LIB)


def test_partial_and_never_valid_cuts():
    K.check_partial_frames(S.SIM_LIB)


def test_acks_slots_and_flags():
    K.check_acks(S.SIM_LIB)


def test_row_end_edges_and_max_frames():
    K.check_row_end(S.SIM_LIB)


@pytest.mark.parametrize("count", K.ROW_COUNTS)
def test_row_counts(count):
    K.check_row_counts(S.SIM_LIB, count)


def test_equals_the_dense_duplex_scan_from_start_zero():
    K.check_dense_equivalence(S.SIM_LIB)


def test_rows_are_all_or_nothing_at_the_cut():
    K.check_cut(S.SIM_LIB)


def test_resume_from_the_consumed_words():
    K.check_resume(S.SIM_LIB)


def test_argument_checks():
    K.check_arguments(S.SIM_LIB, gpu=False)


def test_forged_output_is_refused():
    K.check_forged(S.SIM_LIB)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_forged_output_under_sanitizers(tmp_path):
    """The library's host sources, the test double and the driver in one
    stand-alone program with the sanitizers' runtimes linked in: no report, and
    every forgery refused as the driver expects."""
    csrc = os.path.join(ROOT, "siamese_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    flags = ["-std=c++17", "-O1", "-g", "-mavx2", "-fvisibility=hidden"] + san
    host = ["gf.cpp", "codedef.cpp", "pool.cpp", "placement.cpp", "engine.cpp", "encoder.cpp", "decoder.cpp",
            "arq.cpp", "api.cpp", "batch.cpp", "frames.cpp"]
    jobs, objs = [], []
    for src in [os.path.join(csrc, f) for f in host] + [os.path.join(ROOT, "tools", "backend_hostsim.cpp"),
                                                         os.path.join(ROOT, "tests", "duplex_streams_forged_test.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        jobs.append(subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]))
    for j in jobs:
        assert j.wait(timeout=600) == 0
    exe = str(tmp_path / "duplex_streams_forged_test")
    subprocess.run(["g++"] + san + ["-static-libasan", "-static-libubsan", "-o", exe] + objs + ["-ldl", "-lpthread"],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert "duplex streams forged ok" in out.stdout
