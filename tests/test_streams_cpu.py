"""sgpu_frames_scan_streams and sgpu_frames_recv_streams against the CPU test
double of the backend (tools/backend_hostsim.cpp): the control plane, the gather
slots and tickets the stream scan shares with the other gathers, and the walk's
statement (frames.h stream_walk) that k_streamwalk is held to.  The cases live in
streams_cases.py; test_streams_gpu.py runs the same ones on the MI355X.  Forged
output is also given to a stand-alone host program built with
-fsanitize=address,undefined (tests/streams_forged_test.cpp)."""
import os
import shutil
import subprocess

import pytest

import scenario_lib as S
import streams_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_edges():
    K.check_chunk_edges(S.SIM_LIB)


def test_dense_small_frames_and_max_frames():
    K.check_small_frames(S.SIM_LIB)


def test_starts_and_ends():
    K.check_starts_and_ends(S.SIM_LIB)


@pytest.mark.parametrize("count", K.ROW_COUNTS)
def test_row_counts(count):
    K.check_row_counts(S.SIM_LIB, count)


def test_partial_and_malformed_frames():
    K.check_partial_frames(S.SIM_LIB)


def test_resume_from_the_next_words():
    K.check_resume(S.SIM_LIB)


def test_rows_are_all_or_nothing_at_the_cut():
    K.check_cut(S.SIM_LIB)


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
                                                         os.path.join(ROOT, "tests", "streams_forged_test.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        jobs.append(subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]))
    for j in jobs:
        assert j.wait(timeout=600) == 0
    exe = str(tmp_path / "streams_forged_test")
    subprocess.run(["g++"] + san + ["-static-libasan", "-static-libubsan", "-o", exe] + objs + ["-ldl", "-lpthread"],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert "streams forged ok" in out.stdout
