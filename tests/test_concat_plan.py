"""frames.h concat_plan and concat_copy alone (tests/concat_plan_test.cpp): the
plain C++ statement of one k_offsets job and of k_concat's copy, built as a
stand-alone host program with -fsanitize=address,undefined and run on the CPU.
Every symbol, offsets array, record array, info record and stream of the
program ends where its heap block ends, so the sanitizer checks the bytes
concat_plan and concat_copy may read and write; the program checks the sums,
the stop reasons (1 and 2 among them, and a 64-bit running sum past 2^32) and
the stream themselves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_concat_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "concat_plan_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + san + ["-static-libasan", "-static-libubsan",
                   "-I", os.path.join(ROOT, "siamese_amd", "csrc"),
                   os.path.join(ROOT, "tests", "concat_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert "concat_plan ok" in out.stdout
