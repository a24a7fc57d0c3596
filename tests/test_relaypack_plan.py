"""frames.h pack_plan alone (tests/relaypack_plan_test.cpp): the plain C++
statement of one k_plan job, and relay_row into the spans it gives (k_pack),
built as a stand-alone host program with -fsanitize=address,undefined and run
on the CPU.  Every symbol, record array, length array, info record and row of
the program ends where its heap block ends, so the sanitizer checks the bytes
pack_plan and relay_row may read and write; the program checks the layout and
the rows themselves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pack_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "relaypack_plan_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + san + ["-static-libasan", "-static-libubsan",
                   "-I", os.path.join(ROOT, "siamese_amd", "csrc"),
                   os.path.join(ROOT, "tests", "relaypack_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert "pack_plan ok" in out.stdout
