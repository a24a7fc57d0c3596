"""The decoder's recovery list and readiness walk (DecoderCore::list_insert,
check_recovery_possible) against the reference, on the CPU test double.

A block's recovery packets all have one key, so list_insert starts its search
in front of the tail's run of that key, and check_recovery_possible derives
the walk after an insert in front of the head from the walk before it.  The
test double's decoder is built with SGPU_WALK_CHECK (siamese_amd/Makefile):
every shortcut taken is compared with the search from the tail / the walk from
the head and the process aborts on a difference, in this file and in every
other hostsim test.  Here the call sequences that bear on the shortcuts run
against fixtures recorded from the reference (tests/golden/make_walk_golden.py):
event logs with every is_ready and decode result code.
"""
import os
import shutil
import subprocess

import pytest

import golden
import scenario_lib as S
import walk_cases as W

ROOT = W.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return W.build_driver(tmp_path_factory.mktemp("walks") / "recovery_walks_test")


def _counts(stderr):
    line = [l for l in stderr.splitlines() if l.startswith("walk counts:")][-1].split()
    return {line[i]: int(line[i + 1]) for i in range(2, len(line), 2)}


@needs_gxx
@pytest.mark.parametrize("name", W.SEQUENCES)
def test_sequence_matches_reference(driver, name):
    """block: one key, 30 % loss on both sides; interleave: originals between
    recovery packets of one key; reorder: ends below and above the tail's
    run, equal ends with another start, duplicates; delete_run: the next
    expected packet passes the run, then more packets of its key."""
    env = dict(os.environ, SIAMESE_AMD_WALK_COUNTS="1")
    out = W.run_driver(driver, S.SIM_LIB, name, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    with open(W.sequence_path(name)) as f:
        want = f.read()
    got = out.stdout
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail("%s: event %d differs: got %r, reference %r" % (name, k, a[k:k + 1], b[k:k + 1]))
    c = _counts(out.stderr)
    if name == "reorder":
        assert c["insert_hops"] > c["inserts"]        # the search from the tail ran
    else:
        # one key: no node of the run visited, and all walks but a few derived
        assert c["insert_hops"] == 0 and c["shortcuts"] >= c["inserts"] // 2


@pytest.mark.parametrize("name", sorted(W.CONFIGS))
@pytest.mark.parametrize("path", ["dropin", "batch", "device_ge"])
def test_config_matches_reference(name, path):
    """A block of 64 x 100 B at 30 % loss, and streaming with immediate
    acknowledgements and a recovery packet every 4 originals, through the
    drop-in API, sgpu_decode and sgpu_decode_device."""
    cfg = W.CONFIGS[name]
    if path == "dropin":
        res, _, _ = S.run_capi(S.SIM_LIB, cfg)
    else:
        res, rep = S.run_batch(S.SIM_LIB, cfg, verify=True, device_ge=path == "device_ge", threads=2)
        assert rep.mismatches == 0 and rep.checked > 0
    want = golden.load(name)
    assert S.digests(res) == want["digests"]
    assert [int(r.status) for r in res] == want["status"]


def test_singular_chained_decode_then_more_packets():
    """wide_retry: a chained device decode comes out singular, the host
    repeats it and later recovery packets extend the search; edge_lag: long
    streams whose decodes fail and go on.  Digests of the committed fixtures."""
    import test_chained_wide_cpu as T
    cfg = T.CONFIGS["wide_retry"]
    res, rep = S.run_batch(S.SIM_LIB, cfg, verify=True, device_ge=True, **T.RUN["wide_retry"])
    assert S.engine_dict(rep)["ge_retried"] >= 1
    assert S.digests(res) == golden.load("wide_retry")["digests"] and rep.mismatches == 0
    cfg = golden.config("edge_lag")
    res, rep = S.run_batch(S.SIM_LIB, cfg, verify=True, device_ge=True)
    assert S.digests(res) == golden.load("edge_lag")["digests"] and rep.mismatches == 0


@needs_gxx
def test_sequences_under_sanitizers(tmp_path):
    """The same sequences with the library's host sources and the driver
    built with -fsanitize=address,undefined (and SGPU_WALK_CHECK) into one
    stand-alone program: no report, and the reference's event logs."""
    csrc = os.path.join(ROOT, "siamese_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    flags = ["-std=c++17", "-O1", "-g", "-mavx2", "-fvisibility=hidden",
             "-DSGPU_WALK_CHECK"] + san
    host = ["gf.cpp", "codedef.cpp", "pool.cpp", "placement.cpp", "engine.cpp", "encoder.cpp", "decoder.cpp",
            "arq.cpp", "api.cpp", "batch.cpp", "frames.cpp"]
    jobs = []
    objs = []
    for src in [os.path.join(csrc, f) for f in host] + [os.path.join(ROOT, "tools", "backend_hostsim.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        jobs.append(subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]))
    for j in jobs:
        assert j.wait(timeout=600) == 0
    # one program with the sanitizers' runtimes linked in: it needs nothing
    # from the environment it is started in
    exe = str(tmp_path / "recovery_walks_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + san + ["-static-libasan", "-static-libubsan", "-rdynamic",
                                                               W.DRIVER_SRC, "-o", exe] + objs +
                   ["-ldl", "-lpthread"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in W.SEQUENCES:
        out = W.run_driver(exe, "self", name, env=env)
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
        with open(W.sequence_path(name)) as f:
            assert out.stdout == f.read(), name
