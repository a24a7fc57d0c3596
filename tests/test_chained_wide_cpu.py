"""Chained device decodes of wide windows (DecoderCore::submit_chained with
rows of ldpcCount >= kLdpcSplitMin): CPU parity through the backend's CPU test
double (tests/hostsim, never shipped).

A block decode over a window of 512 originals or more has Siamese rows whose
LDPC picks run in k_ldpc before the OP_ROWS op that reads them.  Chained, those
items carry the gate of that op (ops.h LdpcItem): when the device elimination
finds a singular matrix they write nothing, the sums go back to their state
before the attempt and the host repeats the elimination.  The same checks run
on the MI355X in test_chained_wide_gpu.py.

The expected digests are data under tests/golden/wide_*.json: the reference
(oracle/_ref/libsiamese_ref.so) run through the loopback harness on the
configs below.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import pytest

import golden
import scenario_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_A = S.make_config(block_mode=1, streams=1, originals=640, payload_bytes=96, loss_pct=1,
                   recovery_loss_pct=1)
CONFIGS = {
    # (a) the smallest wide case: one k_ldpc tile per row, live bytes end at 96 + header
    "wide_a": _A,
    # (b) variable payload sizes, several decoders' gates in one launch
    "wide_b": S.replace(_A, payload_bytes=0, streams=8),
    # (c) two tiles per row and more than one k_ldpc item per row and tile
    "wide_c": S.replace(_A, originals=2048, payload_bytes=1400),
    # (a)'s shape over streams 184..191 of seed 1: one of them has a singular
    # first attempt (found on the CPU; a condition on the input)
    "wide_retry": S.replace(_A, streams=8, first_stream=184, seed=1),
}
RUN = {
    "wide_a": {},
    "wide_b": dict(threads=16, groups=2),
    "wide_c": {},
    "wide_retry": dict(threads=8, groups=2),
    "C3": {},
}
BLOCK = ["wide_a", "wide_b", "wide_c", "wide_retry"]


def engine_more():
    """The harness's engine counters past BatchReport.engine[] for the last
    batch run of this process (harness scenario_engine_more)."""
    out = (ctypes.c_uint64 * 4)()
    fn = S.lib().scenario_engine_more
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint]
    fn(out, 4)
    return [int(v) for v in out]


def run_batch(library, cfg, **kw):
    """S.run_batch, returning (results, report, engine dict): the harness's
    engine dict with ge_chained_wide (sgpu_engine_stats_ex[20])."""
    res, rep = S.run_batch(library, cfg, **kw)
    eng = S.engine_dict(rep)
    eng["ge_chained_wide"] = engine_more()[0]
    return res, rep, eng


def config(name):
    return CONFIGS[name] if name in CONFIGS else golden.config(name)


@functools.lru_cache(maxsize=None)
def runs(library, name):
    """(results, report, engine dict) of `name` with the host placement and
    with sgpu_decode_device, computed once per library."""
    cfg = config(name)
    host = run_batch(library, cfg, verify=True, **RUN[name])
    dev = run_batch(library, cfg, verify=True, device_ge=True, **RUN[name])
    return host, dev


def check_reference(library, name):
    _, (res, rep, _) = runs(library, name)
    want = golden.load(name)
    assert S.digests(res) == want["digests"]
    assert [int(r.status) for r in res] == want["status"]
    assert rep.mismatches == 0
    assert rep.checked > 0


def check_chained(library, name):
    _, (_, _, e) = runs(library, name)
    assert e["ge_chained_wide"] > 0
    if name in BLOCK:
        assert e["ge_jobs"] > 0 and e["ge_chained"] == e["ge_jobs"]


def check_accounting(library, name):
    (_, _, e0), (_, _, e1) = runs(library, name)
    assert e1["ldpc_bytes"] > 0
    for key in ("ref_op_bytes", "out_bytes", "ldpc_bytes"):
        assert e1[key] == e0[key], key


def check_retried(library, name):
    _, (_, _, e) = runs(library, name)
    assert e["ge_retried"] >= 1 and e["ge_chained_wide"] == e["ge_jobs"]


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_matches_reference(name):
    check_reference(S.SIM_LIB, name)


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_is_chained(name):
    check_chained(S.SIM_LIB, name)


@pytest.mark.parametrize("name", BLOCK + ["C3"])
def test_chained_wide_accounting(name):
    check_accounting(S.SIM_LIB, name)


def test_chained_wide_singular_retry():
    """A wide chained job whose matrix is singular: every wide job of this
    config is chained, one is retried on the host, and the results are still
    the reference's (test_chained_wide_matches_reference[wide_retry])."""
    check_retried(S.SIM_LIB, "wide_retry")
    check_reference(S.SIM_LIB, "wide_retry")


def test_every_wide_job_gated_off(monkeypatch):
    """SGPU_TEST_GE_FORCE_SINGULAR (hostsim only): every chained job reports
    a singular matrix, so every gated k_ldpc item, row batch and solve is
    skipped beside the encoders' ungated wide rows of the same launches.  The
    host retries give the reference's results, and the skipped attempts count
    no bytes."""
    name = "wide_b"
    (_, _, e0), _ = runs(S.SIM_LIB, name)
    monkeypatch.setenv("SGPU_TEST_GE_FORCE_SINGULAR", "1")
    res, rep, e = run_batch(S.SIM_LIB, config(name), verify=True, device_ge=True, **RUN[name])
    monkeypatch.delenv("SGPU_TEST_GE_FORCE_SINGULAR")
    want = golden.load(name)
    assert S.digests(res) == want["digests"] and rep.mismatches == 0 and rep.checked > 0
    assert e["ge_jobs"] > 0 and e["ge_retried"] == e["ge_jobs"] == e["ge_chained_wide"]
    for key in ("ref_op_bytes", "out_bytes", "ldpc_bytes"):
        assert e[key] == e0[key], key


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gate_unit_on_hostsim(tmp_path):
    """One gated and one ungated wide row through the hostsim backend with the
    outcome word forced to 0 (tests/chained_wide_gate_test.cpp)."""
    exe = tmp_path / "chained_wide_gate_test"
    csrc = os.path.join(ROOT, "siamese_amd", "csrc")
    flags = ["-O1", "-std=c++17", "-mavx2", "-pthread", "-I", csrc, "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "chained_wide_gate_test.cpp"),
                                      os.path.join(ROOT, "tools", "backend_hostsim.cpp"),
                                      os.path.join(csrc, "gf.cpp"), os.path.join(csrc, "codedef.cpp"),
                                      "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, SGPU_TEST_GE_FORCE_SINGULAR="1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gate ok" in out.stdout
    # (without the hook the same job succeeds and the gated row runs)
    env.pop("SGPU_TEST_GE_FORCE_SINGULAR")
    out = subprocess.run([str(exe), "open"], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "open ok" in out.stdout
