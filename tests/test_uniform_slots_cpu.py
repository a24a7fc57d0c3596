"""The uniform subwindows of both codecs (encoder.h EncUniform, decoder.h DecUniform) on the CPU test
double, whose control plane is built with SGPU_SLOT_CHECK (siamese_amd/Makefile):
every uniform subwindow keeps the slot records the per-element code would have
written, and every cover, demotion and teardown compares them with the
descriptor field by field and aborts on a difference -- in this file and in
every other hostsim test.

Here each rule of the range add's fast path runs at the smallest size at which
it can break (uniform_cases.py), through range calls and through per-packet
calls of the same library: harness configs against digests recorded from the
reference (tests/golden/make_uniform_golden.py), scripted ABI sequences with
the two call styles against each other.  The slot counters are printed at
exit, so the cases that assert on them run in a process of their own.
"""
import json
import os
import subprocess
import sys

import pytest

import golden
import scenario_lib as S
import uniform_cases as U

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(*args):
    env = dict(os.environ, SIAMESE_AMD_SLOT_COUNTS="1")
    out = subprocess.run([sys.executable, os.path.join(HERE, "uniform_cases.py"), S.SIM_LIB] + list(args),
                         capture_output=True, text=True, timeout=120, env=env, cwd=HERE)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    counts = {}
    for start, skip in (("slot counts:", 2), ("dec slot counts:", 3)):   # (encoder.cpp, decoder.cpp)
        line = [l for l in out.stderr.splitlines() if l.startswith(start)][-1].split()
        counts.update({line[i]: int(line[i + 1]) for i in range(skip, len(line), 2)})
    return json.loads(out.stdout.splitlines()[-1]), counts


def _demotions(c):
    return sum(v for k, v in c.items() if k.startswith("enc_demote_"))


@pytest.mark.parametrize("n", U.BLOCK_SIZES)
def test_block_range_calls_write_no_slot_record(n):
    """Block mode, 100 B, 30 % loss, range calls, sgpu_decode: the reference's
    digests; every encoder's subwindows enter the uniform state and no slot
    record is written, by an add, a row (Cauchy rows at 64 originals and
    below, Siamese rows above) or a teardown."""
    name = "uni_block%dr" % n
    got, c = _run(name, "batch")
    want = golden.load(name)
    assert got["digests"] == want["digests"] and got["status"] == want["status"]
    cfg = U.CONFIGS[name]
    assert c["encoders"] == cfg.streams
    assert c["enc_uniform"] == cfg.streams * ((n + 63) // 64)
    assert c["enc_slot_writes"] == 0 and _demotions(c) == 0
    # the decoder's subwindows enter too; with 30 % loss each is demoted once,
    # by the decode (matrix columns) or a later reader, never by an add
    # (a subwindow all of whose originals were lost, the 65th alone, is never entered)
    assert c["decoders"] == cfg.streams
    assert cfg.streams * (n // 64 or 1) <= c["dec_uniform"] <= cfg.streams * ((n + 63) // 64)
    assert c["dec_demote_add"] == c["dec_demote_length"] == c["dec_demote_stride"] == 0


@pytest.mark.parametrize("n", U.BLOCK_SIZES)
@pytest.mark.parametrize("path", ["dropin", "batch", "device_ge", "defer"])
def test_block_matches_reference(n, path):
    """The same blocks by per-packet calls (drop-in API and sgpu_decode) and by
    range calls through sgpu_decode_device and the deferred mode."""
    name = "uni_block%d%s" % (n, "r" if path in ("device_ge", "defer") else "")
    got = U.run_config(S.SIM_LIB, name, path)
    want = golden.load(name)
    assert got["digests"] == want["digests"] and got["status"] == want["status"]


def test_streaming_with_acks_rotates_uniform_subwindows():
    """Streaming, an acknowledgement per encode interval, range adds between
    them: remove_elements rotates subwindows out of the window, uniform ones
    without a walk.  A range add continues a descriptor only within the
    millisecond of its send stamp: a later call demotes the subwindow (cause
    stamp) and it stays per-element, so how many subwindows enter depends on
    the clock and only the floor is asserted: every encoder's first."""
    got, c = _run("uni_ack", "batch")
    want = golden.load("uni_ack")
    assert got["digests"] == want["digests"] and got["status"] == want["status"]
    assert c["enc_uniform"] >= c["encoders"] == U.CONFIGS["uni_ack"].streams
    assert c["enc_demote_length"] == c["enc_demote_stride"] == c["enc_demote_arq"] == 0
    for path in ("device_ge", "defer"):
        got = U.run_config(S.SIM_LIB, "uni_ack", path)
        assert got["digests"] == want["digests"] and got["status"] == want["status"]


@pytest.mark.parametrize("name", ["C1r", "C1var_r", "C2x64r"])
def test_existing_range_fixtures(name):
    """Lag-based acknowledgements, variable sizes (every subwindow demotes on
    a length) and the C2 leg, range calls, every byte hashed."""
    cfg = golden.config(name)
    res, rep = S.run_batch(S.SIM_LIB, cfg, verify=True, threads=2)
    want = golden.load(name)
    assert S.digests(res) == want["digests"] and rep.mismatches == 0
    assert [int(r.status) for r in res] == want["status"]


# case -> (what the counters must show)
API = {
    # decoder: duplicates inside ranges, originals after their recovery
    # (two decoders each: the one fed by single calls enters nothing)
    # the first subwindow enters, the single add demotes it; the second enters
    # and is demoted only by the decode (it has no lost slot: by the
    # elimination of its received data)
    "dec_duplicate": lambda c: (c["decoders"] == 2 and c["dec_uniform"] == 2 and c["dec_demote_add"] == 1 and
                                c["dec_demote_matrix"] + c["dec_demote_other"] == 1 and c["dec_demote_length"] == 0),
    # both subwindows enter and the decode demotes both; the late originals
    # are duplicates and write nothing more
    "dec_after_recovery": lambda c: c["dec_uniform"] == 2 and c["dec_demote_matrix"] == 2 and c["dec_demote_add"] == 0,
    # the first subwindow holds a record already: 63 of the range's originals
    # are placed one by one, the rest enter two subwindows (per encoder pair:
    # the single-call encoder enters none)
    "single_then_range": lambda c: c["enc_uniform"] == 2 and _demotions(c) == 0,
    "mixed_length": lambda c: c["enc_demote_length"] == 1 and c["enc_uniform"] == 1,
    "stride": lambda c: c["enc_demote_stride"] == 1,
    "bad_length": lambda c: c["enc_uniform"] == 2 and c["enc_slot_writes"] == 70,
    "max_packets": lambda c: c["enc_uniform"] >= 250,
    "fixed_block": lambda c: c["enc_uniform"] == 3 and c["enc_slot_writes"] == 130 and _demotions(c) == 0,
    "retransmit": lambda c: c["enc_demote_arq"] == 1,
    "restart_window": lambda c: c["enc_uniform"] >= 5,
}


@pytest.mark.parametrize("case", sorted(API))
def test_range_calls_match_single_calls(case):
    """Scripted sequences (uniform_cases.py case_*): what every call returns,
    *added and the first packet number included, and the bytes of the recovery
    packets made afterwards are those of single sgpu_encoder_add calls (for the
    decoder cases: sgpu_decoder_add_original calls and the recovered bytes); the
    counters report the entries and the demotion's cause.  (enc_slot_writes
    counts the single-call encoder's records too.)"""
    got, c = _run(case)
    assert got == {"ok": True}
    assert API[case](c), c
