"""The solves on inconsistent recovery data: the cases shared by
test_solve_inconsistent_cpu.py (the CPU test double, tests/hostsim) and
test_solve_inconsistent_gpu.py (the solve kernels on the MI355X), driven
through the siamese_gpu.h ABI with ctypes like size_cases.py and ge_cases.py.

The solve's device forms (fused sweeps on 1 KiB or 256-byte tiles, split
sweeps, the product X = T R, the solve gated behind a chained k_ge job) agree
with one another only while the recovered rows are true originals: zero past
their recovered lengths.  The reference does not compute T R: its
BackSubstitution cuts each row to header + length as soon as its prefix is
solved, eliminates only the cut row from the rows above, and stops with
Siamese_Disabled at the first invalid prefix.  Here one received original
reaches the decoder altered -- one byte flipped, or handed over short, so that
its length prefix disagrees with the encoder's -- while the encoder summed the
true bytes.  The decode then either succeeds with wrong packets, the
reference's wrong packets to the byte, or disables the decoder at the call the
reference does.

A case is one or more streams (Stream below): all originals to an encoder,
its recovery packets by sgpu_encode_range, a decoder given every original but
the lost ones (the edited one by a per-packet call from a buffer of its own,
deliver_cases.Stream `given`) and every recovery packet.  Every case runs in
one process on fresh codecs with sgpu_decode, and again with
sgpu_decode_device (PENDING, flush, the result): every recovery packet covers
the whole window, so the rows have one length and a square job is chained.
Checked, most independent first:

  1. every recovery packet (DataBytes, FooterBytes, sha256 of its bytes read
     from DeviceData) against the reference's, recorded in
     tests/golden/solve_inconsistent.json by tests/golden/make_solve_golden.py
     -- and against a live run of the reference where oracle/_ref is built;
  2. every decode call's result code and packet count against the reference's
     (a corrupt prefix is found on the device: the batch ABI reports it once
     the flush has completed, DESIGN.md section 6, so there a Disabled case's
     first call may still answer Success and every call after the flush must
     answer Disabled);
  3. every packet the decode returns -- number, length, sha256 -- against the
     reference's record: the reference's wrong bytes, not the originals; read
     from device memory, and delivered into guarded rows (tail zero up to the
     stride, guards intact), where every received original arrives as the
     decoder was given it;
  4. the drop-in siamese_decode of the library under test answers every call
     as the reference did, bytes included; a Disabled decoder answers
     DISABLED to sgpu_decoder_deliver_range;
  5. the path by counters: solves, solves_flagged ([40]: the product came
     back flagged and the sweeps redid the solve), solves_cut ([41]: word 0
     below m) and, for the device placement, ge_jobs and ge_chained.

What selects each form (ops.h): solve_split = 16 solves in a launch or m >=
kSolveSplitMinRows = 16; the product up to kProductMaxRows = 120 rows unless
SGPU_TR_SOLVE=0; 256-byte tiles above kSolveWideMaxRows = 120.  So a
successful decode is flagged exactly when solve_split holds, m <= 120 and the
product path is on (`flagged` below); the test double has no product.

Payloads are size_cases.payloads (SHAKE-256 of seed and index).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import deliver_cases as D
import scenario_lib as S
import size_cases as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_inconsistent.json")

SPLIT_MIN_ROWS, PRODUCT_MAX_ROWS, SPLIT_MIN_SOLVES = 16, 120, 16
DECODES = 2    # calls per stream: the decode, and the one after it


def spread(n, count, seed, avoid=()):
    """n distinct indices below count, none of `avoid`, drawn by SHAKE-256 of
    the seed and the index."""
    order = sorted((i for i in range(count) if i not in avoid),
                   key=lambda i: hashlib.shake_256(b"solve:%d:%d" % (seed, i)).digest(8))
    assert n <= len(order)
    return tuple(sorted(order[:n]))


def ramp(count, top, base=40, step=37):
    """base + step * i mod top: neighbours differ, the lengths spread evenly."""
    return tuple(base + (step * i) % top for i in range(count))


class Stream:
    """lengths, seed: the originals.  lost, recovery: the loss set and the
    recovery packets made.  edit: None, ("flip", index, off, val): payload
    byte `off` of received original `index` XOR val, or ("cut", index, n):
    the first len - n bytes of it."""

    def __init__(self, seed, lengths, lost, recovery, edit=None):
        self.seed, self.lengths, self.lost, self.recovery = seed, tuple(lengths), tuple(lost), recovery
        self.edit = tuple(edit) if edit else None
        assert len(set(self.lost)) == len(self.lost) == recovery and max(self.lost) < len(self.lengths)
        if self.edit:
            kind, index, arg = self.edit[:3]
            assert kind in ("flip", "cut") and index not in self.lost
            assert 0 < arg < self.lengths[index] if kind == "cut" else 0 <= arg < self.lengths[index]
            assert kind == "cut" or 0 < self.edit[3] < 256

    def given(self, data):
        """{index: bytes}: what the decoder is handed in place of the true
        original."""
        if not self.edit:
            return {}
        kind, index, arg = self.edit[:3]
        d = bytearray(data[index])
        if kind == "flip":
            d[arg] ^= self.edit[3]
        else:
            d = d[:len(d) - arg]
        return {index: bytes(d)}

    def flip_symbol_offset(self):
        kind, index, arg = self.edit[:3]
        return Z.prefix_bytes(self.lengths[index]) + arg

    def lost_symbol_bytes(self):
        return [Z.prefix_bytes(self.lengths[i]) + self.lengths[i] for i in self.lost]


class Case:
    """streams: decoded one after another and completed by one flush.
    result: the reference's answer to the edited stream's decode, fixed here
    by name so that a regenerated record cannot quietly change what a case is
    for."""

    def __init__(self, streams, result=D.SUCCESS):
        self.streams = tuple(streams) if isinstance(streams, (list, tuple)) else (streams,)
        self.result = result
        self.edited = [k for k, s in enumerate(self.streams) if s.edit]
        assert len(self.edited) == 1 and result in (D.SUCCESS, D.DISABLED)
        self.m = self.streams[self.edited[0]].recovery

    def split(self):
        return len(self.streams) >= SPLIT_MIN_SOLVES or max(s.recovery for s in self.streams) >= SPLIT_MIN_ROWS

    def flagged(self):
        """Solves the default device path must report flagged."""
        return 1 if self.result == D.SUCCESS and self.split() and self.m <= PRODUCT_MAX_ROWS else 0

    def cut(self):
        return 1 if self.result == D.DISABLED else 0


W100 = ramp(100, 260)          # 40 to 299 bytes: one- and two-byte prefixes
W300 = ramp(300, 260)
LOST10 = (3, 10, 22, 35, 47, 58, 63, 77, 81, 96)


def siamese(m, edit, lengths=W100, seed=1, lost=None):
    """m lost of a Siamese window (more than kCauchyThreshold = 64 originals),
    m recovery packets: one square m x m solve."""
    lost = lost or spread(m, len(lengths), m, avoid=(edit[1],))
    return Stream(seed, lengths, lost, m, edit)


# tile2_wide: 100 originals of 40 to 2599 bytes, 20 lost; original 29 has 2573
# bytes, and its payload byte 2100 is symbol byte 2102: only the third 1 KiB
# tile (2048 to 3071) of the rows has bytes past a length.
WIDE = ramp(100, 2560, step=617)
# tile2_narrow: 300 originals of 40 to 699 bytes, 130 lost; payload byte 600 of
# original 17 (669 bytes) is symbol byte 602, in the third 256-byte tile.
NARROW = ramp(300, 660)
# flip_in_head: the window of fused_10 with originals 22 and 58, both lost, cut
# down to 3 and 5 bytes, below symbol byte 7 = payload byte 5 of original 7.
HEAD = tuple(3 if i == 22 else 5 if i == 58 else n for i, n in enumerate(W100))
# the Cauchy window of the cut cases: 40 originals (at most kCauchyThreshold),
# the longest received one (original 11, 213 bytes) handed over short
C40 = ramp(40, 200, base=30, step=53)
C40_LOST = (1, 8, 15, 22, 30, 39)
C40_CUT = max((n, i) for i, n in enumerate(C40) if i not in C40_LOST)[1]

CASES = {
    # m = 10 < 16 and one solve: k_solve_main's fused sweeps (solve_tile_lds).
    # The flip at payload byte 160 of original 7 (299 bytes) is symbol byte
    # 162; lost symbols of 75 to 297 bytes lie on both sides of it.
    "fused_10": Case(siamese(10, ("flip", 7, 160, 0x5a), lost=LOST10)),
    "fused_10_flip100": Case(siamese(10, ("flip", 7, 100, 0x5a), lost=LOST10)),
    "fused_10_flip290": Case(siamese(10, ("flip", 7, 290, 0x5a), lost=LOST10)),
    # the kSolveSplitMinRows edge: 15 fused, from 16 the product solve,
    # flagged back to the sweeps behind k_solve_pre's prefixes; 16 and 17 are
    # k_solve_tr's two-rows-per-wave and three (four) variants
    "fused_15": Case(siamese(15, ("flip", 7, 160, 0x5a))),
    "split_16": Case(siamese(16, ("flip", 7, 160, 0x5a))),
    "split_17": Case(siamese(17, ("flip", 7, 160, 0x5a))),
    # a window of 300: the last product size, the first solve on 256-byte
    # tiles (solve_tile_narrow; sweeps only), the largest solve
    "product_120": Case(siamese(120, ("flip", 7, 160, 0x5a), W300)),
    "narrow_121": Case(siamese(121, ("flip", 7, 160, 0x5a), W300)),
    "narrow_255": Case(siamese(255, ("flip", 7, 160, 0x5a), W300)),
    # only the third tile has bytes past a length: tiles 0 and 1 are
    # consistent, the flag still sends the whole solve to the sweeps
    "tile2_wide": Case(siamese(20, ("flip", 29, 2100, 0x5a), WIDE, seed=2)),
    "tile2_narrow": Case(siamese(130, ("flip", 17, 600, 0x5a), NARROW, seed=3)),
    # inside the 16 bytes SolveDesc.head carries: the rows' first lane is
    # wrong while every prefix byte is intact
    "flip_in_head": Case(Stream(4, HEAD, LOST10, 10, ("flip", 7, 5, 0x5a))),
    # 17 decoders of 3 lost each, completed by one flush: solve_split holds by
    # count, so m = 3 runs as a product; decoder 5's comes back flagged, and
    # that solve alone goes back to the sweeps
    "many_small": Case([Stream(100 + k, W100, (10, 47, 92), 3, ("flip", 7, 160, 0x5a) if k == 5 else None)
                        for k in range(17)]),
    # m = 20 behind a chained k_ge job (sgpu_decode_device): the gated solve
    # is flagged
    "block_chained": Case(siamese(20, ("flip", 7, 160, 0x5a), seed=5)),
    # The Cauchy window, its longest received original short by n bytes: its
    # prefix disagrees with the encoder's.  make_solve_golden.py walks n = 1
    # to 59 and fixes the smallest n of each outcome here: valid prefixes of
    # wrong lengths (Success, every packet wrong, heavy clipping), or an
    # invalid one (Disabled).
    "cut_success": Case(Stream(6, C40, C40_LOST, 6, ("cut", C40_CUT, 1))),
    "cut_disabled": Case(Stream(6, C40, C40_LOST, 6, ("cut", C40_CUT, 3)), D.DISABLED),
    # Disabled on the product path's prefix pass (k_solve_pre leaves word 0
    # below m: k_solve_tr skips the solve) and on 256-byte tiles
    "cut_disabled_16": Case(siamese(16, ("cut", 7, 1)), D.DISABLED),
    "cut_disabled_130": Case(siamese(130, ("cut", 7, 1), W300), D.DISABLED),
}

# the cases that run again with SGPU_TR_SOLVE=0 on the device: m >= 16, and
# many_small
SWEEPS_AGAIN = [n for n, c in CASES.items() if c.split()]


def describe(stream, packets, decodes, returned):
    """What solve_inconsistent.json records of a stream: its recovery
    packets as size_cases.describe does, every decode call's [result,
    packets], and of the packets the first decode returned [number, length,
    sha256]."""
    longest = max(Z.prefix_bytes(n) + n for n in stream.lengths)
    return {
        "originals": len(stream.lengths),
        "lengths_sha256": hashlib.sha256(json.dumps(stream.lengths).encode()).hexdigest(),
        "lost": list(stream.lost),
        "edit": list(stream.edit) if stream.edit else None,
        "recovery": [{"bytes": len(p), "footer_bytes": len(p) - longest, "sha256": hashlib.sha256(p).hexdigest()}
                     for p in packets],
        "decodes": decodes,
        "packets": [[num, len(d), hashlib.sha256(d).hexdigest()] for num, d in returned],
    }


def dropin_run(path, stream, data):
    """The stream through the siamese.h API of the library at `path`: its
    recovery packets, DECODES decode calls' [result, packets], and the
    packets of the first."""
    lib = Z.binding().SiameseLib(path).init()
    enc, dec = lib.Encoder(), lib.Decoder()
    for i, d in enumerate(data):
        assert enc.add(d) == i
    packets = [enc.encode() for _ in range(stream.recovery)]
    assert all(packets)
    given = stream.given(data)
    for i, d in enumerate(data):
        if i not in stream.lost:
            assert dec.add_original(i, given.get(i, d)) == 0
    for p in packets:
        assert dec.add_recovery(p) == 0
    decodes, returned = [], []
    for call in range(DECODES):
        rc, out = dec.decode_raw()
        decodes.append([rc, len(out) if out else 0])
        if call == 0 and out:
            returned = sorted(out)
    enc.close()
    dec.close()
    return packets, decodes, returned


def conditions(name, case, wants, datas):
    """What keeps a case from passing vacuously, asserted of the record."""
    for k, (s, want, data) in enumerate(zip(case.streams, wants, datas)):
        what = "%s, stream %d" % (name, k)
        mine = describe(s, [], [], [])
        for key in ("originals", "lengths_sha256", "lost", "edit"):
            assert want[key] == mine[key], "%s: solve_inconsistent.json was made for other %s: run " \
                "tests/golden/make_solve_golden.py" % (what, key)
        assert len(want["recovery"]) == s.recovery and len(want["decodes"]) == DECODES
        true = [[i, len(data[i]), hashlib.sha256(data[i]).hexdigest()] for i in sorted(s.lost)]
        if not s.edit:
            assert want["decodes"] == [[D.SUCCESS, len(s.lost)], [D.NEED_MORE, 0]] and want["packets"] == true, \
                "%s: an unedited stream must decode to its originals" % what
            continue
        if case.result == D.DISABLED:
            assert want["decodes"] == [[D.DISABLED, 0]] * DECODES and want["packets"] == [], \
                "%s: the reference does not answer Disabled: %r" % (what, want["decodes"])
        else:
            assert want["decodes"] == [[D.SUCCESS, len(s.lost)], [D.NEED_MORE, 0]], \
                "%s: the reference does not answer Success: %r" % (what, want["decodes"])
            assert [p[0] for p in want["packets"]] == sorted(s.lost)
            assert want["packets"] != true, "%s: every returned packet is its original" % what
        if s.edit[0] == "flip":
            at, sym = s.flip_symbol_offset(), s.lost_symbol_bytes()
            assert any(b <= at for b in sym) and any(b > at for b in sym), \
                "%s: lost symbols of %r bytes do not lie on both sides of symbol byte %d" % (what, sorted(sym), at)
            # (the large solves: the flip lies above at least a third of the lost lengths)
            assert len(sym) < PRODUCT_MAX_ROWS or 3 * sum(b <= at for b in sym) >= len(sym), what


def reference_check(case, wants, datas):
    for s, want, data in zip(case.streams, wants, datas):
        packets, decodes, returned = dropin_run(S.REF_LIB, s, data)
        assert describe(s, packets, decodes, returned) == want, \
            "solve_inconsistent.json is stale: run tests/golden/make_solve_golden.py"


_expected = {}


def expected(name):
    """Per stream of the case, its payloads and the reference's record; where
    the reference is built, a live run of it must agree with the record
    first."""
    if name not in _expected:
        case = CASES[name]
        with open(GOLDEN) as f:
            cases = json.load(f)["cases"]
        assert name in cases, "%s is not in solve_inconsistent.json: run tests/golden/make_solve_golden.py" % name
        wants = cases[name]
        assert len(wants) == len(case.streams)
        datas = [Z.payloads(s) for s in case.streams]
        conditions(name, case, wants, datas)
        if os.path.exists(S.REF_LIB):
            reference_check(case, wants, datas)
        _expected[name] = (datas, wants)
    return _expected[name]


def product_on():
    v = os.environ.get("SGPU_TR_SOLVE")
    if v is None:
        return True
    try:
        return int(v) != 0
    except ValueError:
        return False


def run_once(L, name, case, datas, wants, device, what):
    """One placement of the case on fresh codecs: checks 1 to 3 and the
    DISABLED delivery of 4; returns the counters' growth."""
    e0 = Z.engine(L)      # (every earlier run ended with a flush: nothing of theirs is still queued)
    sts = [D.Stream(L, s.lengths, lost=s.lost, recovery=s.recovery, data=data, given=s.given(data))
           for s, data in zip(case.streams, datas)]
    assert L.sgpu_flush() == 0

    # 1. the recovery packets are the reference's
    for k, (st, want) in enumerate(zip(sts, wants)):
        for j, w in enumerate(want["recovery"]):
            r = st.recs[j]
            assert (r.DataBytes, r.FooterBytes) == (w["bytes"], w["footer_bytes"]), \
                "%s: stream %d recovery packet %d: %d bytes with a %d-byte footer, the reference's has %d with %d" % (
                    what, k, j, r.DataBytes, r.FooterBytes, w["bytes"], w["footer_bytes"])
            assert hashlib.sha256(D.read(L, r.DeviceData, r.DataBytes)).hexdigest() == w["sha256"], \
                "%s: stream %d recovery packet %d (%d bytes) differs from the reference's" % (what, k, j, r.DataBytes)

    # 2. the first decode of every stream, then one flush for all of them
    f = L.sgpu_decode_device if device else L.sgpu_decode
    pending = 0
    if device:
        for st in sts:
            out, got = C.POINTER(D.Orig)(), C.c_uint(0)
            r = f(st.dec, C.byref(out), C.byref(got))
            assert r == D.PENDING, "%s: sgpu_decode_device queued no matrix job: %d" % (what, r)
            pending += 1
        assert L.sgpu_flush() == 0
    outs = []
    for k, (st, want) in enumerate(zip(sts, wants)):
        out, got = C.POINTER(D.Orig)(), C.c_uint(0)
        r = f(st.dec, C.byref(out), C.byref(got))
        rc, n = want["decodes"][0]
        if rc == D.DISABLED:
            # (found on the device: reported once the flush has completed)
            assert (r, got.value) in ((D.SUCCESS, len(case.streams[k].lost)), (D.DISABLED, 0)), \
                "%s: stream %d: the decode returned %d with %d packets" % (what, k, r, got.value)
        else:
            assert (r, got.value) == (rc, n), "%s: stream %d: the decode returned %d with %d packets, the " \
                "reference's %d with %d" % (what, k, r, got.value, rc, n)
        outs.append((out, got.value if r == D.SUCCESS else 0))
    assert L.sgpu_flush() == 0
    e1 = Z.engine(L)

    # 3. the packets the decodes returned, from device memory
    returned = []
    for k, (st, want, (out, n)) in enumerate(zip(sts, wants, outs)):
        mine = {}
        if want["decodes"][0][0] == D.SUCCESS:
            assert n == len(want["packets"])
            for j, (num, length, sha) in enumerate(want["packets"]):
                o = [out[i] for i in range(n) if out[i].PacketNum == num]
                assert len(o) == 1, "%s: stream %d: packet %d returned %d times" % (what, k, num, len(o))
                assert o[0].DataBytes == length, "%s: stream %d: packet %d has %d bytes, the reference's %d" % (
                    what, k, num, o[0].DataBytes, length)
                mine[num] = D.read(L, o[0].Data, length)
                assert hashlib.sha256(mine[num]).hexdigest() == sha, \
                    "%s: stream %d: packet %d (%d bytes) differs from the reference's" % (what, k, num, length)
        returned.append(mine)

    # 2. the calls after the first
    for k, (st, want) in enumerate(zip(sts, wants)):
        for call in range(1, DECODES):
            out, got = C.POINTER(D.Orig)(), C.c_uint(0)
            r = L.sgpu_decode(st.dec, C.byref(out), C.byref(got))
            assert (r, got.value) == tuple(want["decodes"][call]), "%s: stream %d: decode call %d returned %d with " \
                "%d packets, the reference's %r" % (what, k, call, r, got.value, want["decodes"][call])

    # 3. the whole window into guarded rows, 4. or DISABLED
    for k, (s, st, want, data, mine) in enumerate(zip(case.streams, sts, wants, datas, returned)):
        count = len(s.lengths)
        rows = D.Rows(L, count, (max(s.lengths) + 16) & ~15)
        if want["decodes"][0][0] == D.DISABLED:
            _, queued = D.deliver(L, st.dec, 0, count, rows, want=D.DISABLED)
            assert queued == 0
            assert L.sgpu_flush() == 0
            assert rows.untouched()
        else:
            res, queued = D.deliver(L, st.dec, 0, count, rows)
            assert res == [D.SUCCESS] * count and queued == count
            assert L.sgpu_flush() == 0
            got, lens = rows.fetch()
            given = s.given(data)
            for i in range(count):
                d = mine[i] if i in s.lost else given.get(i, data[i])
                D.check_row(got[i], lens[i], d, "%s: stream %d packet %d (%d bytes%s)" % (
                    what, k, i, len(d), ", recovered" if i in s.lost else ", as given" if i in given else ""))
        rows.free()
    for st in sts:
        st.free()
    grew = {k: e1[k] - e0[k] for k in ("solves", "solves_flagged", "solves_cut", "ge_jobs", "ge_chained")}
    assert grew["ge_jobs"] == pending
    return grew


def check(name, path):
    L = D.load(path)
    case = CASES[name]
    datas, wants = expected(name)
    host = run_once(L, name, case, datas, wants, False, name + " (sgpu_decode)")
    dev = run_once(L, name, case, datas, wants, True, name + " (sgpu_decode_device)")
    print("%s: host %r\n%s: device %r" % (name, host, name, dev))

    # 4. the drop-in API of the same library, call by call and byte by byte
    k = case.edited[0]
    s, want = case.streams[k], wants[k]
    packets, decodes, returned = dropin_run(path, s, datas[k])
    mine = describe(s, packets, decodes, returned)
    assert mine["recovery"] == want["recovery"], "%s: the drop-in encoder's packets differ from the reference's" % name
    assert mine["decodes"] == want["decodes"], "%s: siamese_decode answered %r, the reference %r" % (
        name, mine["decodes"], want["decodes"])
    assert mine["packets"] == want["packets"], "%s: siamese_decode's packets differ from the reference's" % name

    # 5. the path
    flagged = case.flagged() if path != S.SIM_LIB and product_on() else 0
    n = len(case.streams)
    for grew, what in ((host, "sgpu_decode"), (dev, "sgpu_decode_device")):
        assert grew["solves"] == n, "%s: %s: %d solves for %d decodes" % (name, what, grew["solves"], n)
        assert grew["solves_flagged"] == flagged, "%s: %s: %d flagged solves, expected %d" % (
            name, what, grew["solves_flagged"], flagged)
        assert grew["solves_cut"] == case.cut(), "%s: %s: %d solves stopped at a prefix, expected %d" % (
            name, what, grew["solves_cut"], case.cut())
    assert (host["ge_jobs"], host["ge_chained"]) == (0, 0)
    assert (dev["ge_jobs"], dev["ge_chained"]) == (n, n), "%s: %d device jobs, %d chained, expected %d of each" % (
        name, dev["ge_jobs"], dev["ge_chained"], n)
    return host, dev


def check_in_child(name, path, env):
    """check() in a fresh process with `env` added to the environment (knobs
    the library reads once per process)."""
    code = "import sys; sys.path.insert(0, %r); import solve_cases; solve_cases.check(%r, %r); print('ok')" % (
        os.path.dirname(os.path.abspath(__file__)), name, path)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=300, cwd=S.ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
