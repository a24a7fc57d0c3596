"""Every path at the 22-bit packet-number wrap: the cases shared by
test_wrap_cpu.py (the CPU test double, tests/hostsim) and test_wrap_gpu.py
(the HIP kernels on the MI355X), driven through the siamese_gpu.h ABI with
ctypes like size_cases.py and exec_shape_cases.py.

Packet numbers are columns modulo kColumnPeriod = 0x400000 (codedef.h).  A
fresh decoder refuses packets far from 0, so a pair has to walk there.

Parking (park): N encoder/decoder pairs go in lock-step from column 0 to PARK =
0x400000 - 1280, STEP one-byte originals at a time.  Per step and pair: one
sgpu_encoder_add_range, one sgpu_decoder_add_original_range of the same
originals, sgpu_encoder_remove_before(the step's first packet), one
sgpu_encode handed to the decoder, and the decoder's sgpu_decoder_ack fed to
sgpu_encoder_acknowledge (an encoder takes an ack only within 2^21 packets of
the last one it took: without them it would drop every ack at the wrap as out
of order); then one flush for all pairs.  STEP = 8000: the remove comes after
the add, so two steps must fit the 16 000-packet window.  Every range add's
packet number and every ack's nextExpected is asserted, and the sha256 over
every recovery packet of the walk (length, footer length, bytes) and every ack
message must be the one the reference's pair produced on the same schedule (wrap_edges.json, "walk"): a
divergence before the wrap is not blamed on the wrap.  Original i of the walk
is byte i of SHAKE-256("wrap:walk").

A case then takes one parked pair, fills up to its window's first packet with
more one-byte originals, empties the encoder's window, and plays its schedule
across the wrap:

  ("add", k)            the next k originals: one sgpu_encoder_add_range, the
                        received ones to the decoder in unbroken stretches by
                        sgpu_decoder_add_original_range
  ("encode", k)         k sgpu_encode calls, each packet handed to the decoder
                        and copied bare into a guarded row
  ("remove_before", i)  sgpu_encoder_remove_before(packet number of original i)
  ("decode",)           flush, then sgpu_decode / sgpu_decode_device until the
                        losses so far are back, or a call fails

Checked against tests/golden/wrap_edges.json, which
tests/golden/make_wrap_golden.py records from the reference walking and
playing the same schedules: DataBytes, FooterBytes and sha256 of every
recovery packet; result, packet numbers, lengths and sha256 of every decode
call's packets in the order returned.  Then every original of the live window
is delivered across the wrap into guarded rows and compared with what this
file generated, and the engine counters must show the path the case is named
for.  Payloads are SHAKE-256 of the case's seed and the packet's index;
lengths cycle through exec_shape_cases.LENGTHS, and every decode's loss set
has a packet that ends in the last 256-byte tile of the longest symbol.

check_ranges: the range calls with firstPacketNum below the wrap and
firstPacketNum + count past it, against rows, frames and streams built here.
check_arq: acknowledgements and retransmissions across the wrap against the
reference's recorded messages and order.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import arq_cases as A
import deliver_cases as D
import exec_shape_cases as X
import frame_cases as F
import pack_cases as P
import relay_cases as R
import relaypack_cases as RP
import scenario_lib as S
import size_cases as Z
import stream_cases as ST
from siamese_amd.binding import OriginalPacket, RecoveryPacket, SiameseLib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrap_edges.json")

PERIOD = 0x400000            # kColumnPeriod
MASK = PERIOD - 1            # SIAMESE_PACKET_NUM_MAX
PARK = PERIOD - 1280
STEP = 8000
FLOW = F.FLOW
LONG = X.LONG


def walk_bytes():
    return hashlib.shake_256(b"wrap:walk").digest(PERIOD)


def steps():
    """[(first packet, count)] of the walk."""
    return [(a, min(STEP, PARK - a)) for a in range(0, PARK, STEP)]


def walk_update(h, data, footerBytes):
    h.update(len(data).to_bytes(4, "little") + footerBytes.to_bytes(4, "little") + data)


# ---- the cases ---------------------------------------------------------------
class Case:
    """before: originals of the case below the wrap (original `before` is
    packet 0).  lost: indices the decoder never receives.  device: decodes by
    sgpu_decode_device: every region the decoder finds has as many packets as
    losses (it stops at the first packet that suffices; ge_cases.py on why
    rows > columns never reach k_ge) and the rows of a case are of one length,
    so every matrix job must be chained.  wide: k_ldpc must have run."""

    def __init__(self, seed, before, schedule, lost, device=False, wide=False, fixed=0):
        self.seed, self.before, self.lost = seed, before, tuple(sorted(set(lost)))
        self.schedule = tuple(tuple(s) for s in schedule)
        self.device, self.wide = device, wide
        count = sum(s[1] for s in self.schedule if s[0] == "add")
        # fixed: every original that long, added with fixedBytes and no bytes[] (the uniform subwindows)
        self.fixed = fixed
        self.lengths = (fixed,) * count if fixed else X.lengths(count, 3, seed)
        self.recovery = sum(s[1] for s in self.schedule if s[0] == "encode")
        self.first = PERIOD - before
        assert PARK <= self.first < PERIOD and before < count
        # every decode: losses on the decoder's side of its window, one of them a long packet
        added, kept, open_ = 0, 0, []
        groups = []
        for s in self.schedule:
            if s[0] == "add":
                open_ += [i for i in self.lost if added <= i < added + s[1]]
                added += s[1]
            elif s[0] == "remove_before":
                kept = s[1]
                assert all(i >= kept for i in open_), "a lost packet the encoder's window has left"
            elif s[0] == "decode":
                groups.append(tuple(open_))
                open_ = []
        assert not open_ and sum(len(g) for g in groups) == len(self.lost)
        for g in groups:
            assert max(self.lengths[i] for i in g) + 3 > (max(self.lengths) + 2) // 256 * 256, \
                "a lost packet must end in the last 256-byte tile of the longest symbol"
        self.groups = groups
        assert min(groups[0]) < before <= max(groups[0]), "the first decode loses packets on both sides of the wrap"

    def num(self, i):
        return (self.first + i) & MASK

    def kept_from(self):
        return max([s[1] for s in self.schedule if s[0] == "remove_before"] or [0])

    def spec_sha256(self):
        return hashlib.sha256(json.dumps([self.seed, self.before, self.schedule, self.lost,
                                          self.fixed]).encode()).hexdigest()


def long_at(seed, lo, hi, want):
    """`want` indices of 600-byte originals of lengths(.., 3, seed) in [lo, hi), spread evenly."""
    at = [i for i in range(lo, hi) if (i - X.long_at(seed)) % 8 == 0]
    assert len(at) >= want
    return tuple(at[k * len(at) // want] for k in range(want))


def _cases():
    c = {}
    # 1. window <= kCauchyThreshold (64) straddling the wrap: Cauchy rows, m = 6 <
    # kSolveSplitMinRows.  0x3fffff (19) and 0 (20) are lost.  Then the stream
    # goes on (8.): the window wholly past 0, Siamese rows over 100 originals.
    lost = (3, 19, 20, 21, 40) + long_at(1, 8, 19, 1)
    c["cauchy48"] = Case(1, 20, [("add", 48), ("encode", 7), ("decode",), ("remove_before", 48), ("add", 100),
                                 ("encode", 6), ("decode",)], lost + (60, 101) + long_at(1, 110, 148, 2))
    # 2. Siamese windows (k_exec's picks), single encodes between adds so that
    # versioned batches join across the wrap; about 200, m = 8, on the device
    lost = (5, 89, 90, 91, 150) + long_at(2, 20, 190, 3)
    c["siamese200"] = Case(2, 90, [("add", 84)] + [("add", 4), ("encode", 1)] * 4 + [("add", 100), ("encode", 8),
                                                                                    ("decode",)], lost, device=True)
    # about 450; m = 19 (original 300 is one of the fifteen long ones) >= kSolveSplitMinRows: the split solve, the product X = T R
    # (or with SGPU_TR_SOLVE=0 the two sweeps)
    lost = (0, 299, 300, 301, 449) + long_at(3, 10, 440, 15)
    c["siamese450"] = Case(3, 300, [("add", 292)] + [("add", 2), ("encode", 1)] * 4 + [("add", 150), ("encode", 20),
                                                                                     ("decode",)], lost)
    # 3. window >= kLdpcSplitMin (512): the rows' picks go to k_ldpc.  As many
    # packets as losses, made in one stretch: square, rows of one length, so
    # sgpu_decode_device chains k_ge -> gated rows -> solve in one submission
    lost = (249, 250, 599) + long_at(4, 100, 500, 2)
    c["wide600"] = Case(4, 250, [("add", 600), ("encode", 5), ("decode",)], lost, device=True, wide=True)
    # 5. m = kSolveSplitMinRows, square, Cauchy window of exactly 64: chained, split solve
    lost = (29, 30, 31, 63) + long_at(5, 0, 29, 3) + long_at(5, 32, 62, 3) + (1, 3, 10, 40, 45, 50)
    c["split16"] = Case(5, 30, [("add", 64), ("encode", 16), ("decode",)], lost, device=True)
    # 4. remove_before across the wrap: a first kept packet below it, encodes, a
    # decode; then one past it, more adds and encodes, a second decode
    lost1 = (120, 149, 150, 151) + long_at(6, 160, 290, 2)
    lost2 = (310, 395, 405) + long_at(6, 320, 390, 1)
    c["trim"] = Case(6, 150, [("add", 300), ("encode", 3), ("remove_before", 100), ("encode", 5), ("decode",),
                              ("add", 100), ("encode", 2), ("remove_before", 200), ("encode", 2), ("add", 20),
                              ("encode", 3), ("decode",)], lost1 + lost2)
    # fixed-length range adds: the uniform subwindows of the encoder and the decoder
    # (one column and one length per subwindow, decoder.cpp add_original_range)
    # with the wrap inside a range, Siamese rows over 120 originals of 257 bytes
    # (0x3ffffe and 3 are lost: the decoder's range 0x3fffff..2 crosses the wrap in one call)
    c["uniform120"] = Case(8, 45, [("add", 50), ("encode", 2), ("add", 70), ("encode", 6), ("decode",)],
                           (2, 30, 43, 48, 60, 119), fixed=257)
    return c


CASES = _cases()
RANGES, ARQ = "ranges", "arq"
ALL = list(CASES) + [RANGES, ARQ]


def payloads(case):
    return [hashlib.shake_256(b"wrap:%d:%d" % (case.seed, i)).digest(n) for i, n in enumerate(case.lengths)]


def describe_packet(p, longest):
    return {"bytes": len(p), "footer_bytes": len(p) - longest, "sha256": hashlib.sha256(p).hexdigest()}


def longest_symbol(lengths):
    return max(Z.prefix_bytes(n) + n for n in lengths)


# ---- the siamese.h side: the reference (make_wrap_golden.py; needs oracle/_ref)
# ---- and the drop-in API of the library under test (check_dropin) -------------
ACK_LIMIT = 64


class ApiPair:
    """An encoder and a decoder of a siamese.h library walked to PARK by the
    walk's schedule, call by call."""

    def __init__(self, path=S.REF_LIB):
        self.lib = lib = SiameseLib(path).init()
        self.enc, self.dec = lib.encoder_create(), lib.decoder_create()
        W = walk_bytes()
        buf = (C.c_ubyte * 1)()
        p = OriginalPacket(0, 1, buf)
        pr, add, recv, e, d = C.byref(p), lib.encoder_add, lib.decoder_add_original, self.enc, self.dec
        rp = RecoveryPacket()
        h = hashlib.sha256()
        self.packets = 0
        for a, n in steps():
            for i in range(a, a + n):
                buf[0] = W[i]
                if add(e, pr) or p.PacketNum != i or recv(d, pr):
                    raise RuntimeError("the reference's walk stopped at packet %d" % i)
            assert lib.encoder_remove_before(e, a) == 0
            assert lib.encode(e, C.byref(rp)) == 0
            data = C.string_at(rp.Data, rp.DataBytes)
            walk_update(h, data, len(data) - 2)    # (a one-byte symbol behind its one-byte prefix)
            assert lib.decoder_add_recovery(d, C.byref(rp)) == 0
            rc, msg = self.ack()
            assert rc == 0 and self.acknowledge(msg) == (0, a + n), "the walk's ack at %d" % a
            h.update(msg)
            self.packets += 1
        self.sha256 = h.hexdigest()
        self.W = W

    def add(self, data):
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        p = OriginalPacket(0, len(data), buf)
        rc = self.lib.encoder_add(self.enc, C.byref(p))
        return rc, p.PacketNum, p

    def recv(self, num, data):
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        return self.lib.decoder_add_original(self.dec, C.byref(OriginalPacket(num, len(data), buf)))

    def approach(self, first):
        for i in range(PARK, first):
            rc, num, p = self.add(self.W[i:i + 1])
            assert (rc, num) == (0, i) and self.lib.decoder_add_original(self.dec, C.byref(p)) == 0
        assert self.lib.encoder_remove_before(self.enc, first) == 0

    def ack(self, limit=ACK_LIMIT):
        buf, used = C.create_string_buffer(limit), C.c_uint()
        rc = self.lib.decoder_ack(self.dec, buf, limit, C.byref(used))
        return rc, buf.raw[:used.value]

    def acknowledge(self, msg):
        nxt = C.c_uint()
        buf = (C.c_ubyte * max(1, len(msg))).from_buffer_copy(msg or b"\0")
        rc = self.lib.encoder_ack(self.enc, C.cast(buf, C.c_void_p), len(msg), C.byref(nxt))
        return rc, nxt.value

    def encode(self):
        rp = RecoveryPacket()
        assert self.lib.encode(self.enc, C.byref(rp)) == 0
        data = C.string_at(rp.Data, rp.DataBytes)
        assert self.lib.decoder_add_recovery(self.dec, C.byref(rp)) == 0
        return data

    def decode(self):
        pk, n = C.POINTER(OriginalPacket)(), C.c_uint()
        rc = self.lib.decode(self.dec, C.byref(pk), C.byref(n))
        return rc, [(pk[k].PacketNum, C.string_at(pk[k].Data, pk[k].DataBytes)) for k in range(n.value)] if rc == 0 else []


def describe_decode(rc, packets):
    return [rc, [[num, len(d), hashlib.sha256(d).hexdigest()] for num, d in packets]]


def reference_case(ref, name):
    """A case's schedule through the reference's siamese.h calls (on a pair
    nothing else uses afterwards): what wrap_edges.json records of it."""
    case = CASES[name]
    data = payloads(case)
    ref.approach(case.first)
    longest = longest_symbol(case.lengths)
    out = {"spec_sha256": case.spec_sha256(), "first": case.first, "recovery": [], "decodes": []}
    added, group = 0, 0
    for s in case.schedule:
        if s[0] == "add":
            for i in range(added, added + s[1]):
                rc, num, _ = ref.add(data[i])
                assert (rc, num) == (0, case.num(i)), "the reference numbered original %d as %d" % (i, num)
                if i not in case.lost:
                    assert ref.recv(num, data[i]) == 0
            added += s[1]
        elif s[0] == "encode":
            for _ in range(s[1]):
                # (every window holds its longest original: the packet is the longest symbol and its footer)
                out["recovery"].append(describe_packet(ref.encode(), longest))
        elif s[0] == "remove_before":
            assert ref.lib.encoder_remove_before(ref.enc, case.num(s[1])) == 0
        else:
            want, got, calls = len(case.groups[group]), [], 0
            group += 1
            while len(got) < want and calls < 8:
                rc, packets = ref.decode()
                out["decodes"].append(describe_decode(rc, packets))
                calls += 1
                if rc != 0 or not packets:
                    break
                got += packets
            back = sorted(got)
            if back != [(case.num(i), data[i]) for i in sorted(case.groups[group - 1], key=case.num)]:
                raise SystemExit("%s: the reference does not decode loss set %d; pick another" % (name, group))
    return out


def reference_arq(ref):
    data, lost = arq_stream()
    first = PERIOD - ARQ_BEFORE
    ref.approach(first)
    out = {"acks": [], "retransmits": []}
    for i, d in enumerate(data):
        rc, num, _ = ref.add(d)
        assert (rc, num) == (0, (first + i) & MASK)
        if not lost[i]:
            assert ref.recv(num, d) == 0
        if i % 4 == 3:
            rc, msg = ref.ack(ARQ_LIMIT)
            out["acks"].append([rc, msg.hex()] + list(ref.acknowledge(msg)))
    time.sleep(ARQ_SLEEP)
    for _ in range(len(data) + 1):
        p = OriginalPacket()
        rc = ref.lib.encoder_retransmit(ref.enc, C.byref(p))
        if rc != 0:
            out["retransmits"].append([rc, 0, 0])
            break
        out["retransmits"].append([rc, p.PacketNum, p.DataBytes])
    return out


def check_dropin(path, name):
    """A case through the drop-in siamese.h calls of the library at `path`, by
    the code that records the reference's: the walk's hash and the case's
    entry of wrap_edges.json must come out."""
    t0 = time.time()
    pair = ApiPair(path)
    t1 = time.time()
    want = golden()
    assert (pair.packets, pair.sha256) == (want["walk"]["packets"], want["walk"]["sha256"]), \
        "the drop-in walk's recovery packets or acks differ from the reference's before the wrap is reached"
    got = reference_case(pair, name)
    print("wrap: drop-in walk %.2f s, %s %.2f s" % (t1 - t0, name, time.time() - t1))
    assert got == want["cases"][name], "%s through the drop-in API differs from the reference's record" % name


def check_dropin_in_child(path, name, seconds=110):
    """check_dropin in a process of its own (the drop-in calls and the batch
    ABI each initialise the library), under a time limit."""
    code = "import sys; sys.path[:0] = [%r, %r]; import wrap_cases as W\nW.check_dropin(%r, %r)\nprint('ok')" % (
        os.path.dirname(os.path.abspath(__file__)), S.ROOT, path, name)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=seconds, cwd=S.ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    print(out.stdout)


# ---- the library's side ------------------------------------------------------
def load(path):
    L = ST.load(path)
    A.load(path)
    R.load(path)
    X.bind(L)
    L.sgpu_decoder_get_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_has.argtypes = [C.c_void_p, C.c_uint]
    return L


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
        assert (_golden["walk"]["park"], _golden["walk"]["step"]) == (PARK, STEP), \
            "wrap_edges.json was made for another walk: run tests/golden/make_wrap_golden.py"
    return _golden


class Parked:
    """len(names) pairs walked to PARK in lock-step, one flush per step."""

    def __init__(self, path, names):
        L = self.L = load(path)
        t0 = time.time()
        self.W = walk_bytes()
        self.src = L.sgpu_device_alloc(PERIOD)
        assert self.src and L.sgpu_h2d(self.src, self.W, PERIOD) == 0
        n = len(names)
        pairs = [(L.sgpu_encoder_create(), L.sgpu_decoder_create()) for _ in range(n)]
        assert all(e and d for e, d in pairs)
        recs = (D.Rec * n)()
        hashes = [hashlib.sha256() for _ in range(n)]
        first, added, calls, used, nxt = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
        ackBuf = C.create_string_buffer(ACK_LIMIT)
        self.packets = 0
        for a, cnt in steps():
            acks = []
            for k, (e, d) in enumerate(pairs):
                r = L.sgpu_encoder_add_range(e, self.src + a, 1, None, 1, cnt, C.byref(first), C.byref(added))
                assert (r, first.value, added.value) == (D.SUCCESS, a, cnt), \
                    "pair %d: range add at %d returned %d, first %d, added %d" % (k, a, r, first.value, added.value)
                r = L.sgpu_decoder_add_original_range(d, a, self.src + a, 1, None, 1, cnt, None, C.byref(calls))
                assert (r, calls.value) == (D.SUCCESS, cnt), "pair %d: the decoder took %d of %d originals at %d: %d" % (
                    k, calls.value, cnt, a, r)
                assert L.sgpu_encoder_remove_before(e, a) == D.SUCCESS
                assert L.sgpu_encode(e, C.byref(recs[k])) == D.SUCCESS
                assert L.sgpu_decoder_add_recovery(d, C.byref(recs[k])) == D.SUCCESS
                # the encoder's ack state follows the stream (it takes acks within 2^21 packets of it only)
                assert L.sgpu_decoder_ack(d, ackBuf, ACK_LIMIT, C.byref(used)) == D.SUCCESS
                acks.append(ackBuf.raw[:used.value])
                r = L.sgpu_encoder_acknowledge(e, acks[-1], used.value, C.byref(nxt))
                assert (r, nxt.value) == (D.SUCCESS, a + cnt), "pair %d: the ack at %d: %d, next expected %d" % (
                    k, a, r, nxt.value)
            assert L.sgpu_flush() == 0
            srcs = (C.c_void_p * n)(*[recs[k].DeviceData for k in range(n)])
            lens = (C.c_uint * n)(*[recs[k].DataBytes for k in range(n)])
            buf = (C.c_ubyte * sum(lens))()
            assert L.sgpu_gather(n, srcs, lens, buf) == 0
            raw, at = bytes(buf), 0
            for k in range(n):
                walk_update(hashes[k], raw[at:at + lens[k]], recs[k].FooterBytes)
                hashes[k].update(acks[k])
                at += lens[k]
            self.packets += 1
        self.seconds = time.time() - t0
        print("wrap: walked %d pairs to %#x in %d steps, %.2f s" % (n, PARK, self.packets, self.seconds))
        want = golden()["walk"]
        assert self.packets == want["packets"]
        for k, h in enumerate(hashes):
            assert h.hexdigest() == want["sha256"], "pair %d (%s): the walk's recovery packets differ from the " \
                "reference's before the wrap is reached" % (k, names[k])
        self.pairs = dict(zip(names, pairs))
        self.taken = 0

    def release(self):
        """Free the pairs no case took, and the walk's source."""
        for e, d in self.pairs.values():
            self.L.sgpu_encoder_free(e)
            self.L.sgpu_decoder_free(d)
        self.pairs = {}
        assert self.L.sgpu_flush() == 0
        self.L.sgpu_device_free(self.src)

    def take(self, name, first):
        """The pair parked for `name`, brought to `first` with an empty encoder window."""
        L = self.L
        e, d = self.pairs.pop(name)
        self.taken += 1
        n = first - PARK
        a, added, calls = C.c_uint(), C.c_uint(), C.c_uint()
        if n:
            assert L.sgpu_encoder_add_range(e, self.src + PARK, 1, None, 1, n, C.byref(a), C.byref(added)) == D.SUCCESS
            assert (a.value, added.value) == (PARK, n)
            assert L.sgpu_decoder_add_original_range(d, PARK, self.src + PARK, 1, None, 1, n, None,
                                                     C.byref(calls)) == D.SUCCESS and calls.value == n
        assert L.sgpu_encoder_remove_before(e, first) == D.SUCCESS
        return e, d


_parked = {}


def parked(path, name, names=None):
    """The walk that holds a pair for `name`: the module's, made once for all
    of `names` at once (default: every case); when that one's pair has been
    taken (a test run again in one process), a walk of one pair."""
    if path not in _parked:
        _parked[path] = Parked(path, list(names or ALL))
    elif name not in _parked[path].pairs:
        release(path)
        _parked[path] = Parked(path, [name])
    return _parked[path]


def release(path):
    pk = _parked.pop(path, None)
    if pk:
        pk.release()


class Source:
    """Payloads in device memory at odd addresses (deliver_cases.Stream's layout)."""

    def __init__(self, L, data, fixed=0):
        self.L, self.fixed = L, fixed
        self.pitch = ((max(len(d) for d in data) + 34) & ~15) + 2
        blob = bytearray(3 + self.pitch * len(data))
        for i, d in enumerate(data):
            blob[3 + i * self.pitch:3 + i * self.pitch + len(d)] = d
        self.src = L.sgpu_device_alloc(len(blob))
        assert self.src and L.sgpu_h2d(self.src, bytes(blob), len(blob)) == 0
        self.lens = (C.c_uint * len(data))(*[len(d) for d in data])

    def at(self, i):
        return self.src + 3 + i * self.pitch

    def add(self, L, enc, i, n, want):
        first, added = C.c_uint(0x7fffffff), C.c_uint(0)
        r = L.sgpu_encoder_add_range(enc, self.at(i), self.pitch, None if self.fixed else C.byref(self.lens, 4 * i),
                                     self.fixed, n, C.byref(first), C.byref(added))
        assert (r, first.value, added.value) == (D.SUCCESS, want, n), \
            "range add of %d originals: result %d, first packet %#x (expected %#x), %d added" % (
                n, r, first.value, want, added.value)

    def recv(self, L, dec, i, j, num):
        """Originals [i, j) as packets num.. by one call."""
        res = (C.c_int * (j - i))(*([-1] * (j - i)))
        calls = C.c_uint(0)
        r = L.sgpu_decoder_add_original_range(dec, num, self.at(i), self.pitch,
                                              None if self.fixed else C.byref(self.lens, 4 * i), self.fixed, j - i,
                                              res, C.byref(calls))
        assert r == D.SUCCESS and calls.value == j - i and list(res) == [D.SUCCESS] * (j - i), \
            "range of %d originals from packet %#x: result %d, %d calls, %r" % (j - i, num, r, calls.value, list(res))

    def free(self):
        self.L.sgpu_device_free(self.src)


def stretches(lo, hi, lost):
    i = lo
    while i < hi:
        j = i
        while j < hi and j not in lost:
            j += 1
        if j > i:
            yield i, j
        i = j + 1


def decode_call(L, dec, device):
    """One decode with its packets read after a flush: (result, [(num, bytes)], matrix jobs)."""
    out, n = C.POINTER(OriginalPacket)(), C.c_uint(0)
    f = L.sgpu_decode_device if device else L.sgpu_decode
    r, jobs = f(dec, C.byref(out), C.byref(n)), 0
    if r == D.PENDING:
        jobs = 1
        assert L.sgpu_flush() == 0
        r = f(dec, C.byref(out), C.byref(n))
    if r != D.SUCCESS:
        return r, [], jobs
    assert L.sgpu_flush() == 0
    return r, [(out[k].PacketNum, D.read(L, C.cast(out[k].Data, C.c_void_p).value, out[k].DataBytes))
               for k in range(n.value)], jobs


def check(name, path, names=None):
    case = CASES[name]
    pk = parked(path, name, names)
    L = pk.L
    want = golden()["cases"][name]
    assert want["spec_sha256"] == case.spec_sha256(), "wrap_edges.json was made for another %s: run " \
        "tests/golden/make_wrap_golden.py" % name
    data = payloads(case)
    enc, dec = pk.take(name, case.first)
    t0 = time.time()
    e0 = Z.engine(L)
    src = Source(L, data, case.fixed)
    recRows = D.Rows(L, case.recovery, (LONG + 3 + 8 + 15) & ~15)
    recs = (D.Rec * case.recovery)()
    added = made = group = solves = jobs = 0
    decodes = []
    for s in case.schedule:
        if s[0] == "add":
            src.add(L, enc, added, s[1], case.num(added))
            for i, j in stretches(added, added + s[1], case.lost):
                src.recv(L, dec, i, j, case.num(i))
            added += s[1]
        elif s[0] == "encode":
            for _ in range(s[1]):
                r = recs[made]
                assert L.sgpu_encode(enc, C.byref(r)) == D.SUCCESS
                assert F.recovery(L, C.byref(r), 1, None, recRows, dst=recRows.dst + made * recRows.stride,
                                  lens=recRows.lens + 4 * made) == 1
                assert L.sgpu_decoder_add_recovery(dec, C.byref(r)) == D.SUCCESS
                made += 1
        elif s[0] == "remove_before":
            assert L.sgpu_encoder_remove_before(enc, case.num(s[1])) == D.SUCCESS
        else:
            assert L.sgpu_flush() == 0
            lostNow, got, calls = case.groups[group], [], 0
            group += 1
            while len(got) < len(lostNow) and calls < 8:
                r, packets, j = decode_call(L, dec, case.device)
                decodes.append(describe_decode(r, packets))
                calls += 1
                jobs += j
                if r != D.SUCCESS or not packets:
                    break
                solves += 1
                got += packets
            assert sorted(got) == [(case.num(i), data[i]) for i in sorted(lostNow, key=case.num)], \
                "decode %d: packets %r came back, lost were %r" % (group, sorted(g[0] for g in got),
                                                                  sorted(case.num(i) for i in lostNow))
    assert L.sgpu_flush() == 0

    # 1. the recovery packets are the reference's
    rows, lens = recRows.fetch()
    assert len(want["recovery"]) == case.recovery
    for k, w in enumerate(want["recovery"]):
        r = recs[k]
        assert (r.DataBytes, r.FooterBytes) == (w["bytes"], w["footer_bytes"]), \
            "recovery packet %d: %d bytes with a %d-byte footer, the reference's has %d with %d" % (
                k, r.DataBytes, r.FooterBytes, w["bytes"], w["footer_bytes"])
        assert lens[k] == r.DataBytes and rows[k][r.DataBytes:] == bytes(recRows.stride - r.DataBytes)
        assert rows[k][r.DataBytes - r.FooterBytes:r.DataBytes] == bytes(r.Footer[:r.FooterBytes]), \
            "recovery packet %d: the footer in device memory is not the host's copy" % k
        assert hashlib.sha256(rows[k][:r.DataBytes]).hexdigest() == w["sha256"], \
            "recovery packet %d (%d bytes) differs from the reference's" % (k, r.DataBytes)

    # 2. the decodes: results, packet numbers, lengths and bytes in the reference's order
    assert decodes == want["decodes"], "the decode calls returned %r, the reference's %r" % (
        [(d[0], [p[:2] for p in d[1]]) for d in decodes], [(d[0], [p[:2] for p in d[1]]) for d in want["decodes"]])

    # 3. the live window across the wrap into guarded rows
    count, kept = len(case.lengths), case.kept_from()
    out = D.Rows(L, count - kept, (LONG + 16) & ~15)
    res, queued = D.deliver(L, dec, case.num(kept), count - kept, out)
    assert res == [D.SUCCESS] * (count - kept) and queued == count - kept, "an original of the live window is missing"
    assert L.sgpu_flush() == 0
    e2 = Z.engine(L)
    got, lens = out.fetch()
    for k in range(kept, count):
        D.check_row(got[k - kept], lens[k - kept], data[k], "packet %#x (%d bytes%s)" % (
            case.num(k), len(data[k]), ", recovered" if k in case.lost else ""))
        assert L.sgpu_decoder_has(dec, case.num(k)) == D.SUCCESS
    out.free()
    recRows.free()
    L.sgpu_encoder_free(enc)
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    src.free()

    # 4. the path
    def grew(key):
        return e2[key] - e0[key]
    # (a loss set may take two calls, as the reference's does: the calls were compared above)
    assert grew("solves") == solves >= len(case.groups), "%d solves for %d decode calls" % (grew("solves"), solves)
    assert (grew("ldpc_bytes") > 0) == case.wide, "k_ldpc took %d bytes of picks" % grew("ldpc_bytes")
    assert grew("ge_jobs") == jobs and (jobs >= 1) == case.device, "%d matrix jobs" % jobs
    assert grew("ge_chained") == jobs, "%d of %d square jobs chained into their decode's submission" % (
        grew("ge_chained"), jobs)
    print("wrap: %s after the walk %.2f s, %d of %d matrix jobs chained" % (name, time.time() - t0, grew("ge_chained"),
                                                                         jobs))


def check_in_child(names, path, env, seconds=110):
    """check() of `names` in a fresh process with `env` added to the
    environment (knobs the library reads once per process): its own walk, of
    the pairs it needs alone.  seconds: the child's limit, below the 120 s of
    test_wrap_gpu.py's own, so that a child never outlives its parent."""
    code = "import sys; sys.path[:0] = [%r, %r]; import wrap_cases as W\nfor n in %r: W.check(n, %r, %r)\nW.release(%r)\nprint('ok')" % (
        os.path.dirname(os.path.abspath(__file__)), S.ROOT, list(names), path, list(names), path)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=seconds, cwd=S.ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    print(out.stdout)


# ---- 6. range calls that cross the wrap inside one call ----------------------
RANGE_SEED, RANGE_BEFORE, RANGE_COUNT, RANGE_LOST = 7, 40, 96, (5, 90)


def py_header(flow, num, n):
    """An original's frame header (siamese_gpu.h, "Framed datagrams")."""
    length = 7 + n
    return P.prefix(length, 1 if length < 128 else 2) + bytes([F.ORIGINAL]) + flow.to_bytes(3, "little") + \
        num.to_bytes(3, "little")


def check_ranges(path, names=None):
    pk = parked(path, RANGES, names)
    L = pk.L
    first = PERIOD - RANGE_BEFORE
    count, lost = RANGE_COUNT, RANGE_LOST
    lengths = X.lengths(count, 3, RANGE_SEED)
    data = [hashlib.shake_256(b"wrap:%d:%d" % (RANGE_SEED, i)).digest(n) for i, n in enumerate(lengths)]
    num = lambda i: (first + i) & MASK
    enc, dec = pk.take(RANGES, first)
    src = Source(L, data)
    # sgpu_encoder_add_range, sgpu_decoder_add_original_range: 6..89 crosses the wrap in one call
    src.add(L, enc, 0, count, first)
    for i, j in stretches(0, count, lost):
        src.recv(L, dec, i, j, num(i))
    lo, hi = lost[0] + 1, lost[1]
    assert lo < RANGE_BEFORE < hi
    present = data[lo:hi]
    frames = [py_header(FLOW, num(k), len(d)) + d for k, d in enumerate(data)]
    for k, d in enumerate(data):
        assert R.framed(L, FLOW, num(k), d) == frames[k], "sgpu_frame_write_header for packet %#x" % num(k)
    for k, want in ((RANGE_BEFORE - 1, b"\xff\xff\x3f"), (RANGE_BEFORE, bytes(3))):
        assert frames[k][len(frames[k]) - len(data[k]) - 3:len(frames[k]) - len(data[k])] == want
    # sgpu_decoder_has
    for k in range(count):
        assert L.sgpu_decoder_has(dec, num(k)) == (D.NEED_MORE if k in lost else D.SUCCESS), "has(%#x)" % num(k)
    assert L.sgpu_decoder_has(dec, num(count)) == D.NEED_MORE
    # every delivery queued in one submission
    bare, framed = D.Rows(L, count, 608), D.Rows(L, count, 624)
    res, queued = D.deliver(L, dec, first, count, bare)
    absent = [D.NEED_MORE if k in lost else D.SUCCESS for k in range(count)]
    assert res == absent and queued == count - 2
    res, queued = R.relay(L, dec, FLOW, first, count, framed)
    assert res == absent and queued == count - 2
    stride = 1424
    _, need = RP.layout([len(f) for f in frames[lo:hi]], stride)
    packed, info = D.Rows(L, need + 1, stride), RP.Info(L)
    res, queued = RP.pack(L, dec, FLOW, num(lo), hi - lo, packed, need + 1, info)
    assert res == [D.SUCCESS] * (hi - lo) and queued == hi - lo
    call = ST.Call(L, dec, num(lo), present, 3, what="deliver_stream across the wrap")
    sent = D.Rows(L, count, 624)
    res, queued = F.originals(L, enc, first, count, FLOW, sent)
    assert res == [D.SUCCESS] * count and queued == count
    _, eneed = RP.layout([len(f) for f in frames], stride)
    epacked = D.Rows(L, eneed + 1, stride)
    res, nrows, nframes = P.pack(L, enc, FLOW, first, count, None, 0, epacked, eneed + 1)
    assert res == [D.SUCCESS] * count and (nrows, nframes) == (eneed, count)
    assert L.sgpu_flush() == 0
    # sgpu_decoder_get_range
    got = (OriginalPacket * count)()
    n = C.c_uint(0)
    assert L.sgpu_decoder_get_range(dec, num(lo), hi - lo, got, C.byref(n)) == D.SUCCESS and n.value == hi - lo
    for k in range(hi - lo):
        assert (got[k].PacketNum, got[k].DataBytes) == (num(lo + k), len(present[k])), "get_range's packet %d" % k
        assert D.read(L, C.cast(got[k].Data, C.c_void_p).value, got[k].DataBytes) == present[k]
    assert L.sgpu_decoder_get_range(dec, first, count, got, C.byref(n)) == D.NEED_MORE and n.value == lost[0]
    # sgpu_decoder_deliver_range, sgpu_decoder_deliver_frames, sgpu_encoder_deliver_range
    rows, lens = bare.fetch()
    frows, flens = framed.fetch()
    srows, slens = sent.fetch()
    for k in range(count):
        what = "packet %#x" % num(k)
        F.check_row(srows[k], slens[k], frames[k], what + " from the encoder")
        if k in lost:
            assert lens[k] == flens[k] == 0 and rows[k] == bytes([D.FILL]) * 608 and frows[k] == bytes([D.FILL]) * 624
        else:
            D.check_row(rows[k], lens[k], data[k], what)
            F.check_row(frows[k], flens[k], frames[k], what + " framed")
    # sgpu_decoder_pack_frames, sgpu_decoder_deliver_stream, sgpu_encoder_pack_frames
    RP.check(packed, info, frames[lo:hi], need + 1, what="decoder_pack_frames across the wrap")
    call.check()
    wantRows, wantLens, _ = RP.expect(frames, stride, eneed + 1)
    erows, elens = epacked.fetch()
    assert elens == wantLens and erows[:eneed] == wantRows, "encoder_pack_frames across the wrap"
    r, fr = P.parse(L, b"".join(erows[:eneed]))
    assert r == D.SUCCESS and [f.PacketNum for f in fr] == [num(k) for k in range(count)]
    for x in (bare, framed, packed, info, sent, epacked):
        x.free()
    L.sgpu_encoder_free(enc)
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    src.free()


# ---- 7. ARQ across the wrap --------------------------------------------------
ARQ_SEED, ARQ_BEFORE, ARQ_LIMIT, ARQ_SINGLES = 9, 20, 64, 3
# the sleep of arq_cases.check_parity, past the initial RTO of 500 ms: the RTO after the walk's acks
# is 1.5 times the longest round trip they measured (arq.cpp update_rto), which nobody measured here
ARQ_SLEEP = A.RTO_SLEEP


def arq_stream():
    data, lost = A.stream(ARQ_SEED)
    lost[ARQ_BEFORE - 1] = lost[ARQ_BEFORE] = True      # 0x3fffff and 0
    lost[ARQ_BEFORE - 2] = lost[ARQ_BEFORE + 1] = False
    assert any(lost[:ARQ_BEFORE - 2]) and any(lost[ARQ_BEFORE + 2:])
    return data, lost


def check_arq(path, names=None):
    """arq_cases.check_parity's call sequence with packet 0 in the middle of the
    stream, against the reference's recorded messages, results, nextExpected
    and retransmission order."""
    pk = parked(path, ARQ, names)
    L = pk.L
    want = golden()["arq"]
    data, lost = arq_stream()
    first = PERIOD - ARQ_BEFORE
    num = lambda i: (first + i) & MASK
    p = A.Pair(L, data)
    L.sgpu_encoder_free(p.enc)
    L.sgpu_decoder_free(p.dec)
    p.enc, p.dec = pk.take(ARQ, first)
    acks = []
    for i in range(len(data)):
        assert p.add(i) == (D.SUCCESS, num(i))
        if not lost[i]:
            assert L.sgpu_decoder_add_original(p.dec, num(i), p.src + i * p.pitch, len(data[i])) == D.SUCCESS
        if i % 4 == 3:
            r, used, msg = p.ack(ARQ_LIMIT)
            assert used == len(msg)
            acks.append([r, msg.hex()] + list(p.acknowledge(msg)))
            assert acks[-1] == want["acks"][len(acks) - 1], "ack after %d adds: %r, the reference's %r" % (
                i + 1, acks[-1], want["acks"][len(acks) - 1])
    assert acks == want["acks"]
    assert L.sgpu_flush() == 0
    time.sleep(ARQ_SLEEP)
    order = [w for w in want["retransmits"] if w[0] == D.SUCCESS]
    # what the reference sends again: every lost packet, on both sides of the wrap, in stream order
    assert [w[1] for w in order if (w[1] - first) & MASK < len(data) and lost[(w[1] - first) & MASK]] == \
        [num(i) for i in range(len(data)) if lost[i]], "wrap_edges.json: the reference's retransmissions"
    assert len(order) > ARQ_SINGLES
    # (every retransmit call before anything slow: a packet sent again is due again an RTO, 20 ms, later)
    stride, maxRows = 1424, len(order)
    rows = D.Rows(L, maxRows, stride)
    singles = [p.retransmit() for _ in order[:ARQ_SINGLES]]
    r, nums, used = A.retransmit_frames(L, p.enc, FLOW, 99, rows, maxRows)
    last, _ = p.retransmit()
    for (rs, q), w in zip(singles, order):
        assert [rs, q.PacketNum, q.DataBytes] == w, "retransmitted %r, the reference %r" % (
            [rs, q.PacketNum, q.DataBytes], w)
        assert D.read(L, q.Data, q.DataBytes) == data[(q.PacketNum - first) & MASK]
    assert r == D.SUCCESS and nums == [w[1] for w in order[ARQ_SINGLES:]], "retransmit_frames sent %r, the " \
        "reference's order is %r" % (nums, [w[1] for w in order[ARQ_SINGLES:]])
    assert last == D.NEED_MORE == want["retransmits"][-1][0]
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    fr = [py_header(FLOW, n, len(data[(n - first) & MASK])) + data[(n - first) & MASK] for n in nums]
    wantRows, wantLens = A.rows_of(fr, stride, maxRows)
    assert used == len(wantRows) and lens == wantLens and got[:used] == wantRows
    rows.free()
    p.free()
