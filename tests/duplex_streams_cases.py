"""sgpu_frames_scan_duplex_streams / sgpu_frames_recv_duplex_streams: the cases
shared by test_duplex_streams_cpu.py (the CPU test double, tests/hostsim) and
test_duplex_streams_gpu.py (k_ackstreamwalk, k_rowsum2, k_compact and k_slots on
the MI355X), driven through the C ABI with ctypes.

The yardstick is existing code, never the code under test.  The first part of
every expected output is what sgpu_frames_scan_duplex_dense writes for a copy of
the rows with [0, start) zeroed and, for a row that ends in a partial frame,
[next, end) zeroed too, with the rows' ends as its length words
(test_duplex_dense_* pin that scan to sgpu_frames_scan_duplex).  The next words
and the SGPU_STREAM_PARTIAL_DUPLEX bits are worked out here from the frame lists
a case laid out (Row.expect), never from the bytes, and the rest of the case's
word is checked against the reference's.  A row with start > end or end > stride
has no such copy: the contract gives it the word and the records of a row whose
length word exceeds the stride, which is what the copy's length word is set to.
The whole pinned buffer is compared byte for byte between two guard records
pre-filled with 0xA5.

Stale ring content: every layout is scanned with the bytes before start and
from end on zero, and again with them filled with junk of three kinds; the
expectation is the same buffer, so the outputs are identical.

The rows of a workgroup come from the kernel's constant in
siamese_amd/csrc/ops.h (kAckStreamWalkThreads).
"""
import ctypes as C
import os
import random
import re
import struct

import dense_cases as DN
import duplex_dense_cases as DD
import pack_cases as P
import scan_cases as K
import streams_cases as ST
from arq_cases import ACK, Pair, ack_frame
from deliver_cases import FILL, INVALID, NEED_MORE, SUCCESS, payload
from frame_cases import ORIGINAL, RECOVERY, Sender
from pack_cases import REC, frame, prefix
from siamese_amd.binding import (PACKED_ACKS_DROPPED, PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, ROW_TRUNCATED,
                                 STREAM_PARTIAL, STREAM_PARTIAL_DUPLEX, PackedHead, bind_duplex_streams_abi)
from streams_cases import DevStreams, original, recovery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_DUPLEX_STREAMS, NSTATS = 43, 44
TIMING_ACKWALK, TIMING_COMPACT, TIMING_ROWSUM2, TIMING_SLOTS, TIMING_STREAMWALK, TIMING_ACKSTREAMWALK, NTIMING = \
    12, 16, 17, 18, 19, 20, 21
PART, BAD, MORE, DROPPED = STREAM_PARTIAL_DUPLEX, PACKED_MALFORMED, PACKED_MORE, PACKED_ACKS_DROPPED
assert PART == 0x10000000 and STREAM_PARTIAL == DROPPED == 0x20000000


def kernel_constants():
    with open(os.path.join(ROOT, "siamese_amd", "csrc", "ops.h")) as f:
        src = f.read()

    def value(name):
        m = re.search(r"constexpr uint32_t %s = (\d+|0x[0-9a-fA-F]+)u?;" % name, src)
        assert m, "%s not found in ops.h" % name
        return int(m.group(1), 0)

    return dict(walk=value("kAckStreamWalkThreads"), partial=value("kStreamPartialDuplex"))


KC = kernel_constants()
assert KC["partial"] == PART
ROW_COUNTS = [1, 63, 64, 65, KC["walk"] - 1, KC["walk"] + 1]


def load(path):
    L = DD.load(path)
    ST.load(path)
    if getattr(L, "_duplex_streams_cases", False):
        return L
    # (the four symbols under test: an AttributeError here is the parent's answer)
    bind_duplex_streams_abi(L)
    L._duplex_streams_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


# ---------------------------------------------------------------------------
# rows as lists of frames

class Row(ST.Row):
    """streams_cases.Row with acknowledgement frames: ack() remembers the message
    length of the frame it adds, and expect() follows the duplex walk."""

    def __init__(self, stride):
        ST.Row.__init__(self, stride)
        self.ackAt = {}

    def ack(self, flow, msg, width=1):
        return self.add(ack_frame(flow, msg, width))

    def add(self, data, good=True, never=None, total=None):
        w = 1 + (data[0] >= 0x80) + (data[0] >= 0xC0) + (data[0] >= 0xE0)
        if good and never is None and total is None and len(data) > w + 4 and data[w] == ACK:
            self.ackAt[len(self.buf)] = len(data) - w - 4   # (a whole ack frame: its message's length)
        return ST.Row.add(self, data, good, never, total)

    def expect(self, start, end, m, s=1, ab=16):
        """(row word, next) of a walk of [start, end); start lies at a frame's
        first byte or in a zero gap."""
        if start > end or end > self.stride:
            return BAD, min(start, self.stride)
        n = a = flags = 0
        for off, have, total, good, never in self.parts:
            if off + have <= start:
                continue
            assert off >= start, "the case's start %d lies inside the frame at %d" % (start, off)
            if off >= end:
                break
            if n == m:
                return n | flags | MORE, off
            if off + total > end:
                left = end - off
                return n | flags | (BAD if never is not None and left >= never else PART), off
            assert have == total
            if not good:
                return n | flags | BAD, off
            if off in self.ackAt:
                if a >= s or self.ackAt[off] > ab:
                    flags |= DROPPED
                a += 1
            n += 1
        return n | flags, end


def junked(row, start, end, kind):
    """The row with its stale bytes -- [0, start) and [end, stride) -- filled."""
    stride = len(row)
    if kind == 0 or start > end or end > stride:
        return row
    if kind == 1:     # valid-looking frames, the first right behind end
        unit = original(77, 12) + ack_frame(1, b"stale")
    elif kind == 2:   # the byte 3: where a cut-off frame's type byte would be, a type that is never valid
        unit = b"\x03"
    else:
        unit = b"\xff"
    fill = unit * (stride // len(unit) + 1)
    b = bytearray(row)
    b[end:] = fill[:stride - end]
    b[:start] = fill[len(fill) - start:] if start else b""
    return bytes(b)


# ---------------------------------------------------------------------------
# one scan against the dense duplex scan of the zeroed copy

class Out:
    """A duplex stream scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxRecords, maxAcks, ab):
        self.L = L
        self.total = L.sgpu_frames_duplex_streams_bytes(count, maxRecords, maxAcks, ab)
        self.next = L.sgpu_frames_duplex_streams_next(count, maxRecords, maxAcks, ab)
        assert self.next == L.sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ab) == \
            DD.slots_offset(count, maxRecords) + maxAcks * ab
        assert self.total == self.next + ((4 * count + 15) & ~15)
        self.bytes = self.total + 2 * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the output was written"
        assert raw[-REC:] == guard, "guard record after the next words was written"
        return raw[REC:-REC]

    def untouched(self):
        return C.string_at(self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_host_free(self.base)


def zeroed_copy(rowBytes, stride, starts, ends, expect):
    rows, lens = [], []
    for k, row in enumerate(rowBytes):
        s, e = starts[k], ends[k]
        word, nxt = expect[k]
        if s > e or e > stride:
            rows.append(row)
            lens.append(stride + 16)
            continue
        b = bytearray(row)
        b[:s] = bytes(s)
        if word is not None and word & PART:
            b[nxt:e] = bytes(e - nxt)
        rows.append(bytes(b))
        lens.append(e)
    return rows, lens


def expected_output(L, rowBytes, stride, starts, ends, expect, m, s, ab, maxRecords, maxAcks):
    """The bytes the contract asks for, the reference copy's DevRows (the caller
    frees it) and the reference dense bytes.  An expectation whose word is None
    takes the reference's word (rows without a partial frame)."""
    count = len(rowBytes)
    rows, lens = zeroed_copy(rowBytes, stride, starts, ends, expect)
    ref = K.DevRows(L, rows, stride, lens)
    dense, o = DD.scan(L, ref.dev, stride, ref.lens, count, m, s, ab, maxRecords, maxAcks)
    o.free()
    b = bytearray(dense)
    for k in range(count):
        word, = struct.unpack_from("<I", b, 16 + 4 * k)
        want = expect[k][0]
        if want is None:
            continue
        assert word == want & ~PART, "row %d: the case expects word %#x, the dense duplex scan of the copy gives %#x" \
            % (k, want, word)
        struct.pack_into("<I", b, 16 + 4 * k, want)
    nxt = struct.pack("<%dI" % count, *[e[1] for e in expect])
    return bytes(b) + nxt + bytes(-len(nxt) % 16), ref, dense


def first_difference(got, want, count, maxRecords, maxAcks, ab):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    nextAt = DD.slots_offset(count, maxRecords) + maxAcks * ab
    if at >= nextAt:
        return "first difference at byte %d (next words, row %d): %r, expected %r" % (
            at, (at - nextAt) // 4, got[at:at + 8], want[at:at + 8])
    if 16 <= at < 16 + 4 * count:
        k = (at - 16) // 4
        return "row word %d: %#x, expected %#x" % (k, struct.unpack_from("<I", got, 16 + 4 * k)[0],
                                                   struct.unpack_from("<I", want, 16 + 4 * k)[0])
    return DD.first_difference(got, want, count, maxRecords)


def scan(L, ds, starts, ends, m, s, ab, maxRecords, maxAcks):
    """(the output's bytes, Out) of one duplex stream scan; starts / ends: device arrays or None."""
    o = Out(L, ds.count, maxRecords, maxAcks, ab)
    t = L.sgpu_frames_scan_duplex_streams(ds.dev, ds.stride, starts, ends, ds.count, m, s, ab, maxRecords, maxAcks,
                                          o.out)
    assert t > 0, "sgpu_frames_scan_duplex_streams returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return o.fetch(), o


def check_raw(L, rowBytes, stride, m, s, ab, starts, ends, expect, maxRecords=None, maxAcks=None, junk=(0,)):
    """One duplex stream scan per junk fill of the rows against the expectation;
    starts / ends: lists, or None for a null array (no junk then on that side).
    Returns the output's bytes."""
    count = len(rowBytes)
    st = starts if starts is not None else [0] * count
    en = ends if ends is not None else [stride] * count
    maxRecords = count * m if maxRecords is None else maxRecords
    maxAcks = count * s if maxAcks is None else maxAcks
    want, ref, _ = expected_output(L, rowBytes, stride, st, en, expect, m, s, ab, maxRecords, maxAcks)
    ref.free()
    got = None
    for kind in junk:
        ds = DevStreams(L, [junked(rowBytes[k], st[k], en[k], kind) for k in range(count)], stride)
        if starts is not None:
            ds.put(ds.starts, starts)
        if ends is not None:
            ds.put(ds.ends, ends)
        got, o = scan(L, ds, ds.starts if starts is not None else None, ds.ends if ends is not None else None, m, s,
                      ab, maxRecords, maxAcks)
        o.free()
        ds.free()
        assert got == want, "count %d, maxFrames %d, ackSlots %d, ackBytes %d, maxRecords %d, maxAcks %d, junk %d: %s" \
            % (count, m, s, ab, maxRecords, maxAcks, kind, first_difference(got, want, count, maxRecords, maxAcks, ab))
    return got


def check_layout(L, layout, stride, m, s, ab, starts=None, ends=None, maxRecords=None, maxAcks=None, junk=(0, 1, 2, 3)):
    """check_raw for Row objects.  Returns (the output's bytes, the expectation per row)."""
    count = len(layout)
    st = starts if starts is not None else [0] * count
    en = ends if ends is not None else [stride] * count
    expect = [layout[k].expect(st[k], en[k], m, s, ab) for k in range(count)]
    got = check_raw(L, [r.bytes() for r in layout], stride, m, s, ab, starts, ends, expect, maxRecords, maxAcks, junk)
    return got, expect


def info(got):
    return struct.unpack_from("<4I", got, 0)


# 1 -------------------------------------------------------------------------
def start_end_rows(stride):
    """(rows, starts, ends): every residue of start and of end around a 16-byte
    boundary, with acks among the frames, and the degenerate windows."""
    rows, starts, ends = [], [], []

    def add(r, s, e):
        rows.append(r)
        starts.append(s)
        ends.append(e)

    for res in range(16):
        # the walk starts at a frame that begins at 32 + res, behind frames an earlier scan consumed
        r = Row(stride).add(original(res, 20)).to(32 + res).ack(1, payload(res, 1 + res)).add(recovery(50 + res, 21))
        add(r.add(original(70 + res, 13)), 32 + res, r.at)
        # ... and in the middle of the zero run before it
        r = Row(stride).ack(2, b"old").to(40 + res).add(original(90 + res, 14)).ack(1, payload(res, 5))
        add(r, 12 + res, r.at)
        # the data ends at 64 + res: right behind an ack's message, and behind zeros
        r = Row(stride).add(original(res, 30)).to(64 + res - 11).ack(3, payload(110 + res, 6))
        assert r.at == 64 + res
        add(r, 0, r.at)
        add(Row(stride).add(recovery(res, 25)).ack(0, b"abc").to(64 + res), 25, 64 + res)
    r = Row(stride).add(original(1, 20)).ack(1, payload(2, 15))
    add(r, 20, 20)            # start == end
    add(r, 0, 0)
    add(r, 40, 40)
    add(r, 41, 40)            # start past end
    add(r, stride + 1, 40)
    add(r, 0, stride + 16)    # end past the stride
    add(r, stride + 32, stride + 16)
    add(Row(stride).add(original(3, stride)), 0, stride)                  # one frame fills the row
    add(Row(stride).add(original(4, 20)), stride - 1, stride)             # start on the row's last byte, a zero
    fr = ack_frame(1, b"abc")
    add(Row(stride).to(stride - 1).add(fr[:1], total=len(fr)), stride - 1, stride)   # ... and a frame's first byte
    add(Row(stride).add(original(5, stride - 6)).ack(1, b"z", 1), stride - 6, stride)   # an ack ends the row
    return rows, starts, ends


def check_starts_and_ends(path):
    L = load(path)
    stride, m, s, ab = 128, 4, 2, 16
    rows, starts, ends = start_end_rows(stride)
    got, expect = check_layout(L, rows, stride, m, s, ab, starts, ends)
    bad = [k for k, (w, _) in enumerate(expect) if w == BAD]
    assert len(bad) == 4 and [expect[k][1] for k in bad] == [41, stride, 0, stride]
    assert expect[-3] == (0, stride) and expect[-2] == (PART, stride - 1) and expect[-1] == (1, stride)
    # the four null/given combinations (rows that walk from 0 and up to the stride as well)
    ok = [k for k in range(len(rows)) if k not in bad and k != len(rows) - 2]
    rows, starts, ends = [rows[k] for k in ok], [starts[k] for k in ok], [ends[k] for k in ok]
    for st in (starts, None):
        for en in (ends, None):
            check_layout(L, rows, stride, m, s, ab, st, en, junk=(0, 3))


# 2 -------------------------------------------------------------------------
def cuts():
    """(name, flag, frame bytes, left, never, total, good): every way a row's
    last frame can be cut off or be wrong."""
    out = []
    for w in (1, 2, 3, 4):
        for name, fr in (("ack", ack_frame(1, b"msg", w)), ("original", original(8, w + 9, w)),
                         ("recovery", recovery(9, w + 7, w))):
            for left in range(1, len(fr)):
                out.append(("%s (w %d) cut to %d" % (name, w, left), PART, fr, left, None, None, True))
            out.append(("%s (w %d) whole" % (name, w), 0, fr, len(fr), None, None, True))
    return out


def never_cuts(stride):
    out = []
    for w in (1, 2, 3, 4):
        if w > 1:
            big = prefix(stride, w) + bytes([ACK, 1, 0, 0])
            out.append(("w + L above the stride, prefix whole (w %d)" % w, BAD, big, w, w, w + stride, True))
            out.append(("w + L above the stride, prefix cut (w %d)" % w, PART, big, w - 1, w, w + stride, True))
            out.append(("L == 0 in a wide prefix (w %d)" % w, BAD, prefix(0, w), w + 3, None, None, False))
            out.append(("L == 0 in a wide prefix, its last byte the row's (w %d)" % w, BAD, prefix(0, w), w, None, None,
                        False))
        for t in (3, 0xff):
            fr = prefix(30, w) + bytes([t, 1, 0, 0]) + payload(t, 26)
            out.append(("type %#x present (w %d)" % (t, w), BAD, fr, w + 1, w + 1, None, False))
            out.append(("type %#x not yet there (w %d)" % (t, w), PART, fr, w, w + 1, None, False))
            out.append(("type %#x, whole (w %d)" % (t, w), BAD, fr, len(fr), w + 1, None, False))
        for kind, inner in ((ORIGINAL, 7), (RECOVERY, 4), (ACK, 4)):
            fr = prefix(inner, w) + bytes([kind, 1, 0, 0, 9, 0, 0][:inner])
            out.append(("L == inner of type %d, type present (w %d)" % (kind, w), BAD, fr, w + 1, w + 1, None, False))
            out.append(("L == inner of type %d, type not there (w %d)" % (kind, w), PART, fr, w, w + 1, None, False))
            out.append(("L == inner of type %d, whole (w %d)" % (kind, w), BAD, fr, len(fr), w + 1, None, False))
        # L = 5 is enough for an ack and a recovery frame and too little for an original: with the type byte
        # missing nothing is known yet
        fr = prefix(5, w) + bytes([ACK, 1, 0, 0, 0x55])
        out.append(("L 5, type not there (w %d)" % w, PART, fr, w, None, None, True))
        fr = prefix(27, w) + bytes([ORIGINAL, 1, 0, 0, 0x00, 0x00, 0x40]) + payload(3, 20)
        out.append(("PacketNum above the maximum, all there (w %d)" % w, BAD, fr, w + 7, w + 7, None, False))
        out.append(("PacketNum above the maximum, two bytes there (w %d)" % w, PART, fr, w + 6, w + 7, None, False))
        out.append(("PacketNum above the maximum, whole (w %d)" % w, BAD, fr, len(fr), w + 7, None, False))
    return out


def check_partial_frames(path):
    """Each cut behind zero, one and maxFrames - 1 good frames; stale bytes behind
    the cut filled with every kind of junk."""
    L = load(path)
    stride, m, s, ab = 256, 4, 2, 16
    all_cuts = cuts() + never_cuts(stride)
    assert len([c for c in all_cuts if c[1] == PART]) > 100 and len([c for c in all_cuts if c[1] == BAD]) > 40
    rows, ends, what = [], [], []
    for lead in (0, 1, m - 1):
        for name, flag, data, left, never, total, good in all_cuts:
            r = Row(stride)
            for j in range(lead):
                r.gap((len(rows) + j) % 3)
                r.ack(1, b"a%d" % j) if j == 1 else r.add(original(len(rows) + j, 12 + j))
            r.gap(len(rows) % 17 if lead == 1 else 0)   # (the cut frame at every residue mod 16)
            at = r.at
            r.add(data, good=good, never=never, total=total)
            rows.append(r)
            ends.append(at + left)
            what.append((name, flag, lead, at))
    for lo in range(0, len(rows), 200):   # (257 rows a scan at the most)
        hi = min(lo + 200, len(rows))
        got, expect = check_layout(L, rows[lo:hi], stride, m, s, ab, None, ends[lo:hi])
        for k in range(lo, hi):
            name, flag, lead, at = what[k]
            if flag:   # (the case's own statement of the outcome against Row.expect's)
                assert expect[k - lo] == (lead | flag, at), "%s behind %d frames: %#x" % (name, lead, expect[k - lo][0])
            else:
                assert expect[k - lo] == (lead + 1, ends[k]), name
    # a partial ack as the row's only ack: astart does not advance and no slot byte is non-zero
    r = Row(stride).add(original(1, 20)).ack(1, b"not yet here")
    got, expect = check_layout(L, [r], stride, m, s, ab, None, [r.at - 1])
    assert expect == [(1 | PART, 20)] and info(got) == (1, 1, 1, 0)
    so = DD.slots_offset(1, m)
    assert got[DD.acks_offset(1, m):so + s * ab] == bytes(so - DD.acks_offset(1, m) + s * ab)


# 3 -------------------------------------------------------------------------
def check_acks(path):
    L = load(path)
    # messages at every byte of a 16-byte word, of 1 .. ackBytes + 1 bytes, ackSlots 1, 2 and maxFrames, ackBytes 16
    # and 1024 (duplex_dense_cases.slot_rows): start 0 and no partial frame, so the words are the reference's
    m = 4
    for ab in (16, 1024):
        stride = ab + 80
        rows, lens = DD.slot_rows(ab, stride)
        for s in (1, 2):
            expect = [(None, e) for e in lens]
            for lo in range(0, len(rows), 112):
                check_raw(L, rows[lo:lo + 112], stride, m, s, ab, None, lens[lo:lo + 112], expect[lo:lo + 112],
                          junk=(0, 1, 3))
    # the flags together, and messages that straddle 16-byte words and end exactly at end
    stride, m, ab = 256, 5, 16
    long_msg = payload(9, ab + 1)
    for s in (1, 2):
        rows, ends = [], []

        def add(r, end=None):
            rows.append(r)
            ends.append(r.at if end is None else end)

        # one and two boundaries crossed, the message's last byte the window's last
        add(Row(stride).gap(9).ack(1, payload(1, 12)))                       # bytes 14..25
        add(Row(stride).gap(9).ack(1, payload(2, ab), 2))                    # bytes 15..30
        add(Row(stride).gap(10).ack(1, payload(3, ab)).ack(2, long_msg))     # bytes 15..30, then ackBytes + 1
        add(Row(stride).gap(27).ack(1, payload(4, ab)))                      # bytes 32..47: none crossed
        add(Row(stride).gap(11).ack(1, payload(5, 1)))                       # one byte, the word's last
        three = lambda: Row(stride).ack(1, b"first").add(original(7, 20)).ack(2, b"second").gap(2).ack(3, b"third")
        add(three())
        r = three().add(original(8, 30))
        add(r, r.at - 4)                                                     # dropped and partial (ackSlots 1, 2)
        add(three().add(recovery(9, 12)).add(original(10, 9)))               # dropped and more: a sixth frame
        add(three().add(bytes([30, 3, 0, 0, 0]) + payload(1, 26), good=False))   # dropped and malformed
        r = Row(stride).ack(1, long_msg).ack(2, b"ok")
        add(r.add(bytes([30, 0xee]), never=2, total=31), r.at + 2)           # too long, then a type never valid
        r = Row(stride).ack(1, long_msg).ack(1, b"cut short")
        add(r, r.at - 1)                                                     # too long, then a partial ack
        got, expect = check_layout(L, rows, stride, m, s, ab, None, ends)
        words = [w for w, _ in expect]
        assert words[:5] == [1, 1, 2 | DROPPED, 1, 1]
        assert words[5] == 4 | DROPPED
        assert words[6] == 4 | DROPPED | PART and words[7] == 5 | DROPPED | MORE and words[8] == 4 | DROPPED | BAD
        assert words[9] == 2 | DROPPED | BAD and words[10] == 1 | DROPPED | PART
        assert expect[6][1] == rows[6].parts[4][0] and expect[10][1] == rows[10].parts[1][0]
        # the record of the third ack of a row with ackSlots slots
        st = struct.unpack_from("<%dI" % (len(rows) + 1), got, 16 + 4 * len(rows))
        h = PackedHead.from_buffer_copy(got, DD.records_offset(len(rows)) + (st[5] + 3) * REC)
        assert (h.Type, h.PacketNum, h.Status) == (ACK, 2, ROW_TRUNCATED)


# 4 -------------------------------------------------------------------------
def check_row_end(path):
    """Frames that start in the row's last 16 bytes, where the walk loads no
    second word, and maxFrames 1 and 256."""
    L = load(path)
    stride, m, s, ab = 128, 4, 2, 16
    rows, starts = [], []
    for d in range(1, 17):
        at = stride - d
        lead = lambda: Row(stride).add(original(d, 20)).to(at)
        # whole frames that end with the row
        if d >= 6:
            rows.append(lead().ack(1, payload(d, d - 5)))
            rows.append(lead().add(recovery(d, d)))
        if d >= 9:
            rows.append(lead().add(original(100 + d, d)))
        # frames the row cannot hold whole (w + L <= stride): partial, whatever lies behind the row
        for w in (1, 2, 3, 4):
            for fr in (prefix(5, w) + bytes([ACK, 1, 0, 0, 0x55]), original(200 + d, 40, w), recovery(d, 33, w),
                       ack_frame(2, payload(d, 20), w)):
                rows.append(lead().add(fr[:d], total=len(fr)) if d < len(fr) else lead().add(fr))
        # a type byte that is never valid, present or not
        fr = bytes([30, 3, 0, 0, 0]) + payload(1, 26)
        rows.append(lead().add(fr[:d], good=False, never=2, total=len(fr)))
    ends = [stride] * len(rows)
    for lo in range(0, len(rows), 200):
        got, expect = check_layout(L, rows[lo:lo + 200], stride, m, s, ab, None, ends[lo:lo + 200], junk=(0, 3))
        assert all(nxt in (stride, r.parts[1][0]) for r, (w, nxt) in zip(rows[lo:], expect))
    check_layout(L, rows[:150], stride, m, s, ab, None, None, junk=(0,))   # a null ends array

    # maxFrames reached: only zeros left (no flag, next = end), a non-zero byte left (MORE, next = that byte)
    stride = 2048
    for m in (1, 256):
        full = Row(stride)
        for i in range(m):
            full.ack(1, b"k") if i % 64 == 7 else full.add(recovery(i, 6) if i % 2 else original(i, 9))
        tail = full.at
        rows = [full, Row(stride), Row(stride)]
        for r in rows[1:]:
            r.buf, r.parts, r.ackAt = bytearray(full.buf), list(full.parts), dict(full.ackAt)
        rows[1].gap(5).ack(2, b"more")
        rows[2].gap(1).add(bytes([9]), total=10)
        sl = min(m, 2)
        got, expect = check_layout(L, rows, stride, m, sl, ab, None, [tail + 9, rows[1].at, rows[2].at], junk=(0, 1))
        flag = DROPPED if m == 256 else 0   # (256 frames hold four acks, ackSlots 2)
        assert expect == [(m | flag, tail + 9), (m | flag | MORE, tail + 5), (m | flag | MORE, tail + 1)]


# 5 -------------------------------------------------------------------------
def check_row_counts(path, count):
    """A mixture of outcomes per row at one row count: workgroup edges."""
    L = load(path)
    stride, m, s, ab = 128, 2, 1, 16
    rows, starts, ends = start_end_rows(stride)
    rows.insert(0, Row(stride).ack(1, b"one").ack(1, b"two: no slot"))
    starts.insert(0, 0)
    ends.insert(0, rows[0].at)
    extra = cuts()
    for i in range(0, len(extra), 7):
        name, flag, data, left, never, total, good = extra[i]
        r = Row(stride).ack(1, b"x").gap(i % 5)
        at = r.at
        rows.append(r.add(data))
        starts.append(0)
        ends.append(at + left)
    pick = [(7 * k) % len(rows) for k in range(count)]
    rows, starts, ends = [rows[k] for k in pick], [starts[k] for k in pick], [ends[k] for k in pick]
    got, expect = check_layout(L, rows, stride, m, s, ab, starts, ends, junk=(0, 2))
    if count >= 63:
        words = [w for w, _ in expect]
        assert all(any(w & f for w in words) for f in (PART, BAD, MORE, DROPPED)) and any(w < 4 for w in words)


def check_dense_equivalence(path):
    """Start 0 and no partial frame: the first duplex_dense_bytes bytes are
    sgpu_frames_scan_duplex_dense's on the same rows, with and without ends."""
    L = load(path)
    stride, m, s, ab = 96, 4, 2, 16
    for count in (1, 70, KC["walk"] + 1):
        rows, lens, ns, aks = DD.mixed_rows(count, stride, m, s, 900 + count)
        dr = K.DevRows(L, rows, stride, lens)
        for maxRecords, maxAcks in ((count * m, count * s), (max(m, sum(ns) // 2), max(s, sum(aks) // 3))):
            dense, o = DD.scan(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords, maxAcks)
            o.free()
            for ends in (dr.lens, None):
                oo = Out(L, count, maxRecords, maxAcks, ab)
                t = L.sgpu_frames_scan_duplex_streams(dr.dev, stride, None, ends, count, m, s, ab, maxRecords, maxAcks,
                                                      oo.out)
                assert t > 0 and L.sgpu_gather_wait(t) == 0
                got = oo.fetch()
                oo.free()
                if ends:
                    assert got[:len(dense)] == dense
                    assert got[len(dense):] == struct.pack("<%dI" % count, *lens) + bytes(-4 * count % 16)
                else:   # (the zero tail of a row holds nothing)
                    assert got[:len(dense)] == dense
                    assert got[len(dense):] == struct.pack("<%dI" % count, *([stride] * count)) + bytes(-4 * count % 16)
        dr.free()


# 6 -------------------------------------------------------------------------
def recv(L, decs, encs, out, m, s, ab, maxRecords, maxAcks, dev, stride, count):
    res = (C.c_int * maxRecords)(*([-1] * maxRecords))
    nxt = (C.c_uint * maxRecords)(*([0xEEEE] * maxRecords))
    cons = (C.c_uint * count)(*([0xdeadbeef] * count))
    nrows, n = C.c_uint(12345), C.c_uint(12345)
    r = L.sgpu_frames_recv_duplex_streams(decs, len(decs) if decs else 0, encs, len(encs) if encs else 0, out, m, s,
                                          ab, maxRecords, maxAcks, dev, stride, count, res, nxt, cons, C.byref(nrows),
                                          C.byref(n))
    return r, list(res), list(nxt), list(cons), nrows.value, n.value


def check_cut(path):
    """Rows are all or nothing over both budgets; the next words of the rows from
    c on are present, and consumedOut is left untouched for them."""
    L = load(path)
    stride, m, s, ab, count = 128, 4, 2, 16, 20
    snd = Pair(L, [payload(i, 20) for i in range(4)])
    for i in range(4):
        assert snd.add(i) == (SUCCESS, i)
    assert snd.recv(0) == SUCCESS
    r, _, msg = snd.ack(16)
    assert r == SUCCESS
    rows, ns, aks = [], [], []
    for k in range(count):
        r = Row(stride)
        n, a = 1 + k % 4, (k % 3 == 0) + (k % 6 == 0)
        for j in range(n):
            r.gap(j)
            r.ack(0, msg) if j < a else r.add(original(10 * k + j, 12 + j, flow=0))
        rows.append(r)
        ns.append(n)
        aks.append(min(a, n))
    rows[5].add(original(99, 40, flow=0))
    ends = [r.at for r in rows]
    ends[5] -= 7   # row 5 ends in a partial frame
    st = [sum(ns[:k]) for k in range(count + 1)]
    ast = [sum(aks[:k]) for k in range(count + 1)]
    T, TA = st[count], ast[count]
    rowR = 10   # three frames, no ack: fails maxRecords alone
    rowA = 12   # one frame, an ack: fails maxAcks alone
    assert ns[rowR] == 3 and aks[rowR] == 0 and aks[rowA] == 1
    for maxRecords, maxAcks, wantC in ((st[rowR] + 1, count * s, rowR), (count * m, ast[rowA], rowA), (T, TA, count),
                                       (m, s, max(k for k in range(count + 1) if st[k] <= m and ast[k] <= s))):
        got, expect = check_layout(L, rows, stride, m, s, ab, None, ends, maxRecords, maxAcks, junk=(0,))
        gT, W, c, WA = info(got)
        assert (gT, W, c, WA) == (T, st[wantC], wantC, ast[wantC]), (maxRecords, maxAcks)
        assert expect[5][0] == 2 | PART
        nextAt = L.sgpu_frames_duplex_streams_next(count, maxRecords, maxAcks, ab)
        assert list(struct.unpack_from("<%dI" % count, got, nextAt)) == [e[1] for e in expect]
        o = Out(L, count, maxRecords, maxAcks, ab)
        C.memmove(o.out, got, len(got))
        ds = DevStreams(L, [r.bytes() for r in rows], stride)
        dec, rcv = L.sgpu_decoder_create(), Pair(L, snd.data)
        for i in range(4):
            assert rcv.add(i) == (SUCCESS, i)
        r, res, nxt, consumed, nrows, n = recv(L, (C.c_void_p * 1)(dec), (C.c_void_p * 1)(rcv.enc), o.out, m, s, ab,
                                               maxRecords, maxAcks, ds.dev, stride, count)
        assert (nrows, n) == (c, W) and r in (SUCCESS, 4), r   # (the same ack again is a duplicate)
        assert consumed[:c] == [e[1] for e in expect[:c]] and consumed[c:] == [0xdeadbeef] * (count - c)
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
        rcv.free()
        o.free()
        ds.free()
    snd.free()


# 7 -------------------------------------------------------------------------
def encoder_stats(L, enc):
    return DD.encoder_stats(L, enc)


def check_resume(path):
    """Two peers, each with an encoder and a decoder.  Row d is the receive
    buffer of direction d's receiver: the sender's originals and recovery frames
    (flow d, for the receiver's decoder) and the sender's acks of what it got in
    the other direction (flow 1 - d, for the receiver's encoder).  The rows arrive
    in pieces of 1 to 37 bytes; every round scans from the last round's consumed
    words with maxFrames 2.  A twin set of instances takes the complete rows
    through one sgpu_frames_scan_duplex_dense and sgpu_frames_recv_duplex_dense."""
    L = load(path)
    npk = 10
    lengths = [30 + (i * 37) % 90 for i in range(npk)]
    lost = {0: (1, 6), 1: (0, 3, 8)}
    senders = [Sender(L, lengths, seed=470 + d) for d in range(2)]
    frames = [P.wire_frames(L, senders[d], d, [k for k in range(npk) if k not in lost[d]], len(lost[d]) + 1)
              for d in range(2)]
    # the acks a receiver would write while it gets the packets: three states of a model decoder
    adata = [payload(300 + i, 40 + i) for i in range(npk)]
    model = Pair(L, adata)
    for i in range(npk):
        assert model.add(i) == (SUCCESS, i)
    msgs = []
    for got in ((0, 1), (3, 4), (2, 5, 6, 7)):
        for i in got:
            assert model.recv(i) == SUCCESS
        r, _, msg = model.ack(48)
        assert r == SUCCESS and 1 <= len(msg) <= 48
        msgs.append(msg)
    model.free()
    rnd = random.Random(67)
    stride, m, s, ab = 2048, 2, 2, 48
    layout, acksIn = [], []
    for d in range(2):
        r = Row(stride)
        slots = sorted(rnd.sample(range(len(frames[d])), len(msgs)))
        if d == 1:
            slots[1] = slots[0]   # two acks back to back
        for i, fr in enumerate(frames[d]):
            for j, at in enumerate(slots):
                if at == i:
                    r.gap(rnd.randrange(3)).ack(1 - d, msgs[j])
            r.gap(rnd.randrange(3)).add(fr)
        layout.append(r)
        acksIn.append(len(msgs))
    count = 2
    total = sum(len(r.parts) for r in layout)
    full = [r.bytes() for r in layout]
    lengthOf = [r.at for r in layout]

    class World:
        def __init__(self):
            self.decs = (C.c_void_p * 2)(*[L.sgpu_decoder_create() for _ in range(2)])
            self.pairs = [Pair(L, adata) for _ in range(2)]   # (their encoders take the acks)
            for p in self.pairs:
                for i in range(npk):
                    assert p.add(i) == (SUCCESS, i)
            self.encs = (C.c_void_p * 2)(*[p.enc for p in self.pairs])

        def state(self):
            return ([DN.decoder_stats(L, d) for d in self.decs], [encoder_stats(L, p.enc) for p in self.pairs],
                    [[L.sgpu_decoder_has(self.decs[d], i) for i in range(npk)] for d in range(2)])

        def free(self):
            for d in self.decs:
                L.sgpu_decoder_free(d)
            for p in self.pairs:
                p.free()

    one, two = World(), World()
    ds = DevStreams(L, [bytes(stride)] * count, stride)
    starts, ends = [0] * count, [0] * count
    acc = rounds = partials = mores = 0
    flat = [[], []]   # per row: (result, next expected) of every record, in order
    s0 = stats(L)
    while starts != lengthOf:
        rounds += 1
        assert rounds < 400
        for k in range(count):   # the transport appends a piece to every row
            more = min(lengthOf[k] - ends[k], 1 + rnd.randrange(37))
            if more:
                assert L.sgpu_h2d(ds.dev + k * stride + ends[k], full[k][ends[k]:ends[k] + more], more) == 0
            ends[k] += more
        have = [Row(stride) for _ in range(count)]
        for k in range(count):
            have[k].buf, have[k].parts, have[k].ackAt = bytearray(full[k][:ends[k]]), layout[k].parts, layout[k].ackAt
        expect = [have[k].expect(starts[k], ends[k], m, s, ab) for k in range(count)]
        maxRecords, maxAcks = count * m, count * s
        want, ref, _ = expected_output(L, [h.bytes() for h in have], stride, starts, ends, expect, m, s, ab, maxRecords,
                                       maxAcks)
        ref.free()
        ds.put(ds.starts, starts)
        ds.put(ds.ends, ends)
        got, o = scan(L, ds, ds.starts, ds.ends, m, s, ab, maxRecords, maxAcks)
        assert got == want, "round %d: %s" % (rounds, first_difference(got, want, count, maxRecords, maxAcks, ab))
        r, res, nxt, consumed, nrows, n = recv(L, one.decs, one.encs, o.out, m, s, ab, maxRecords, maxAcks, ds.dev,
                                               stride, count)
        assert r == SUCCESS and nrows == count and consumed == [e[1] for e in expect]
        assert not any(w & DROPPED for w, _ in expect), "every ack has a slot: none is behind a next word unread"
        st = struct.unpack_from("<%dI" % (count + 1), got, 16 + 4 * count)
        for k in range(count):
            for i in range(st[k], st[k + 1]):
                h = PackedHead.from_buffer_copy(got, DD.records_offset(count) + i * REC)
                flat[k].append((res[i], nxt[i] if h.Type == ACK else None))
        partials += sum(1 for w, _ in expect if w & PART)
        mores += sum(1 for w, _ in expect if w & MORE)
        acc += n
        assert L.sgpu_flush() == 0
        o.free()
        starts = consumed
    assert stats(L)[STAT_DUPLEX_STREAMS] - s0[STAT_DUPLEX_STREAMS] == rounds * count
    assert acc == total and partials > 20 and mores >= 1, "every frame exactly once"
    # the twin: the complete rows in one dense duplex scan
    M = max(len(r.parts) for r in layout)
    S = max(acksIn)
    dr = K.DevRows(L, full, stride, lengthOf)
    gotD, od = DD.scan(L, dr.dev, stride, dr.lens, count, M, S, ab, count * M, count * S)
    r, resD, nxtD, nrowsD, nD = DD.recv(L, two.decs, two.encs, od.out, M, S, ab, count * M, count * S, dr.dev, stride,
                                        count)
    assert (r, nrowsD, nD) == (SUCCESS, count, total)
    stD = struct.unpack_from("<%dI" % (count + 1), gotD, 16 + 4 * count)
    for k in range(count):
        twin = []
        for i in range(stD[k], stD[k + 1]):
            h = PackedHead.from_buffer_copy(gotD, DD.records_offset(count) + i * REC)
            twin.append((resD[i], nxtD[i] if h.Type == ACK else None))
        assert flat[k] == twin, "row %d" % k
    od.free()
    assert L.sgpu_flush() == 0
    assert one.state() == two.state()
    for d in range(2):
        for w in (one, two):
            out, k = C.c_void_p(), C.c_uint(0)
            assert L.sgpu_decoder_is_ready(w.decs[d]) == SUCCESS
            assert L.sgpu_decode(w.decs[d], C.byref(out), C.byref(k)) == SUCCESS and k.value == len(lost[d])
        a, atail = K.delivered(L, one.decs[d], npk, 128)
        b, btail = K.delivered(L, two.decs[d], npk, 128)
        assert a == b == senders[d].data and atail == btail
    assert L.sgpu_flush() == 0
    one.free()
    two.free()
    assert L.sgpu_flush() == 0
    dr.free()
    ds.free()
    for sn in senders:
        sn.free()


# 8 -------------------------------------------------------------------------
def check_arguments(path, gpu):
    """Every refusal with nothing queued and the counters unchanged; count == 0;
    the size functions; the counter and the timing entries of the one scan that
    was queued."""
    L = load(path)
    stride, count, m, s, ab = 64, 4, 2, 1, 16
    rows = [Row(stride).add(original(k, 19 + k, flow=0)).gap(3).ack(0, payload(5, 4)) for k in range(count)]
    ds = DevStreams(L, [r.bytes() for r in rows], stride)
    ds.put(ds.starts, [0] * count)
    ds.put(ds.ends, [r.at for r in rows])
    maxRecords, maxAcks = count * m, count * s
    o = Out(L, count, maxRecords, maxAcks, ab)
    p = Pair(L, [payload(1, 20)])
    decs, encs = (C.c_void_p * 1)(p.dec), (C.c_void_p * 1)(p.enc)
    assert L.sgpu_flush() == 0
    s0 = stats(L)
    B, N, D = L.sgpu_frames_duplex_streams_bytes, L.sgpu_frames_duplex_streams_next, L.sgpu_frames_duplex_dense_bytes
    for args in ((3, 0, 3, 16), (3, 3 * 256 + 1, 3, 16), (3, 3, 0, 16), (3, 3, 3 * 256 + 1, 16), (0, 1, 1, 16),
                 (3, 3, 3, 0), (3, 3, 3, 8), (3, 3, 3, 24), (3, 3, 3, 1040), (1 << 20, 1 << 27, 1 << 20, 1024)):
        assert D(*args) == 0 and B(*args) == 0 and N(*args) == 0, args
    assert N(3, 6, 3, 16) == D(3, 6, 3, 16) == 48 + 6 * 32 + 16 + 3 * 16 and B(3, 6, 3, 16) == N(3, 6, 3, 16) + 16
    assert [B(n, 256, 1, 16) - N(n, 256, 1, 16) for n in (1, 4, 5, 8, 9)] == [16, 16, 32, 32, 48]
    # the 4 GiB edge: the dense part still fits and the next words push the output to 4 GiB
    edge = (1 << 32) // 60 - 4
    while DD.slots_offset(edge, edge) + 16 * edge + ((4 * edge + 15) & ~15) < 1 << 32:
        edge += 1

    def scan_args(**kw):
        a = dict(rows=ds.dev, stride=stride, starts=ds.starts, ends=ds.ends, count=count, m=m, s=s, b=ab, r=maxRecords,
                 a=maxAcks, out=o.out)
        a.update(kw)
        return L.sgpu_frames_scan_duplex_streams(a["rows"], a["stride"], a["starts"], a["ends"], a["count"], a["m"],
                                                 a["s"], a["b"], a["r"], a["a"], a["out"])

    shared = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=ds.dev + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=72)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("maxFrames zero", dict(m=0)),
        ("maxFrames above 256", dict(m=257, r=4 * 257)),
        ("ackSlots zero", dict(s=0)),
        ("ackSlots above maxFrames", dict(s=3, a=4 * 3)),
        ("ackBytes zero", dict(b=0)),
        ("ackBytes below 16", dict(b=8)),
        ("ackBytes no multiple of 16", dict(b=24)),
        ("ackBytes above 1024", dict(b=1040)),
        ("maxRecords below maxFrames", dict(r=m - 1)),
        ("maxRecords zero", dict(r=0)),
        ("maxRecords above count * maxFrames", dict(r=count * m + 1)),
        ("maxAcks below ackSlots", dict(m=4, s=2, r=8, a=1)),
        ("maxAcks zero", dict(a=0)),
        ("maxAcks above count * ackSlots", dict(a=count * s + 1)),
    ]
    more = [("null output", dict(out=None)), ("output not 16-byte aligned", dict(out=o.out + 8)),
            ("starts not 4-byte aligned", dict(starts=ds.starts + 2)),
            ("ends not 4-byte aligned", dict(ends=ds.ends + 1)),
            ("a duplex output above 4 GiB", dict(count=1 << 19, m=256, s=1, r=256, a=1)),
            ("an output of 4 GiB", dict(count=edge, m=1, s=1, r=edge, a=edge))]
    for what, kw in shared + more:
        assert scan_args(**kw) == -1, what
    assert L.sgpu_flush() == 0
    assert o.untouched()
    s1 = stats(L)
    watched = (0, 1, STAT_DUPLEX_STREAMS, ST.STAT_STREAMS, DD.STAT_DUPLEX_DENSE, DD.STAT_DENSE, DD.STAT_DUPLEX)
    assert [s1[i] for i in watched] == [s0[i] for i in watched]

    L.sgpu_timing(1, 1, None, None)
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_ACKSTREAMWALK] > 0 and ms[TIMING_ROWSUM2] > 0 and ms[TIMING_COMPACT] > 0 and \
            ms[TIMING_SLOTS] > 0
        assert ms[TIMING_ACKWALK] == 0 and ms[TIMING_STREAMWALK] == 0, "the duplex stream walk has its own entry"
    got = o.fetch()
    expect = [r.expect(0, r.at, m, s, ab) for r in rows]
    want, ref, _ = expected_output(L, [r.bytes() for r in rows], stride, [0] * count, [r.at for r in rows], expect, m, s,
                                   ab, maxRecords, maxAcks)
    ref.free()
    assert got == want and info(got) == (8, 8, 4, 4)
    s2 = stats(L)
    assert s2[STAT_DUPLEX_STREAMS] - s1[STAT_DUPLEX_STREAMS] == count, "only the one valid scan was counted"
    assert s2[DD.STAT_DUPLEX_DENSE] - s1[DD.STAT_DUPLEX_DENSE] == count, "(the reference scan of this case)"
    assert s2[ST.STAT_STREAMS] == s1[ST.STAT_STREAMS]

    def recv_args(**kw):
        a = dict(decs=decs, encs=encs, heads=o.out, rows=ds.dev, stride=stride, count=count, m=m, s=s, b=ab,
                 r=maxRecords, a=maxAcks, rowsOut=True, consumed=True)
        a.update(kw)
        n, nrows = C.c_uint(99), C.c_uint(99)
        res = (C.c_int * maxRecords)(*([-1] * maxRecords))
        cons = (C.c_uint * count)(*([77] * count))
        r = L.sgpu_frames_recv_duplex_streams(a["decs"], 1, a["encs"], 1, a["heads"], a["m"], a["s"], a["b"], a["r"],
                                              a["a"], a["rows"], a["stride"], a["count"], res, None,
                                              cons if a["consumed"] else None,
                                              C.byref(nrows) if a["rowsOut"] else None, C.byref(n))
        return r, n.value, nrows.value if a["rowsOut"] else 0, list(res), list(cons)

    for what, kw in shared + [("null decoders", dict(decs=None)), ("null encoders", dict(encs=None)),
                              ("null output", dict(heads=None)), ("output not 4-byte aligned", dict(heads=o.out + 2)),
                              ("null rowsOut", dict(rowsOut=False)), ("null consumedOut", dict(consumed=False))]:
        assert recv_args(**kw) == (INVALID, 0, 0, [-1] * maxRecords, [77] * count), what
    for k in range(count):
        assert L.sgpu_decoder_has(p.dec, k) == NEED_MORE, "a refused call must not reach the decoder"
    assert p.enc_stats()[6] == 0, "a refused call must not reach the encoder"

    # count == 0: a ticket that is complete, nothing scanned, nothing written; nothing accepted
    before = C.string_at(o.base, o.bytes)
    for kw in (dict(count=0), dict(count=0, r=0, a=0), dict(count=0, rows=None, starts=None, ends=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    assert recv_args(count=0)[:3] == (SUCCESS, 0, 0)
    assert recv_args(count=0, heads=None, rows=None, consumed=False)[:3] == (SUCCESS, 0, 0)
    assert L.sgpu_flush() == 0
    s3 = stats(L)
    assert [s3[i] for i in watched] == [s2[i] for i in watched], "nothing was queued by any of them"
    assert C.string_at(o.base, o.bytes) == before

    # (the arguments were fine otherwise: the originals are accepted, the acks are no messages of a decoder)
    r, n, nrows, res, cons = recv_args()
    assert nrows == count and res[0::2] == [SUCCESS] * count and n >= count and cons == [r.at for r in rows]
    assert L.sgpu_flush() == 0
    p.free()
    o.free()
    ds.free()


# 9 (the CPU double only) ----------------------------------------------------
def check_forged(path):
    """The output is caller data: sgpu_frames_recv_duplex_streams refuses what no
    scan could have written (duplex_streams_forged_test.cpp runs these under the
    sanitizers)."""
    L = load(path)
    stride, m, s, ab, count = 128, 2, 1, 16, 6
    data = [payload(800 + i, 12 + i) for i in range(2 * count)]
    snd = Pair(L, data)
    for i in range(2 * count):
        assert snd.add(i) == (SUCCESS, i)
    assert snd.recv(0) == SUCCESS and snd.recv(2) == SUCCESS
    r, _, msg = snd.ack(16)
    assert r == SUCCESS and len(msg) <= ab
    rows = [Row(stride).add(frame(ORIGINAL, 0, 50 + k, payload(800 + k, 12 + k))).gap(1 + k).ack(0, msg)
            for k in range(count)]
    ds = DevStreams(L, [r.bytes() for r in rows], stride)
    ds.put(ds.ends, [r.at for r in rows])
    maxRecords, maxAcks = count * m, count * s
    good, o = scan(L, ds, None, ds.ends, m, s, ab, maxRecords, maxAcks)
    nextAt = o.next
    startAt, recAt = 16 + 4 * count, DD.records_offset(count)
    ackAt = DD.acks_offset(count, maxRecords)

    def word(at, v):
        return lambda b: b.__setitem__(slice(at, at + 4), struct.pack("<I", v))

    def record(i, **kw):
        def edit(b):
            h = PackedHead.from_buffer_copy(b, recAt + i * REC)
            for f, v in kw.items():
                setattr(h, f, v)
            b[recAt + i * REC:recAt + (i + 1) * REC] = bytes(h)
        return edit

    def both(*edits):
        return lambda b: [e(b) for e in edits]

    # (what is forged, the result, rows routed before the refusal, frames accepted)
    cases = [
        ("nothing forged", lambda b: None, SUCCESS, count, 2 * count),
        ("a next word above the stride", word(nextAt + 4 * 2, stride + 1), INVALID, 2, 4),
        ("a huge next word", word(nextAt, 0xffffffff), INVALID, 0, 0),
        ("a next word below the end of the row's last record", word(nextAt + 4 * 3, rows[3].at - 1), INVALID, 3, 6),
        ("a next word of zero behind records", word(nextAt + 4 * 5, 0), INVALID, 5, 10),
        ("a next word at the stride", word(nextAt + 4 * 4, stride), SUCCESS, count, 2 * count),
        ("an astart step that disagrees with the row's ack records", word(ackAt + 4 * 2, 3), INVALID, 1, 2),
        ("a start beyond W", word(startAt + 4 * 3, maxRecords + 1), INVALID, 2, 4),
        ("c > count", word(8, count + 1), INVALID, 0, 0),
        ("a slot index outside the row's span", record(3, PacketNum=1), INVALID, 1, 2),
        ("a word count above maxFrames", word(16, m + 1), INVALID, count, 2 * count - 2),
        ("the partial flag on a complete row", word(16 + 4, 2 | PART), SUCCESS, count, 2 * count),
        ("the partial flag together with a forged record", both(word(16 + 4, 2 | PART), record(2, Offset=stride - 8)),
         INVALID, count, 2 * count - 1),
    ]
    for what, forge, result, rowsDone, accepted in cases:
        b = bytearray(good)
        forge(b)
        C.memmove(o.out, bytes(b), len(b))
        rcv, dec = Pair(L, data), L.sgpu_decoder_create()
        for i in range(2 * count):
            assert rcv.add(i) == (SUCCESS, i)
        r, res, nxt, consumed, nrows, n = recv(L, (C.c_void_p * 1)(dec), (C.c_void_p * 1)(rcv.enc), o.out, m, s, ab,
                                               maxRecords, maxAcks, ds.dev, stride, count)
        assert (r, nrows, n) == (result, rowsDone, accepted), "%s: %r" % (what, (r, nrows, n))
        nw = struct.unpack_from("<%dI" % count, b, nextAt)
        assert consumed == list(nw[:rowsDone]) + [0xdeadbeef] * (count - rowsDone), what
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
        rcv.free()
    assert L.sgpu_flush() == 0
    o.free()
    ds.free()
    snd.free()
