"""sgpu_frames_scan_streams / sgpu_frames_recv_streams: the cases shared by
test_streams_cpu.py (the CPU test double, tests/hostsim) and test_streams_gpu.py
(k_streamwalk, k_rowsum and k_compact on the MI355X), driven through the C ABI
with ctypes.

The yardstick is existing code, never the code under test.  The first part of
every expected output is what sgpu_frames_scan_dense writes for a copy of the
rows with [0, start) zeroed and, for a row that ends in a partial frame, [next,
end) zeroed too, with the rows' ends as its length words (test_dense_* pin that
scan to sgpu_frames_scan_packed and test_pack_* pin that one to
sgpu_frames_parse).  The next words and the SGPU_STREAM_PARTIAL bits are worked
out here from the frame lists a case laid out (Row.expect), never from the bytes.
A row with start > end or end > stride has no such copy: the contract gives it
the word and the records of a row whose length word exceeds the stride, which is
what the copy's length word is set to.  The whole pinned buffer is compared byte
for byte between two guard records pre-filled with 0xA5.  For routing a second
set of decoders is fed by sgpu_frames_recv_dense on the zeroed copy, and the two
sets must agree.

The chunk the walk stages at a time comes from the kernel's constant in
siamese_amd/csrc/ops.h (kStreamChunk).
"""
import ctypes as C
import os
import random
import re
import struct

import dense_cases as DN
import pack_cases as P
import scan_cases as K
from deliver_cases import FILL, INVALID, NEED_MORE, SUCCESS, payload
from frame_cases import ORIGINAL, RECOVERY, Sender
from pack_cases import REC, frame, prefix
from siamese_amd.binding import (PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, STREAM_PARTIAL,
                                 bind_streams_abi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_STREAMS = 42
NSTATS = 43
TIMING_ROWSUM, TIMING_COMPACT, TIMING_STREAMWALK, NTIMING = 15, 16, 19, 20
PACKET_NUM_MAX = 0x3fffff


def kernel_constants():
    with open(os.path.join(ROOT, "siamese_amd", "csrc", "ops.h")) as f:
        src = f.read()

    def value(name):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m, "%s not found in ops.h" % name
        return int(m.group(1))

    return dict(chunk=value("kStreamChunk"), walk=value("kWalkThreads"))


KC = kernel_constants()
CH = KC["chunk"]
ROW_COUNTS = [1, 63, 64, 65, KC["walk"] - 1, KC["walk"] + 1]


def load(path):
    L = DN.load(path)
    if getattr(L, "_streams_cases", False):
        return L
    # (the four symbols under test: an AttributeError here is the parent's answer)
    bind_streams_abi(L)
    L._streams_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


# ---------------------------------------------------------------------------
# rows as lists of frames

class Row:
    """One stream row laid out frame by frame.  A part is (offset, bytes in the
    row, w + L as its prefix states it, good: accepted when whole, never: the
    fewest bytes present at which the frame can no longer become valid, or None)."""

    def __init__(self, stride):
        self.stride, self.buf, self.parts = stride, bytearray(), []

    def gap(self, n):
        self.buf += bytes(n)
        return self

    def to(self, offset):
        assert offset >= len(self.buf), "offset %d is behind the cursor %d" % (offset, len(self.buf))
        return self.gap(offset - len(self.buf))

    def add(self, data, good=True, never=None, total=None):
        assert data[0] != 0
        self.parts.append((len(self.buf), len(data), len(data) if total is None else total, good, never))
        self.buf += data
        return self

    @property
    def at(self):
        return len(self.buf)

    def bytes(self):
        assert len(self.buf) <= self.stride, "%d bytes in a row of %d" % (len(self.buf), self.stride)
        return bytes(self.buf) + bytes(self.stride - len(self.buf))

    def expect(self, start, end, m):
        """(row word, next) of a walk of [start, end) with maxFrames m; start lies
        at a frame's first byte or in a zero gap."""
        if start > end or end > self.stride:
            return PACKED_MALFORMED, min(start, self.stride)
        n = 0
        for off, have, total, good, never in self.parts:
            if off + have <= start:
                continue
            assert off >= start, "the case's start %d lies inside the frame at %d" % (start, off)
            if off >= end:
                break
            if n == m:
                return n | PACKED_MORE, off
            if off + total > end:
                left = end - off
                return n | (PACKED_MALFORMED if never is not None and left >= never else STREAM_PARTIAL), off
            assert have == total
            if not good:
                return n | PACKED_MALFORMED, off
            n += 1
        return n, end


def narrowest(size):
    """The narrowest prefix with which a frame of `size` bytes in all can be stated."""
    return 1 if size - 1 < 0x80 else 2 if size - 2 < 0x4000 else 3


def original(num, size, width=None, flow=5):
    """An original's frame of `size` bytes in all."""
    width = width or narrowest(size)
    data = size - width - 7
    assert data >= 1
    return frame(ORIGINAL, flow, num & PACKET_NUM_MAX, payload(num, data), width)


def recovery(seed, size, width=None, flow=6):
    width = width or narrowest(size)
    data = size - width - 4
    assert data >= 1
    return frame(RECOVERY, flow, 0, payload(seed, data), width)


# ---------------------------------------------------------------------------
# one scan against the dense scan of the zeroed copy

class DevStreams:
    """Rows, starts and ends in device memory; the row area is exactly count *
    stride bytes, so the last row ends where the allocation ends."""

    def __init__(self, L, rows, stride):
        self.L, self.stride, self.count = L, stride, len(rows)
        blob = b"".join(rows)
        assert len(blob) == stride * len(rows)
        self.dev = L.sgpu_device_alloc(len(blob))
        self.starts = L.sgpu_device_alloc(4 * len(rows))
        self.ends = L.sgpu_device_alloc(4 * len(rows))
        assert self.dev and self.starts and self.ends and self.dev % 16 == 0
        assert L.sgpu_h2d(self.dev, blob, len(blob)) == 0

    def put(self, where, values):
        raw = struct.pack("<%dI" % len(values), *values)
        assert self.L.sgpu_h2d(where, raw, len(raw)) == 0

    def free(self):
        for p in (self.dev, self.starts, self.ends):
            self.L.sgpu_device_free(p)


class Out:
    """A stream scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxRecords):
        self.L = L
        self.total = L.sgpu_frames_streams_bytes(count, maxRecords)
        self.next = L.sgpu_frames_streams_next(count, maxRecords)
        assert self.next == L.sgpu_frames_dense_bytes(count, maxRecords) == DN.records_offset(count) + maxRecords * REC
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
    """(rows, length words) of the dense scan that states the expectation."""
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
        if word & STREAM_PARTIAL:
            b[nxt:e] = bytes(e - nxt)
        rows.append(bytes(b))
        lens.append(e)
    return rows, lens


def expected_output(L, rowBytes, stride, starts, ends, expect, m, maxRecords):
    """The bytes the contract asks for, the reference copy's DevRows (the caller
    frees it) and the reference dense bytes."""
    count = len(rowBytes)
    rows, lens = zeroed_copy(rowBytes, stride, starts, ends, expect)
    ref = K.DevRows(L, rows, stride, lens)
    dense, o = DN.scan(L, ref.dev, stride, ref.lens, count, m, maxRecords)
    o.free()
    b = bytearray(dense)
    for k in range(count):
        word, = struct.unpack_from("<I", b, 16 + 4 * k)
        want = expect[k][0]
        assert word == want & ~STREAM_PARTIAL, "row %d: the case expects word %#x, the dense scan of the copy gives %#x" \
            % (k, want, word)
        struct.pack_into("<I", b, 16 + 4 * k, want)
    nxt = struct.pack("<%dI" % count, *[e[1] for e in expect])
    return bytes(b) + nxt + bytes(-len(nxt) % 16), ref, dense


def first_difference(got, want, count, maxRecords):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    nextAt = DN.records_offset(count) + maxRecords * REC
    part = ("next words (row %d)" % ((at - nextAt) // 4) if at >= nextAt else
            "info" if at < 16 else "row words (row %d)" % ((at - 16) // 4) if at < 16 + 4 * count else
            "starts" if at < 16 + 4 * (2 * count + 1) else "padding" if at < DN.records_offset(count) else
            "record %d" % ((at - DN.records_offset(count)) // REC))
    return "first difference at byte %d (%s): %r, expected %r" % (at, part, got[at:at + 8], want[at:at + 8])


def scan(L, ds, starts, ends, m, maxRecords):
    """(the output's bytes, Out) of one stream scan; starts / ends: device arrays or None."""
    o = Out(L, ds.count, maxRecords)
    t = L.sgpu_frames_scan_streams(ds.dev, ds.stride, starts, ends, ds.count, m, maxRecords, o.out)
    assert t > 0, "sgpu_frames_scan_streams returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return o.fetch(), o


def check_streams(L, layout, stride, m, starts=None, ends=None, maxRecords=None, ds=None):
    """One stream scan of the rows in `layout` (Row objects) against the
    expectation; starts / ends: lists, or None for a null array.  Returns (the
    output's bytes, the expectation per row)."""
    count = len(layout)
    rowBytes = [r.bytes() for r in layout]
    s = starts if starts is not None else [0] * count
    e = ends if ends is not None else [stride] * count
    expect = [layout[k].expect(s[k], e[k], m) for k in range(count)]
    if maxRecords is None:
        maxRecords = max(m, sum(w & PACKED_COUNT_MASK for w, _ in expect))
    want, ref, _ = expected_output(L, rowBytes, stride, s, e, expect, m, maxRecords)
    ref.free()
    own = ds is None
    if own:
        ds = DevStreams(L, rowBytes, stride)
    if starts is not None:
        ds.put(ds.starts, starts)
    if ends is not None:
        ds.put(ds.ends, ends)
    got, o = scan(L, ds, ds.starts if starts is not None else None, ds.ends if ends is not None else None, m,
                  maxRecords)
    o.free()
    if own:
        ds.free()
    assert got == want, "count %d, maxFrames %d, maxRecords %d: %s" % (count, m, maxRecords,
                                                                        first_difference(got, want, count, maxRecords))
    return got, expect


def all_ways(L, layout, stride, m, starts, ends):
    """The four combinations of null and given starts and ends.  The rows must be
    walkable from 0 and up to the stride as well."""
    for s in (starts, None):
        for e in (ends, None):
            check_streams(L, layout, stride, m, s, e)


# 1 -------------------------------------------------------------------------
def chunk_edge_rows(stride):
    """Frames at the edges of the chunks the walk stages: (rows, ends)."""
    rows = []
    # a frame whose first byte is 1..11 bytes before a chunk's end: its header straddles into the halo
    for d in range(1, 12):
        for kind, width in ((ORIGINAL, 1 + d % 4), (RECOVERY, 1 + (d + 1) % 4)):
            r = Row(stride).add(original(10 + d, CH - d - 3)).gap(3)
            assert r.at == CH - d
            r.add(original(100 + d, 40 + d, width) if kind == ORIGINAL else recovery(200 + d, 30 + d, width))
            rows.append(r.gap(d % 3).add(original(300 + d, 17)))
    # a frame that ends exactly at the chunk's end and one that starts there
    rows.append(Row(stride).add(recovery(1, 24)).add(original(2, CH - 24)).add(original(3, 33)).add(recovery(4, 6)))
    rows.append(Row(stride).to(CH - 9).add(original(5, 9)).add(recovery(6, 6)))
    # a frame of two chunks and five bytes: whole chunks are never loaded
    rows.append(Row(stride).gap(7).add(original(7, 2 * CH + 5, 2)).add(original(8, 12)).gap(2).add(recovery(9, 7)))
    rows.append(Row(stride).add(recovery(10, 2 * CH + 5, 3)).add(recovery(11, 9)))
    # a zero run that covers exactly one chunk, at the row's start and between two frames
    rows.append(Row(stride).gap(CH).add(original(12, 20)))
    rows.append(Row(stride).to(CH - 20).add(original(13, 20)).gap(CH).add(original(14, 20)))
    # a recovery frame whose tail lies in a later chunk than its header ...
    rows.append(Row(stride).to(CH - 20).add(recovery(15, 120)).add(original(16, 10)))
    rows.append(Row(stride).gap(5).add(recovery(17, CH + 100, 2)).add(original(18, 10)))
    # ... and whose last byte lies at each position of the 16-byte words around a chunk's end
    for e in range(-8, 17):
        rows.append(Row(stride).to(CH + e - 40).add(recovery(400 + e, 40)).gap(1).add(original(19, 11)))
    return rows, [r.at for r in rows]


def check_chunk_edges(path):
    L = load(path)
    stride = 4 * CH
    rows, ends = chunk_edge_rows(stride)
    for e in (ends, None):
        got, expect = check_streams(L, rows, stride, 8, None, e)
        assert all(1 <= w <= 4 and nxt == (stride if e is None else e[k]) for k, (w, nxt) in enumerate(expect))


# 2 -------------------------------------------------------------------------
def small_frames(stride, n, seed):
    """A row of n minimum frames back to back: 6-byte recovery frames and 9-byte originals."""
    rnd = random.Random(seed)
    r = Row(stride)
    for i in range(n):
        r.add(recovery(seed + i, 6) if rnd.randrange(2) else original(seed + i, 9))
    return r


def records_of(got, count, k):
    """Row k's records in a dense output all of whose rows are complete."""
    starts = struct.unpack_from("<%dI" % (count + 1), got, 16 + 4 * count)
    at = DN.records_offset(count)
    return got[at + REC * starts[k]:at + REC * starts[k + 1]]


def check_small_frames(path):
    """Chunks filled with minimum frames, the deepest chains; maxFrames reached in
    the middle of a chunk, and the rest of the row from the next word."""
    L = load(path)
    stride = 4 * CH
    # every frame of well-filled chunks
    rows = [small_frames(stride, 256, 40), small_frames(stride, 170, 41), Row(stride).gap(3), small_frames(stride, 1, 42)]
    rows[1].gap(CH // 2)
    for i in range(60):
        rows[1].add(original(900 + i, 9))
    got, expect = check_streams(L, rows, stride, 256, None, [r.at for r in rows])
    assert [w for w, _ in expect] == [256, 230, 0, 1]
    # more frames than maxFrames
    big = small_frames(stride, 300, 43)
    assert big.at > CH
    for m in (1, 2, 255, 256):
        got, expect = check_streams(L, [big, rows[1], big], stride, m, None, [big.at, rows[1].at, big.at])
        assert expect[0] == expect[2] == (m | PACKED_MORE, big.parts[m][0])
    # a second scan from the next word yields the rest: both together are one packed walk
    whole = small_frames(stride, 200, 44)
    dr = K.DevRows(L, [whole.bytes()], stride, [whole.at])
    raw = DN.packed_raw(L, dr.dev, stride, dr.lens, 1, 256)
    dr.free()
    assert DN.packed_words(raw, 1, 256) == [200]
    for m in (1, 2, 100, 199):
        first, e1 = check_streams(L, [whole], stride, m, None, [whole.at])
        assert e1[0] == (m | PACKED_MORE, whole.parts[m][0])
        rest, e2 = check_streams(L, [whole], stride, 256, [e1[0][1]], [whole.at])
        assert e2[0] == (200 - m, whole.at)
        assert records_of(first, 1, 0) + records_of(rest, 1, 0) == raw[:200 * REC]


# 3 -------------------------------------------------------------------------
def start_end_rows(stride):
    """(rows, starts, ends): every residue of start and of end around a 16-byte
    boundary, and the degenerate windows."""
    rows, starts, ends = [], [], []

    def add(r, s, e):
        rows.append(r)
        starts.append(s)
        ends.append(e)

    for res in range(16):
        # the walk starts at a frame that begins at 32 + res, behind frames an earlier scan consumed
        r = Row(stride).add(original(res, 20)).to(32 + res).add(recovery(50 + res, 21)).add(original(70 + res, 13))
        add(r, 32 + res, r.at)
        # ... and in the middle of the zero run before it
        r = Row(stride).add(original(res, 11)).to(40 + res).add(original(90 + res, 14))
        add(r, 12 + res, r.at)
        # the data ends at 64 + res: right behind a frame, and behind zeros
        r = Row(stride).add(original(res, 30)).to(64 + res - 9).add(original(110 + res, 9))
        add(r, 0, r.at)
        add(Row(stride).add(recovery(res, 25)).to(64 + res), 25, 64 + res)
    r = Row(stride).add(original(1, 20)).add(original(2, 20))
    add(r, 20, 20)            # start == end
    add(r, 0, 0)
    add(r, 40, 40)
    add(r, 41, 40)            # start past end
    add(r, stride + 1, 40)
    add(r, 0, stride + 16)    # end past the stride
    add(r, stride + 32, stride + 16)
    add(Row(stride).add(original(3, stride)), 0, stride)   # one frame fills the row
    return rows, starts, ends


def check_starts_and_ends(path):
    L = load(path)
    stride = 128
    rows, starts, ends = start_end_rows(stride)
    got, expect = check_streams(L, rows, stride, 4, starts, ends)
    bad = [k for k, (w, _) in enumerate(expect) if w == PACKED_MALFORMED]
    assert len(bad) == 4 and [expect[k][1] for k in bad] == [41, stride, 0, stride]
    # null arrays: start 0, end = stride (the rows walk from 0 and to the stride as well)
    ok = [k for k in range(len(rows)) if k not in bad]
    rows, starts, ends = [rows[k] for k in ok], [starts[k] for k in ok], [ends[k] for k in ok]
    all_ways(L, rows, stride, 4, starts, ends)


def check_row_counts(path, count):
    """The mix of starts and ends above, repeated to one row count."""
    L = load(path)
    stride = 128
    rows, starts, ends = start_end_rows(stride)
    pick = [(7 * k) % len(rows) for k in range(count)]
    rows, starts, ends = [rows[k] for k in pick], [starts[k] for k in pick], [ends[k] for k in pick]
    check_streams(L, rows, stride, 3, starts, ends)


# 4 -------------------------------------------------------------------------
def partial_rows(stride):
    """(rows, ends, what each row is): every way a row's last frame can be cut off,
    and the malformed frames, each behind two good frames."""
    rows, ends, what = [], [], []

    def lead():
        return Row(stride).add(original(len(rows), 19)).gap(len(rows) % 3).add(recovery(len(rows), 14))

    def cut(name, flag, data, left, never=None, total=None, good=True):
        r = lead()
        at = r.at
        r.add(data, good=good, never=never, total=total)
        rows.append(r)
        ends.append(at + left)
        what.append((name, flag))

    PART, BAD = STREAM_PARTIAL, PACKED_MALFORMED
    for w in (2, 3, 4):
        for left in range(1, w):
            cut("prefix of %d bytes cut to %d" % (w, left), PART, original(7, 40, w), left)
    for w in (1, 2, 3, 4):
        fr = original(8, 40, w)
        cut("body cut by one byte (w %d)" % w, PART, fr, len(fr) - 1)
        cut("cut right behind the prefix (w %d)" % w, PART, fr, w)
        cut("cut right behind the type byte (w %d)" % w, PART, fr, w + 1)
        cut("cut inside PacketNum (w %d)" % w, PART, fr, w + 6)
        cut("cut inside the flow (w %d)" % w, PART, recovery(9, 40, w), w + 2)
        # frames that can never become valid
        if w > 1:
            big = prefix(stride, w) + bytes([ORIGINAL, 1, 0, 0])
            cut("w + L above the stride, prefix whole (w %d)" % w, BAD, big, w, never=w, total=w + stride)
            cut("w + L above the stride, prefix cut (w %d)" % w, PART, big, w - 1, never=w, total=w + stride)
        for t in (2, 0xff):
            fr = prefix(30, w) + bytes([t, 1, 0, 0]) + payload(t, 26)
            cut("type %#x present (w %d)" % (t, w), BAD, fr, w + 1, never=w + 1, good=False)
            cut("type %#x not yet there (w %d)" % (t, w), PART, fr, w, never=w + 1, good=False)
            cut("type %#x, whole (w %d)" % (t, w), BAD, fr, len(fr), never=w + 1, good=False)
        for kind, inner in ((ORIGINAL, 7), (RECOVERY, 4)):
            fr = prefix(inner, w) + bytes([kind, 1, 0, 0, 9, 0, 0][:inner])
            cut("L == inner header of type %d, type present (w %d)" % (kind, w), BAD, fr, w + 1, never=w + 1, good=False)
            cut("L == inner header of type %d, type not there (w %d)" % (kind, w), PART, fr, w, never=w + 1, good=False)
            cut("L == inner header of type %d, whole (w %d)" % (kind, w), BAD, fr, len(fr), never=w + 1, good=False)
        fr = prefix(27, w) + bytes([ORIGINAL, 1, 0, 0, 0x00, 0x00, 0x40]) + payload(3, 20)
        cut("PacketNum above the maximum, all there (w %d)" % w, BAD, fr, w + 7, never=w + 7, good=False)
        cut("PacketNum above the maximum, two bytes there (w %d)" % w, PART, fr, w + 6, never=w + 7, good=False)
        cut("PacketNum above the maximum, whole (w %d)" % w, BAD, fr, len(fr), never=w + 7, good=False)
        if w > 1:
            cut("L == 0 in a wide prefix (w %d)" % w, BAD, prefix(0, w), w + 3, good=False)
    # a partial row between complete rows must not disturb them
    for k in range(len(rows), 0, -5):
        r = lead().add(original(k, 23))
        rows.insert(k, r)
        ends.insert(k, r.at)
        what.insert(k, ("complete", 0))
    return rows, ends, what


def check_partial_frames(path):
    L = load(path)
    stride = 256
    rows, ends, what = partial_rows(stride)
    got, expect = check_streams(L, rows, stride, 4, None, ends)
    for k, (w, nxt) in enumerate(expect):
        name, flag = what[k]
        if flag == 0:
            assert (w, nxt) == (3, ends[k]), name
        else:   # (the case's own statement of the outcome against Row.expect's)
            assert (w, nxt) == (2 | flag, rows[k].parts[2][0]), "%s: %#x" % (name, w)
    # the same rows behind a start that skips the first frame
    check_streams(L, rows, stride, 4, [19] * len(rows), ends)


# 5 -------------------------------------------------------------------------
def decoder_stats(L, dec):
    return DN.decoder_stats(L, dec)


def recv(L, decs, n, out, m, maxRecords, dev, stride, count, consumed=None):
    res = (C.c_int * maxRecords)(*([-1] * maxRecords))
    cons = (C.c_uint * count)(*(consumed if consumed is not None else [0xdeadbeef] * count))
    nrows, acc = C.c_uint(12345), C.c_uint(12345)
    r = L.sgpu_frames_recv_streams(decs, n, out, m, maxRecords, dev, stride, count, res, cons, C.byref(nrows),
                                   C.byref(acc))
    return r, list(res), list(cons), nrows.value, acc.value


def check_resume(path):
    """Three connections' streams arrive in pieces that cut frames anywhere.  Each
    round scans from the last round's next words: decoders A take
    sgpu_frames_recv_streams, decoders B sgpu_frames_recv_dense on the zeroed copy
    of the same round, decoders C sgpu_frames_recv on a host copy of the whole
    streams."""
    L = load(path)
    lengths = [30 + (i * 37) % 90 for i in range(10)]
    lost = {0: (1, 6), 1: (0,), 2: (3, 4, 8)}
    senders = [Sender(L, lengths, seed=270 + f) for f in range(3)]
    frames = [P.wire_frames(L, senders[f], f, [k for k in range(10) if k not in lost[f]], len(lost[f]) + 1)
              for f in range(3)]
    rnd = random.Random(61)
    stride, m = 3 * CH, 6
    # connection k carries flow k's frames, with gaps of 0..2 zero bytes
    layout = []
    for k in range(3):
        r = Row(stride)
        for fr in frames[k]:
            r.gap(rnd.randrange(3)).add(fr)
        layout.append(r)
    count = 3
    total = sum(len(r.parts) for r in layout)
    full = [r.bytes() for r in layout]
    lengthOf = [r.at for r in layout]
    assert max(lengthOf) > CH

    def decoders():
        return (C.c_void_p * 3)(*[L.sgpu_decoder_create() for _ in range(3)])

    decA, decB, decC = decoders(), decoders(), decoders()
    ds = DevStreams(L, [bytes(stride)] * count, stride)
    starts, ends = [0] * count, [0] * count
    accA = accB = rounds = partials = 0
    s0 = stats(L)
    while starts != lengthOf:
        rounds += 1
        assert rounds < 200
        # the transport appends a piece to every row
        for k in range(count):
            more = min(lengthOf[k] - ends[k], rnd.choice((1, 2, 3, 5, 17, 60, 200, CH)))
            if more:
                assert L.sgpu_h2d(ds.dev + k * stride + ends[k], full[k][ends[k]:ends[k] + more], more) == 0
            ends[k] += more
        have = [Row(stride) for _ in range(count)]
        for k in range(count):
            have[k].buf, have[k].parts = bytearray(full[k][:ends[k]]), layout[k].parts
        expect = [have[k].expect(starts[k], ends[k], m) for k in range(count)]
        maxRecords = count * m
        want, ref, dense = expected_output(L, [h.bytes() for h in have], stride, starts, ends, expect, m, maxRecords)
        ds.put(ds.starts, starts)
        ds.put(ds.ends, ends)
        got, o = scan(L, ds, ds.starts, ds.ends, m, maxRecords)
        assert got == want, "round %d: %s" % (rounds, first_difference(got, want, count, maxRecords))
        r, resA, consumed, nrows, n = recv(L, decA, 3, o.out, m, maxRecords, ds.dev, stride, count)
        # B: the dense scan's bytes of the zeroed copy, whose payloads lie where A's do
        po = DN.Out(L, count, maxRecords)
        C.memmove(po.out, dense, len(dense))
        rB, resB, nrowsB, nB = DN.recv(L, decB, po.out, m, maxRecords, ref.dev, stride, count)
        assert (r, resA, nrows, n) == (rB, resB, nrowsB, nB) and r == SUCCESS and nrows == count
        assert consumed == [e[1] for e in expect]
        partials += sum(1 for w, _ in expect if w & STREAM_PARTIAL)
        accA += n
        accB += nB
        assert L.sgpu_flush() == 0
        po.free()
        o.free()
        ref.free()
        starts = consumed
    assert stats(L)[STAT_STREAMS] - s0[STAT_STREAMS] == rounds * count
    assert accA == accB == total and partials > 5 and rounds > 5
    # C: the whole streams, from a host copy
    wire = b"".join(full)
    host = L.sgpu_host_alloc(len(wire))
    C.memmove(host, wire, len(wire))
    resC = (C.c_int * total)(*([-1] * total))
    nC = C.c_uint(0)
    assert L.sgpu_frames_recv(decC, 3, host, ds.dev, len(wire), resC, total, C.byref(nC)) == SUCCESS
    assert nC.value == total
    for f in range(3):
        for num in range(10):
            want = NEED_MORE if num in lost[f] else SUCCESS
            assert L.sgpu_decoder_has(decA[f], num) == L.sgpu_decoder_has(decB[f], num) == \
                L.sgpu_decoder_has(decC[f], num) == want
        assert decoder_stats(L, decA[f]) == decoder_stats(L, decB[f]) == decoder_stats(L, decC[f])
        for dec in (decA[f], decC[f]):
            out, k = C.c_void_p(), C.c_uint(0)
            assert L.sgpu_decoder_is_ready(dec) == SUCCESS
            assert L.sgpu_decode(dec, C.byref(out), C.byref(k)) == SUCCESS and k.value == len(lost[f])
        a, atail = K.delivered(L, decA[f], 10, 128)
        c, ctail = K.delivered(L, decC[f], 10, 128)
        assert a == c == senders[f].data and atail == ctail
    assert L.sgpu_flush() == 0
    for f in range(3):
        for d in (decA, decB, decC):
            L.sgpu_decoder_free(d[f])
    assert L.sgpu_flush() == 0
    L.sgpu_host_free(host)
    ds.free()
    for sn in senders:
        sn.free()


# 6 -------------------------------------------------------------------------
def check_cut(path):
    """Rows are all or nothing at maxRecords, and consumedOut is left untouched
    from *rowsOut on."""
    L = load(path)
    stride, m, count = 128, 4, 20
    rows = []
    for k in range(count):
        r = Row(stride)
        for j in range(1 + k % 4):
            r.gap(j).add(original(10 * k + j, 12 + j, flow=0))
        rows.append(r)
    rows[5].add(original(99, 40, flow=0))
    ends = [r.at for r in rows]
    ends[5] -= 7   # row 5 ends in a partial frame
    ds = DevStreams(L, [r.bytes() for r in rows], stride)
    ns = [1 + k % 4 for k in range(count)]
    for maxRecords in (m, 10, sum(ns[:6]), sum(ns[:6]) + 1, sum(ns)):
        got, expect = check_streams(L, rows, stride, m, None, ends, maxRecords=maxRecords, ds=ds)
        T, W, c, _ = struct.unpack_from("<4I", got, 0)
        starts = [sum(ns[:k]) for k in range(count + 1)]
        assert T == sum(ns) and c == max(k for k in range(count + 1) if starts[k] <= maxRecords) and W == starts[c]
        o = Out(L, count, maxRecords)
        C.memmove(o.out, got, len(got))
        dec = L.sgpu_decoder_create()
        r, res, consumed, nrows, n = recv(L, (C.c_void_p * 1)(dec), 1, o.out, m, maxRecords, ds.dev, stride, count)
        assert (r, nrows, n) == (SUCCESS, c, W)
        assert consumed[:c] == [e[1] for e in expect[:c]] and consumed[c:] == [0xdeadbeef] * (count - c)
        assert expect[5][0] == 2 | STREAM_PARTIAL
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
        o.free()
    assert L.sgpu_flush() == 0
    ds.free()


# 7 -------------------------------------------------------------------------
def check_arguments(path, gpu):
    """Every refusal with nothing queued and the counter unchanged; count == 0;
    the counter and the timing entries of the one scan that was queued."""
    L = load(path)
    stride, count, m = 64, 4, 2
    rows = [Row(stride).add(original(k, 19 + k, flow=0)).gap(3).add(original(10 + k, 12, flow=0)) for k in range(count)]
    ds = DevStreams(L, [r.bytes() for r in rows], stride)
    ds.put(ds.starts, [0] * count)
    ds.put(ds.ends, [r.at for r in rows])
    maxRecords = count * m
    o = Out(L, count, maxRecords)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    assert L.sgpu_flush() == 0
    s0 = stats(L)
    assert L.sgpu_frames_streams_bytes(3, 0) == 0 and L.sgpu_frames_streams_bytes(3, 3 * 256 + 1) == 0
    assert L.sgpu_frames_streams_next(3, 0) == 0 and L.sgpu_frames_streams_bytes(0, 1) == 0
    assert L.sgpu_frames_streams_next(3, 3 * 256) == 48 + 3 * 256 * 32
    assert [L.sgpu_frames_streams_bytes(n, 256) - L.sgpu_frames_streams_next(n, 256) for n in (1, 4, 5, 8, 9)] == \
        [16, 16, 32, 32, 48]

    def scan_args(**kw):
        a = dict(rows=ds.dev, stride=stride, starts=ds.starts, ends=ds.ends, count=count, m=m, r=maxRecords, out=o.out)
        a.update(kw)
        return L.sgpu_frames_scan_streams(a["rows"], a["stride"], a["starts"], a["ends"], a["count"], a["m"], a["r"],
                                          a["out"])

    rowArgs = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=ds.dev + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=72)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("maxFrames zero", dict(m=0)),
        ("maxFrames above 256", dict(m=257, r=4 * 257)),
        ("maxRecords below maxFrames", dict(r=m - 1)),
        ("maxRecords zero", dict(r=0)),
        ("maxRecords above count * maxFrames", dict(r=count * m + 1)),
    ]
    for what, kw in rowArgs + [("null output", dict(out=None)), ("output not 16-byte aligned", dict(out=o.out + 8)),
                               ("starts not 4-byte aligned", dict(starts=ds.starts + 2)),
                               ("ends not 4-byte aligned", dict(ends=ds.ends + 1)),
                               ("a packed output above 4 GiB", dict(count=1 << 19, m=256, r=256)),
                               ("an output of 4 GiB", dict(count=119304647, m=1, r=119304647))]:
        assert scan_args(**kw) == -1, what
    assert L.sgpu_flush() == 0
    assert o.untouched()
    s1 = stats(L)
    assert [s1[i] for i in (0, 1, STAT_STREAMS, DN.STAT_DENSE, P.STAT_WALKS)] == \
        [s0[i] for i in (0, 1, STAT_STREAMS, DN.STAT_DENSE, P.STAT_WALKS)]

    L.sgpu_timing(1, 1, None, None)
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_STREAMWALK] > 0 and ms[TIMING_ROWSUM] > 0 and ms[TIMING_COMPACT] > 0
        assert ms[8] == 0 and ms[7] == 0, "the stream walk has its own entry"
    got = o.fetch()
    expect = [r.expect(0, r.at, m) for r in rows]
    want, ref, _ = expected_output(L, [r.bytes() for r in rows], stride, [0] * count, [r.at for r in rows], expect, m,
                                   maxRecords)
    ref.free()
    assert got == want
    s2 = stats(L)
    assert s2[STAT_STREAMS] - s1[STAT_STREAMS] == count, "only the one valid scan was counted"
    assert s2[DN.STAT_DENSE] - s1[DN.STAT_DENSE] == count, "(the reference scan of this case)"

    def recv_args(**kw):
        a = dict(decs=decs, heads=o.out, rows=ds.dev, stride=stride, count=count, m=m, r=maxRecords, rowsOut=True,
                 consumed=True)
        a.update(kw)
        n, nrows = C.c_uint(99), C.c_uint(99)
        res = (C.c_int * maxRecords)(*([-1] * maxRecords))
        cons = (C.c_uint * count)(*([77] * count))
        r = L.sgpu_frames_recv_streams(a["decs"], 1, a["heads"], a["m"], a["r"], a["rows"], a["stride"], a["count"],
                                       res, cons if a["consumed"] else None,
                                       C.byref(nrows) if a["rowsOut"] else None, C.byref(n))
        return r, n.value, nrows.value if a["rowsOut"] else 0, list(res), list(cons)

    for what, kw in rowArgs + [("null decoders", dict(decs=None)), ("null output", dict(heads=None)),
                               ("output not 4-byte aligned", dict(heads=o.out + 2)),
                               ("null rowsOut", dict(rowsOut=False)), ("null consumedOut", dict(consumed=False))]:
        assert recv_args(**kw) == (INVALID, 0, 0, [-1] * maxRecords, [77] * count), what
    for k in range(count):
        assert L.sgpu_decoder_has(dec, k) == NEED_MORE, "a refused call must not reach the decoder"

    # count == 0: a ticket that is complete, nothing scanned, nothing written; nothing accepted
    before = C.string_at(o.base, o.bytes)
    for kw in (dict(count=0), dict(count=0, r=0), dict(count=0, rows=None, starts=None, ends=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    assert recv_args(count=0)[:3] == (SUCCESS, 0, 0)
    assert recv_args(count=0, decs=None, heads=None, rows=None, consumed=False)[:3] == (SUCCESS, 0, 0)
    assert L.sgpu_flush() == 0
    s3 = stats(L)
    assert (s3[0], s3[1], s3[STAT_STREAMS]) == (s2[0], s2[1], s2[STAT_STREAMS]), "nothing was queued by any of them"
    assert C.string_at(o.base, o.bytes) == before

    # (the arguments were fine otherwise)
    assert recv_args() == (SUCCESS, maxRecords, count, [SUCCESS] * maxRecords, [r.at for r in rows])
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    ds.free()


# 8 (the CPU double only) ----------------------------------------------------
def check_forged(path):
    """The output is caller data: a next word above the stride or below the end
    of its row's last record stops the routing at that row, as a start that fails
    does (streams_forged_test.cpp runs these and the dense forgeries under the
    sanitizers)."""
    L = load(path)
    stride, m, count = 128, 2, 6
    rows = [Row(stride).add(original(50 + k, 19 + k, flow=0)).gap(1 + k).add(original(150 + k, 19 + k, flow=0))
            for k in range(count)]
    ds = DevStreams(L, [r.bytes() for r in rows], stride)
    ds.put(ds.ends, [r.at for r in rows])
    maxRecords = count * m
    good, o = scan(L, ds, None, ds.ends, m, maxRecords)
    nextAt = o.next
    startAt = 16 + 4 * count

    def word(at, v):
        return lambda b: b.__setitem__(slice(at, at + 4), struct.pack("<I", v))

    cases = [
        ("nothing forged", lambda b: None, SUCCESS, count, maxRecords),
        ("a next word above the stride", word(nextAt + 4 * 2, stride + 1), INVALID, 2, 4),
        ("a huge next word", word(nextAt, 0xffffffff), INVALID, 0, 0),
        ("a next word below the end of the row's last record", word(nextAt + 4 * 3, rows[3].at - 1), INVALID, 3, 6),
        ("a next word of zero behind records", word(nextAt + 4 * 5, 0), INVALID, 5, 10),
        ("a next word at the stride", word(nextAt + 4 * 4, stride), SUCCESS, count, maxRecords),
        ("decreasing starts", word(startAt + 4 * 3, 3), INVALID, 2, 4),
        ("a partial bit on a complete row", word(16 + 4, 2 | STREAM_PARTIAL), SUCCESS, count, maxRecords),
        ("c > count", word(8, count + 1), INVALID, 0, 0),
    ]
    for what, forge, result, rowsDone, accepted in cases:
        b = bytearray(good)
        forge(b)
        C.memmove(o.out, bytes(b), len(b))
        dec = L.sgpu_decoder_create()
        r, res, consumed, nrows, n = recv(L, (C.c_void_p * 1)(dec), 1, o.out, m, maxRecords, ds.dev, stride, count)
        assert (r, nrows, n) == (result, rowsDone, accepted), "%s: %r" % (what, (r, nrows, n))
        nxt = struct.unpack_from("<%dI" % count, b, nextAt)
        assert consumed == list(nxt[:rowsDone]) + [0xdeadbeef] * (count - rowsDone), what
        for k in range(count):
            want = SUCCESS if k < rowsDone else NEED_MORE
            assert L.sgpu_decoder_has(dec, 50 + k) == L.sgpu_decoder_has(dec, 150 + k) == want, what
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    ds.free()
