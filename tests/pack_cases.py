"""sgpu_frames_scan_packed / sgpu_frames_recv_packed / sgpu_encoder_pack_frames:
the cases shared by test_pack_cpu.py (the CPU test double, tests/hostsim) and
test_pack_gpu.py (k_walk and k_frame on the MI355X), driven through the C ABI
with ctypes.

Expected records come from sgpu_frames_parse over row[:end] and plain slices
of the bytes a case put into the rows (expected_row); expected decoder state
comes from sgpu_frames_recv over a host copy of the same rows; the packer's
layout from a model of its rule (model_layout).  Every scan writes between two
guard records pre-filled with 0xA5, and host-built rows lie in a device
allocation of exactly count * stride bytes, so the last row ends where the
allocation ends.
"""
import ctypes as C
import random

import deliver_cases as D
import frame_cases as F
import scan_cases as K
from deliver_cases import FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, PENDING, SUCCESS, Rec, Rows, payload
from frame_cases import ORIGINAL, RECOVERY, Sender, header
from scan_cases import DevRows
from siamese_amd.binding import (PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, ROW_OK, PackedHead,
                                 bind_packed_abi)

STAT_FRAMES = 22
STAT_WALKS = 24
NSTATS = 25
REC = C.sizeof(PackedHead)
PARSE_MAX = 512


def load(path):
    L = K.load(path)
    if getattr(L, "_pack_cases", False):
        return L
    # (the four symbols under test: an AttributeError here is the parent's answer)
    bind_packed_abi(L)
    L._pack_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


def parse(L, raw):
    """(result, frames) of sgpu_frames_parse over raw."""
    out = (K.Frame * PARSE_MAX)()
    n = C.c_uint(0)
    r = L.sgpu_frames_parse(raw, len(raw), out, PARSE_MAX, C.byref(n))
    assert n.value < PARSE_MAX
    return r, [out[k] for k in range(n.value)]


def fields(h):
    return (h.Offset, h.Status, h.Type, h.HeaderBytes, h.TailBytes, h.Flow, h.PacketNum, h.DataBytes,
            bytes(h.Head), bytes(h.Tail))


ZERO = (0, 0, 0, 0, 0, 0, 0, 0, bytes(4), bytes(8))


def expected_row(L, row, stride, length, maxFrames):
    """(records, row word) of one row: length = its length word, None without."""
    end = stride if length is None else length
    if end > stride:
        return [ZERO] * maxFrames, PACKED_MALFORMED
    raw = row[:end]
    r, fr = parse(L, raw) if end else (SUCCESS, [])
    recs, flags, at = [], 0, 0
    for f in fr + ([None] if r != SUCCESS else []):
        if len(recs) == maxFrames:
            flags = PACKED_MORE
            break
        if f is None or (f.Type == ORIGINAL and f.PacketNum > PACKET_NUM_MAX):
            flags = PACKED_MALFORMED
            break
        while raw[at] == 0:   # the zero bytes before the frame
            at += 1
        data = raw[f.Offset:f.Offset + f.Bytes]
        if f.Type == ORIGINAL:
            recs.append((at, ROW_OK, ORIGINAL, f.Offset - at, 0, f.Flow, f.PacketNum, f.Bytes, bytes(4), bytes(8)))
        else:
            t = min(8, f.Bytes)
            recs.append((at, ROW_OK, RECOVERY, f.Offset - at, t, f.Flow, 0, f.Bytes,
                         data[:4] + bytes(4 - len(data[:4])), bytes(8 - t) + data[len(data) - t:]))
        at = f.Offset + f.Bytes
    return recs + [ZERO] * (maxFrames - len(recs)), len(recs) | flags


class Out:
    """A packed scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxFrames):
        self.L, self.count, self.maxFrames = L, count, maxFrames
        self.total = L.sgpu_frames_packed_bytes(count, maxFrames)
        assert self.total == count * maxFrames * REC + 4 * count
        self.bytes = self.total + 2 * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        """(records of each row as field tuples, row words), guards checked."""
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the records was written"
        assert raw[-REC:] == guard, "guard record after the row words was written"
        m = self.maxFrames
        recs = [[fields(PackedHead.from_buffer_copy(raw, REC * (1 + k * m + j))) for j in range(m)]
                for k in range(self.count)]
        w0 = REC * (1 + self.count * m)
        words = [int.from_bytes(raw[w0 + 4 * k:w0 + 4 * k + 4], "little") for k in range(self.count)]
        return recs, words

    def untouched(self):
        return C.string_at(self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_host_free(self.base)


def scan(L, dev, stride, lens, count, maxFrames):
    o = Out(L, count, maxFrames)
    t = L.sgpu_frames_scan_packed(dev, stride, lens, count, maxFrames, o.out)
    assert t > 0, "sgpu_frames_scan_packed returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    recs, words = o.fetch()
    return recs, words, o


def check_packed(L, rows, stride, lens, maxFrames):
    """Scan host-built rows with and without their lengths, against
    expected_row; returns the expectation with lengths."""
    dr = DevRows(L, rows, stride, lens)
    first = None
    for lp in (dr.lens, None):
        want = [expected_row(L, rows[k], stride, lens[k] if lp else None, maxFrames) for k in range(len(rows))]
        recs, words, o = scan(L, dr.dev, stride, lp, len(rows), maxFrames)
        for k in range(len(rows)):
            how = "row %d (%s lengths)" % (k, "with" if lp else "without")
            assert words[k] == want[k][1], "%s: word %#x, expected %#x" % (how, words[k], want[k][1])
            assert recs[k] == want[k][0], "%s: %r, expected %r" % (how, recs[k], want[k][0])
        o.free()
        first = first or want
    dr.free()
    return first


def prefix(length, width):
    """The length prefix of `length` in `width` bytes (wider than needed is allowed)."""
    if width == 1:
        assert length < 0x80
        return bytes([length])
    if width == 2:
        assert length < 0x4000
        return bytes([0x80 | (length >> 8), length & 0xff])
    if width == 3:
        assert length < 0x200000
        return bytes([0xC0 | (length >> 16), (length >> 8) & 0xff, length & 0xff])
    return bytes([0xE0 | (length >> 24), (length >> 16) & 0xff, (length >> 8) & 0xff, length & 0xff])


def frame(kind, flow, num, data, width=1):
    inner = bytes([kind]) + flow.to_bytes(3, "little") + (num.to_bytes(3, "little") if kind == ORIGINAL else b"")
    return prefix(len(inner) + len(data), width) + inner + data


def row_of(parts, stride):
    """(row, end of the last part): parts are bytes, or an int for a zero gap."""
    b = b"".join(bytes(p) if isinstance(p, int) else p for p in parts)
    assert len(b) <= stride, "%d bytes in a row of %d" % (len(b), stride)
    return b + bytes(stride - len(b)), len(b)


# 1 -------------------------------------------------------------------------
def check_header_offsets(path):
    """A second frame of each type at each offset 16..31 behind a first one,
    with prefixes of 1 and 2 bytes and wider ones than the L needs: headers of
    8..11 bytes that lie inside one aligned word, straddle two, or start in
    the first word's last bytes."""
    L = load(path)
    stride = 128
    first = frame(ORIGINAL, 0x030201, 9, payload(1, 5))
    assert len(first) == 13 and first == header(L, ORIGINAL, 0x030201, 9, 5) + payload(1, 5)
    rows, lens = [], []
    for kind in (ORIGINAL, RECOVERY):
        for off in range(16, 32):
            for width in (1, 2, 3, 4):
                second = frame(kind, 0xABCDEF - off, 1000 + off, payload(10 * off + width, 20 + width), width)
                row, end = row_of([first, off - len(first), second], stride)
                rows.append(row)
                lens.append(end)
    # a frame that ends exactly at the stride, in the last row of the allocation
    n = stride - 16 - 9
    last = frame(ORIGINAL, 7, 77, payload(3, n), 2)
    row, end = row_of([first, 3, last], stride)
    assert end == stride
    rows.append(row)
    lens.append(end)
    want = check_packed(L, rows, stride, lens, 3)
    assert all(w[1] == 2 for w in want)
    assert {w[0][1][3] for w in want} == {5, 6, 7, 8, 9, 10, 11}, "every header width"
    assert {w[0][1][0] for w in want} == set(range(16, 32))


# 2 -------------------------------------------------------------------------
TAIL_D = list(range(1, 10)) + [24]


def check_recovery_tails(path):
    """Recovery frames of D = 1..9 and 24 bytes whose last byte lies at each of
    the 16 positions of an aligned word, in a middle word and in the row's
    last word."""
    L = load(path)
    stride = 64
    first = frame(ORIGINAL, 1, 2, payload(4, 5))
    rows, lens = [], []
    for base in (32, 48):
        for d in TAIL_D:
            for e in list(range(1, 16)) + [16]:
                end = base + e
                start = end - 5 - d
                parts = [first, start - len(first)] if start >= 16 else [start]
                row, used = row_of(parts + [frame(RECOVERY, 0x00FACE, 0, payload(100 * d + e, d))], stride)
                assert used == end
                rows.append(row)
                lens.append(end)
    assert lens[-1] == stride
    want = check_packed(L, rows, stride, lens, 2)
    assert {w[0][w[1] - 1][4] for w in want} == set(range(1, 9))


# 3 -------------------------------------------------------------------------
def check_gaps(path):
    L = load(path)
    stride = 256
    a = frame(ORIGINAL, 5, 50, payload(5, 21))
    b = frame(RECOVERY, 5, 0, payload(6, 33))
    c = frame(ORIGINAL, 6, 51, payload(7, 3))
    rows, lens = [], []
    for gap in (1, 15, 16, 17, 100):
        row, end = row_of([a, gap, b, min(gap, 17), c], stride)
        rows.append(row)
        lens.append(end)
    # leading zeros, then frames
    row, end = row_of([37, a, b], stride)
    rows.append(row)
    lens.append(end)
    # all zero, with and without a length
    rows += [bytes(stride), bytes(stride)]
    lens += [stride, 0]
    # a zero length over stale frames
    row, end = row_of([a, b, c], stride)
    rows.append(row)
    lens.append(0)
    # lengths shorter than the content: at the end of the first frame, in the gap after it, at the second's end
    for cut in (len(a), len(a) + 2, len(a) + 3 + len(b)):
        row, end = row_of([a, 3, b, 5, c], stride)
        rows.append(row)
        lens.append(cut)
    want = check_packed(L, rows, stride, lens, 4)
    assert [w[1] for w in want] == [3] * 5 + [2, 0, 0, 0, 1, 1, 2]


# 4 -------------------------------------------------------------------------
def check_max_frames(path):
    L = load(path)
    stride, m = 128, 4
    fr = [frame(ORIGINAL, 2, k, payload(40 + k, 2 + k)) for k in range(m + 1)]
    rows, lens = [], []
    for n in (m - 1, m, m + 1):
        row, end = row_of(fr[:n], stride)
        rows.append(row)
        lens.append(end)
    # maxFrames frames and then zeros only, inside the length
    row, end = row_of(fr[:m] + [20], stride)
    rows.append(row)
    lens.append(end)
    # ... and a single non-zero byte far behind them
    row, end = row_of(fr[:m] + [40, b"\x01"], stride)
    rows.append(row)
    lens.append(end)
    want = check_packed(L, rows, stride, lens, m)
    assert [w[1] for w in want] == [m - 1, m, m | PACKED_MORE, m, m | PACKED_MORE]

    # maxFrames == 1 on rows of one frame: sgpu_frames_scan_rows' record, but for Offset / FrameBytes
    singles = [K.frame_row(L, kind, 9 + i, i, payload(60 + i, n), stride)
               for i, (kind, n) in enumerate([(ORIGINAL, 1), (RECOVERY, 3), (RECOVERY, 9), (ORIGINAL, 100)])]
    dr = DevRows(L, [r for r, _ in singles], stride, [n for _, n in singles])
    for lp in (dr.lens, None):
        one, hd = K.scan(L, dr.dev, stride, lp, len(singles))
        recs, words, o = scan(L, dr.dev, stride, lp, len(singles), 1)
        assert words == [1] * len(singles)
        for k in range(len(singles)):
            assert recs[k][0][0] == 0 and recs[k][0][1:] == one[k][1:]
        hd.free()
        o.free()
    dr.free()


# 5 -------------------------------------------------------------------------
def check_malformed(path):
    """Each way a frame can be malformed, as the third frame of a row between
    good rows: the two frames before it are reported, the flag is set and the
    neighbours are exact."""
    L = load(path)
    stride, m = 128, 4
    fill = payload(499, 40)
    a = frame(ORIGINAL, 0, 10, payload(8, 11))
    b = frame(RECOVERY, 0, 0, payload(9, 17))
    lead = [a, 2, b, 1]
    at = len(a) + 2 + len(b) + 1
    whole = frame(ORIGINAL, 0, 12, fill[:20])
    # (third frame's bytes, the row's length word or None for "where the bytes end")
    bad = [
        (bytes([0x80, 0x00, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20], None),          # L = 0 behind a wide prefix
        (bytes([0xE0, 0x00, 0x00, 0x00, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20], None),
        (bytes([24, 2, 0, 0, 0]) + fill[:20], None),                                 # type 2
        (bytes([7, ORIGINAL, 0, 0, 0, 99, 0, 0]), None),                              # L <= inner header
        (bytes([4, RECOVERY, 0, 0, 0]), None),
        (bytes([1, ORIGINAL]), None),
        (bytes([27, ORIGINAL, 0, 0, 0, 0x00, 0x00, 0x40]) + fill[:20], None),         # PacketNum too large
        (whole, at + len(whole) - 1),                                                # the frame crosses end
        (bytes([60, RECOVERY, 0, 0, 0]) + fill[:30], None),                           # ... its L says so
        (frame(ORIGINAL, 0, 13, fill[:20], 2), at + 1),                               # the prefix is cut by end
        (frame(ORIGINAL, 0, 13, fill[:20], 4), at + 3),
    ]
    rows, lens, isBad = [], [], []

    def good(i):
        row, end = row_of([frame(ORIGINAL, 0, 100 + i, payload(400 + i, 5 + i)), i % 5,
                           frame(ORIGINAL, 0, 200 + i, payload(450 + i, 30 - i))], stride)
        rows.append(row)
        lens.append(end)
        isBad.append(False)

    for i, (third, length) in enumerate(bad):
        good(i)
        row, end = row_of(lead + [third], stride)
        rows.append(row)
        lens.append(end if length is None else length)
        isBad.append(True)
    good(len(bad))
    # a length word above the stride: no records at all
    rows.append(row_of(lead, stride)[0])
    lens.append(stride + 1)
    isBad.append(True)
    good(len(bad) + 1)
    want = check_packed(L, rows, stride, lens, m)
    for k, w in enumerate(want):
        if not isBad[k]:
            assert w[1] == 2, "good row %d" % k
        elif lens[k] > stride:
            assert w[1] == PACKED_MALFORMED
        else:
            assert w[1] == 2 | PACKED_MALFORMED, "bad row %d: %#x" % (k, w[1])
            assert [r[0] for r in w[0][:2]] == [0, len(a) + 2]

    # routing: the good frames of every row reach the decoder, the call reports the bad ones
    count = len(rows)
    dr = DevRows(L, rows, stride, lens)
    recs, words, o = scan(L, dr.dev, stride, dr.lens, count, m)
    dec = L.sgpu_decoder_create()
    results = (C.c_int * (count * m))(*([-1] * (count * m)))
    n = C.c_uint(99)
    assert L.sgpu_frames_recv_packed((C.c_void_p * 1)(dec), 1, o.out, m, dr.dev, stride, count, results,
                                     C.byref(n)) == INVALID
    res = [list(results[k * m:(k + 1) * m]) for k in range(count)]
    # (the same original 10 and recovery packet in every bad row: the first is new, the rest duplicates or refused
    # alike; what matters here is which slots were used)
    for k in range(count):
        if not isBad[k]:
            assert res[k] == [SUCCESS, SUCCESS, NEED_MORE, NEED_MORE], "row %d: %r" % (k, res[k])
        elif lens[k] > stride:
            assert res[k] == [INVALID, NEED_MORE, NEED_MORE, NEED_MORE]
        else:
            assert res[k][2:] == [INVALID, NEED_MORE] and NEED_MORE not in res[k][:2], "row %d: %r" % (k, res[k])
    for k in range(count):
        if not isBad[k]:
            for r in want[k][0][:2]:
                assert L.sgpu_decoder_has(dec, r[6]) == SUCCESS
    assert L.sgpu_decoder_has(dec, 10) == SUCCESS
    for num in (1, 12, 13, 99):
        assert L.sgpu_decoder_has(dec, num) == NEED_MORE
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    dr.free()


# 6 -------------------------------------------------------------------------
def wire_frames(L, sn, flow, nums, nrec, stride=512):
    """The frames of a sender as bytes: originals `nums`, then nrec recovery packets."""
    rows = Rows(L, len(nums) + nrec, stride)
    for i, num in enumerate(nums):
        res, queued = F.originals(L, sn.enc, num, 1, flow, rows, dst=rows.dst + i * stride, lens=rows.lens + 4 * i)
        assert res == [SUCCESS] and queued == 1
    at = len(nums)
    recs = sn.encode(nrec)
    assert F.recovery(L, recs, nrec, [flow] * nrec, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at) == nrec
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    rows.free()
    return [got[k][:lens[k]] for k in range(len(got))]


def check_parity_routing(path):
    """Three flows' originals and recovery packets packed by hand, several to a
    row at odd offsets: decoders A through a host copy and sgpu_frames_recv, B
    through scan_packed -> recv_packed.  Flow 3 has no decoder, flow 4's has a
    matrix job pending."""
    L = load(path)
    stride, m = 512, 16
    lengths = [30 + (i * 37) % 90 for i in range(10)]
    lost = {0: (1, 6), 1: (0,), 2: (3, 4, 8)}
    senders = [Sender(L, lengths, seed=70 + f) for f in range(5)]
    frames = []
    for f in range(5):
        gone = lost.get(f, ())
        frames.append(wire_frames(L, senders[f], f, [k for k in range(10) if k not in gone], len(gone) + 1))
    # interleave the flows frame by frame, pack with gaps of 0..5 bytes
    order = []
    for i in range(max(len(x) for x in frames)):
        order += [x[i] for x in frames if i < len(x)]
    rnd = random.Random(6)
    rows, lens, parts = [], [], []
    for fr in order:
        gap = rnd.randrange(6)
        if sum(p if isinstance(p, int) else len(p) for p in parts) + gap + len(fr) > stride:
            row, end = row_of(parts, stride)
            rows.append(row)
            lens.append(end)
            parts = []
        parts += [gap, fr]
    row, end = row_of(parts, stride)
    rows.append(row)
    lens.append(end)
    count = len(rows)
    assert count >= 4
    dr = DevRows(L, rows, stride, lens)

    # flow 4's decoder: a matrix job pending from its own earlier packets
    busy = D.Stream(L, D.REC_LENGTHS, lost=D.REC_LOST, recovery=4, seed=22)
    r, _ = busy.decode(device=True)
    assert r == PENDING

    def decoders():
        return (C.c_void_p * 5)(L.sgpu_decoder_create(), L.sgpu_decoder_create(), L.sgpu_decoder_create(), None,
                                busy.dec)

    # A: the host copy
    wire = b"".join(rows)
    host = L.sgpu_host_alloc(len(wire))
    C.memmove(host, wire, len(wire))
    decA = decoders()
    resA = (C.c_int * len(order))(*([-1] * len(order)))
    nA = C.c_uint(0)
    assert L.sgpu_frames_recv(decA, 5, host, dr.dev, len(wire), resA, len(order), C.byref(nA)) == INVALID
    assert nA.value == len(order)

    # B: the records
    decB = decoders()
    s0 = stats(L)
    recs, words, o = scan(L, dr.dev, stride, dr.lens, count, m)
    assert stats(L)[STAT_WALKS] - s0[STAT_WALKS] == count
    assert sum(words) == len(order) and max(words) <= m
    resB = (C.c_int * (count * m))(*([-1] * (count * m)))
    nB = C.c_uint(0)
    assert L.sgpu_frames_recv_packed(decB, 5, o.out, m, dr.dev, stride, count, resB, C.byref(nB)) == INVALID
    flat = []
    for k in range(count):
        slot = list(resB[k * m:(k + 1) * m])
        assert slot[words[k]:] == [NEED_MORE] * (m - words[k]), "unused slots of row %d" % k
        flat += slot[:words[k]]
    assert flat == list(resA)
    flows = [r[5] for k in range(count) for r in recs[k][:words[k]]]
    assert flat == [INVALID if f >= 3 else SUCCESS for f in flows]
    assert nB.value == sum(1 for f in flows if f < 3)

    for f in range(3):
        for num in range(10):
            want = NEED_MORE if num in lost[f] else SUCCESS
            assert L.sgpu_decoder_has(decA[f], num) == L.sgpu_decoder_has(decB[f], num) == want
        for dec in (decA[f], decB[f]):
            out, k = C.c_void_p(), C.c_uint(0)
            assert L.sgpu_decoder_is_ready(dec) == SUCCESS
            assert L.sgpu_decode(dec, C.byref(out), C.byref(k)) == SUCCESS and k.value == len(lost[f])
        a, atail = K.delivered(L, decA[f], 10, 128)
        b, btail = K.delivered(L, decB[f], 10, 128)
        assert a == b == senders[f].data and atail == btail
    # the pending job was not disturbed
    assert L.sgpu_flush() == 0
    assert busy.decode(device=True) == (SUCCESS, len(D.REC_LOST))
    for f in range(3):
        L.sgpu_decoder_free(decA[f])
        L.sgpu_decoder_free(decB[f])
    assert L.sgpu_flush() == 0
    busy.free()
    L.sgpu_host_free(host)
    o.free()
    dr.free()
    for sn in senders:
        sn.free()


# 7 -------------------------------------------------------------------------
def model_layout(sizes, stride):
    """The packer's rule: [(row, off)] of frames of `sizes` bytes, rows used, each row's length."""
    row = off = 0
    at, ends = [], {}
    for t in sizes:
        assert t <= stride
        if off + t > stride:
            row, off = row + 1, 0
        at.append((row, off))
        ends[row] = off + t
        off = (off + t + 15) & ~15
    return at, (row + 1 if sizes else 0), ends


def pack(L, enc, flow, first, count, recs, nrec, rows, maxRows, stride=None, want=SUCCESS):
    res = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    nrows, nframes = C.c_uint(12345), C.c_uint(12345)
    r = L.sgpu_encoder_pack_frames(enc, flow, first, count, recs, nrec, rows.dst, rows.stride if stride is None else stride,
                                   maxRows, rows.lens, res, C.byref(nrows), C.byref(nframes))
    assert r == want, "sgpu_encoder_pack_frames returned %d, expected %d" % (r, want)
    return list(res)[:count], nrows.value, nframes.value


def packed_and_checked(L, sn, lengths, flow, recs, nrec, stride, spare=2):
    """Pack a sender's originals and recovery packets, compare every byte with
    the layout rule's; returns (rows, maxRows, sizes, need)."""
    want = [header(L, ORIGINAL, flow, k, len(d)) + d for k, d in enumerate(sn.data)]
    recBytes = [recs[k].DataBytes for k in range(nrec)]
    sizes = [len(w) for w in want] + [5 + n for n in recBytes]
    at, need, ends = model_layout(sizes, stride)
    maxRows = need + spare
    rows = Rows(L, maxRows, stride)

    # one row short: nothing written, the rows needed reported
    s0 = stats(L)
    res, nrows, nframes = pack(L, sn.enc, flow, 0, len(lengths), recs, nrec, rows, need - 1, want=INVALID)
    assert (nrows, nframes) == (need, 0)
    assert L.sgpu_flush() == 0
    assert rows.untouched() and stats(L)[STAT_FRAMES] == s0[STAT_FRAMES]

    res, nrows, nframes = pack(L, sn.enc, flow, 0, len(lengths), recs, nrec, rows, maxRows)
    assert res == [SUCCESS] * len(lengths) and (nrows, nframes) == (need, len(sizes))
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_FRAMES] - s0[STAT_FRAMES] == len(sizes) + maxRows - need
    got, lens = rows.fetch()   # (the guard rows and words)
    assert lens == [ends[r] for r in range(need)] + [0] * (maxRows - need)
    for r in range(need, maxRows):
        assert got[r] == bytes([FILL]) * stride, "row %d past the rows used was written" % r
    # the recovery packets' bytes, from the library's older way out
    recData = [D.read(L, recs[k].DeviceData, recBytes[k]) for k in range(nrec)]
    frames = want + [header(L, RECOVERY, flow, 0, len(d)) + d for d in recData]
    model = [bytearray(stride) for _ in range(need)]
    for (r, off), fr in zip(at, frames):
        model[r][off:off + len(fr)] = fr
    for r in range(need):
        assert got[r] == bytes(model[r]), "row %d differs from the layout rule's" % r
    # the whole buffer is a frame stream
    r, fr = parse(L, b"".join(got[:need]))
    assert r == SUCCESS and len(fr) == len(frames)
    assert [(f.Type, f.Flow, f.PacketNum, f.Bytes) for f in fr] == \
        [(ORIGINAL, flow, k, n) for k, n in enumerate(lengths)] + [(RECOVERY, flow, 0, n) for n in recBytes]
    # ... and input for the packed scan
    recsOut, words, o = scan(L, rows.dst, stride, rows.lens, maxRows, 16)
    wantScan = [expected_row(L, got[k], stride, lens[k], 16) for k in range(maxRows)]
    assert (recsOut, words) == ([w[0] for w in wantScan], [w[1] for w in wantScan])
    assert sum(words) == len(frames) and words[need:] == [0] * (maxRows - need)
    o.free()
    return rows, maxRows, sizes, need


def check_packer(path):
    L = load(path)
    stride = 256
    # frame sizes T = 8 + n (9 + n from n = 121): T = 0, 1, 15 (mod 16), a frame of exactly the stride, small ones
    lengths = [24, 25, 39, 8, 40, stride - 9, 23, 57, 120, 121, 1, 72, 9, 200, 30, 31]
    sn = Sender(L, lengths, seed=81)
    sizes = [len(header(L, ORIGINAL, 0x00BEEF, k, n)) + n for k, n in enumerate(lengths)]
    assert {t % 16 for t in sizes} >= {0, 1, 15} and stride in sizes
    rows, maxRows, sizes, need = packed_and_checked(L, sn, lengths, 0x00BEEF, None, 0, stride)
    assert need >= 6
    # originals and the recovery packets that protect them (a recovery packet is longer than the longest original)
    small = [24, 25, 39, 60, 7, 100]
    sr = Sender(L, small, seed=83)
    nrec = 3
    r2, m2, sizes2, need2 = packed_and_checked(L, sr, small, 7, sr.encode(nrec), nrec, stride)
    assert need2 >= 2 and max(sizes2[-nrec:]) > 105
    r2.free()
    sr.free()

    # absent originals take no space
    assert L.sgpu_encoder_remove_before(sn.enc, 3) == SUCCESS
    rows.refill()
    res, nrows, nframes = pack(L, sn.enc, 1, 0, 6, None, 0, rows, maxRows)
    at2, need2, ends2 = model_layout(sizes[3:6], stride)
    assert res == [NEED_MORE] * 3 + [SUCCESS] * 3 and (nrows, nframes) == (need2, 3)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens == [ends2[r] for r in range(need2)] + [0] * (maxRows - need2)
    r, fr = parse(L, b"".join(got[:need2]))
    assert r == SUCCESS and [(f.Flow, f.PacketNum, f.Bytes) for f in fr] == [(1, 3 + k, lengths[3 + k]) for k in range(3)]
    # nothing present: no rows, every length zero, no row touched
    rows.refill()
    res, nrows, nframes = pack(L, sn.enc, 1, 0, 3, None, 0, rows, maxRows)
    assert res == [NEED_MORE] * 3 and (nrows, nframes) == (0, 0)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens == [0] * maxRows and all(g == bytes([FILL]) * stride for g in got)

    # a frame one byte longer than the stride
    rows.refill()
    s1 = stats(L)
    res, nrows, nframes = pack(L, sn.enc, 1, 3, 3, None, 0, rows, maxRows, stride=stride - 16, want=INVALID)
    assert (nrows, nframes) == (0, 0)
    short = Sender(L, [stride - 8], seed=82)   # T = 9 + n = stride + 1
    res, nrows, nframes = pack(L, short.enc, 1, 0, 1, None, 0, rows, maxRows, want=INVALID)
    assert L.sgpu_flush() == 0
    assert rows.untouched() and stats(L)[STAT_FRAMES] == s1[STAT_FRAMES]
    short.free()
    rows.free()
    sn.free()


# 8 -------------------------------------------------------------------------
TRIP_STREAMS, TRIP_ORIGINALS, TRIP_RECOVERY, TRIP_STRIDE, TRIP_ROWS, TRIP_MAX = 40, 50, 36, 1424, 20, 32
TRIP_SEED = 8


def check_round_trip(path, device):
    """40 encoders' packets of 40-300 bytes packed into 1424-byte rows, one
    row in five dropped by zeroing its length, more than 256 rows in one scan:
    scan_packed -> recv_packed -> decode -> deliver_range gives the originals
    back."""
    L = load(path)
    rnd = random.Random(TRIP_SEED)
    stride, per = TRIP_STRIDE, TRIP_ROWS
    nrows = TRIP_STREAMS * per
    senders = [Sender(L, [rnd.randrange(40, 301) for _ in range(TRIP_ORIGINALS)], seed=900 + i)
               for i in range(TRIP_STREAMS)]
    dev = L.sgpu_device_alloc(nrows * stride)
    lensDev = L.sgpu_device_alloc(4 * nrows)
    assert dev and lensDev

    class Area:   # (pack()'s view of one stream's rows)
        pass

    used, queued = [], 0
    for i, sn in enumerate(senders):
        recs = sn.encode(TRIP_RECOVERY)
        a = Area()
        a.dst, a.lens, a.stride = dev + i * per * stride, lensDev + 4 * i * per, stride
        res, r, n = pack(L, sn.enc, i, 0, TRIP_ORIGINALS, recs, TRIP_RECOVERY, a, per)
        assert res == [SUCCESS] * TRIP_ORIGINALS and n == TRIP_ORIGINALS + TRIP_RECOVERY
        used.append(r)
        queued += n
    assert L.sgpu_flush() == 0
    assert sum(used) > 256
    # the network: about one row in five never arrives
    raw = D.read(L, lensDev, 4 * nrows)
    lens = [int.from_bytes(raw[4 * k:4 * k + 4], "little") for k in range(nrows)]
    assert all((lens[i * per + r] != 0) == (r < used[i]) for i in range(TRIP_STREAMS) for r in range(per))
    dropped = [k for k in range(nrows) if lens[k] and rnd.random() < 0.2]
    for k in dropped:
        lens[k] = 0
    raw = b"".join(v.to_bytes(4, "little") for v in lens)
    assert L.sgpu_h2d(lensDev, raw, len(raw)) == 0

    recs, words, o = scan(L, dev, stride, lensDev, nrows, TRIP_MAX)
    assert all(w == (w & PACKED_COUNT_MASK) for w in words), "no row is malformed or has more frames"
    assert all((words[k] != 0) == (lens[k] != 0) for k in range(nrows))
    decs = (C.c_void_p * TRIP_STREAMS)(*[L.sgpu_decoder_create() for _ in range(TRIP_STREAMS)])
    n = C.c_uint(0)
    assert L.sgpu_frames_recv_packed(decs, TRIP_STREAMS, o.out, TRIP_MAX, dev, stride, nrows, None,
                                     C.byref(n)) == SUCCESS
    assert n.value == sum(words) and 0 < n.value < queued
    pending = []
    for i in range(TRIP_STREAMS):
        out, k = C.c_void_p(), C.c_uint(0)
        r = (L.sgpu_decode_device if device else L.sgpu_decode)(decs[i], C.byref(out), C.byref(k))
        if r == PENDING:
            pending.append(i)
        else:
            assert r in (SUCCESS, NEED_MORE), "stream %d: decode returned %d" % (i, r)
    assert L.sgpu_flush() == 0
    for i in pending:
        out, k = C.c_void_p(), C.c_uint(0)
        assert L.sgpu_decode_device(decs[i], C.byref(out), C.byref(k)) == SUCCESS, "stream %d" % i
    back = Rows(L, TRIP_STREAMS * TRIP_ORIGINALS, 304)
    for i in range(TRIP_STREAMS):
        res, q = D.deliver(L, decs[i], 0, TRIP_ORIGINALS, back, dst=back.dst + i * TRIP_ORIGINALS * 304,
                           lens=back.lens + 4 * i * TRIP_ORIGINALS)
        assert res == [SUCCESS] * TRIP_ORIGINALS, "stream %d did not decode: choose another TRIP_SEED" % i
    assert L.sgpu_flush() == 0
    got, glens = back.fetch()
    for i, sn in enumerate(senders):
        for k, d in enumerate(sn.data):
            D.check_row(got[i * TRIP_ORIGINALS + k], glens[i * TRIP_ORIGINALS + k], d, "stream %d original %d" % (i, k))
    for i in range(TRIP_STREAMS):
        L.sgpu_decoder_free(decs[i])
    assert L.sgpu_flush() == 0
    back.free()
    o.free()
    L.sgpu_device_free(dev)
    L.sgpu_device_free(lensDev)
    for sn in senders:
        sn.free()


# 9 -------------------------------------------------------------------------
def check_arguments(path, gpu):
    L = load(path)
    stride, count, m = 64, 4, 2
    built = [row_of([frame(ORIGINAL, 0, k, payload(700 + k, 10 + k)), 3, frame(ORIGINAL, 0, 10 + k, payload(5, 4))],
                    stride) for k in range(count)]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    o = Out(L, count, m)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    assert L.sgpu_flush() == 0
    s0 = stats(L)
    assert L.sgpu_frames_packed_bytes(3, 0) == 0 and L.sgpu_frames_packed_bytes(3, 257) == 0
    assert L.sgpu_frames_packed_bytes(3, 256) == 3 * 256 * 32 + 12

    def scan_args(**kw):
        a = dict(rows=dr.dev, stride=stride, lens=dr.lens, count=count, m=m, out=o.out)
        a.update(kw)
        return L.sgpu_frames_scan_packed(a["rows"], a["stride"], a["lens"], a["count"], a["m"], a["out"])

    rowArgs = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=dr.dev + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=72)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("maxFrames zero", dict(m=0)),
        ("maxFrames above 256", dict(m=257)),
    ]
    for what, kw in rowArgs + [("null output", dict(out=None)), ("output not 16-byte aligned", dict(out=o.out + 8)),
                               ("lengths not 4-byte aligned", dict(lens=dr.lens + 2)),
                               ("an output above 4 GiB", dict(count=1 << 19, m=256))]:
        assert scan_args(**kw) == -1, what
    assert o.untouched()

    L.sgpu_timing(1, 1, None, None)
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * 9)()
    L.sgpu_timing_kernels(ms, 9)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[8] > 0 and ms[7] == 0, "k_walk's device time is timing index 8"
    recs, words = o.fetch()
    assert words == [2] * count
    s1 = stats(L)
    assert s1[STAT_WALKS] - s0[STAT_WALKS] == count, "only the one valid scan was queued"
    assert s1[K.STAT_SCANS] == s0[K.STAT_SCANS]

    def recv_args(**kw):
        a = dict(decs=decs, heads=o.out, rows=dr.dev, stride=stride, count=count, m=m)
        a.update(kw)
        n = C.c_uint(99)
        res = (C.c_int * (count * m))(*([-1] * (count * m)))
        r = L.sgpu_frames_recv_packed(a["decs"], 1, a["heads"], a["m"], a["rows"], a["stride"], a["count"], res,
                                      C.byref(n))
        return r, n.value, list(res)

    for what, kw in rowArgs + [("null decoders", dict(decs=None)), ("null records", dict(heads=None)),
                               ("records not 4-byte aligned", dict(heads=o.out + 2))]:
        r, n, res = recv_args(**kw)
        assert (r, n, res) == (INVALID, 0, [-1] * (count * m)), what
    assert L.sgpu_frames_recv_packed(decs, 1, o.out, m, dr.dev, stride, count, None, None) == INVALID
    for k in range(count):
        assert L.sgpu_decoder_has(dec, k) == NEED_MORE, "a refused call must not reach the decoder"

    # count == 0: a ticket that is complete, nothing scanned; nothing accepted
    for kw in (dict(count=0), dict(count=0, rows=None, lens=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    assert recv_args(count=0)[:2] == (SUCCESS, 0)
    assert recv_args(count=0, decs=None, heads=None, rows=None)[:2] == (SUCCESS, 0)
    assert L.sgpu_flush() == 0
    s2 = stats(L)
    assert (s2[0], s2[1], s2[STAT_WALKS]) == (s1[0], s1[1], s1[STAT_WALKS]), "nothing was queued by any of them"
    assert o.fetch() == (recs, words)

    # the packer's arguments
    sn = Sender(L, [20, 30], seed=91)
    other = Sender(L, [20, 30], seed=92)
    mine, theirs = sn.encode(1), other.encode(1)
    rows = Rows(L, 4, stride)

    def pack_args(**kw):
        a = dict(enc=sn.enc, flow=1, first=0, n=2, recs=mine, nrec=1, dst=rows.dst, stride=stride, maxRows=4,
                 lens=rows.lens, rowsOut=True, framesOut=True)
        a.update(kw)
        nr, nf = C.c_uint(7), C.c_uint(7)
        r = L.sgpu_encoder_pack_frames(a["enc"], a["flow"], a["first"], a["n"], a["recs"], a["nrec"], a["dst"],
                                       a["stride"], a["maxRows"], a["lens"], None,
                                       C.byref(nr) if a["rowsOut"] else None, C.byref(nf) if a["framesOut"] else None)
        if r != SUCCESS:
            assert (nr.value if a["rowsOut"] else 0, nf.value if a["framesOut"] else 0) == (0, 0), "nothing was queued"
        return r if r != SUCCESS else (r, nr.value, nf.value)

    stale = (Rec * 1)()
    C.memmove(stale, mine, C.sizeof(Rec))
    stale[0].DeviceData = theirs[0].DeviceData
    for what, kw in [("null encoder", dict(enc=None)), ("null rows", dict(dst=None)), ("null lengths", dict(lens=None)),
                     ("rows not 16-byte aligned", dict(dst=rows.dst + 8)), ("stride zero", dict(stride=0)),
                     ("stride no multiple of 16", dict(stride=72)), ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
                     ("lengths not 4-byte aligned", dict(lens=rows.lens + 2)), ("flow above 2^24-1", dict(flow=1 << 24)),
                     ("SGPU_FRAME_NONE", dict(flow=F.NONE)), ("first above the maximum", dict(first=PACKET_NUM_MAX + 1)),
                     ("null recovery with a count", dict(recs=None)), ("another encoder's packet", dict(recs=theirs)),
                     ("a buffer that is not this encoder's output", dict(recs=stale)),
                     ("null rowsOut", dict(rowsOut=False)), ("null framesOut", dict(framesOut=False))]:
        assert pack_args(**kw) == INVALID, what
    assert L.sgpu_flush() == 0
    assert rows.untouched() and stats(L)[STAT_FRAMES] == s2[STAT_FRAMES]
    r, nr, nf = pack_args()
    assert (r, nf) == (SUCCESS, 3) and 2 <= nr <= 3   # frames of 28 and 38 bytes and the recovery packet's
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert all(lens[:nr]) and lens[nr:] == [0] * (4 - nr)

    # (the arguments were fine otherwise)
    r, n, res = recv_args()
    assert (r, n, res) == (SUCCESS, count * m, [SUCCESS] * (count * m))
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    rows.free()
    sn.free()
    other.free()
    o.free()
    dr.free()


# 10 (the CPU double only) ---------------------------------------------------
def check_forged(path):
    """Records and row words are caller data: sgpu_frames_recv_packed refuses
    the ones no scan could have written, without touching a decoder."""
    L = load(path)
    stride, m = 128, 2
    kinds = [ORIGINAL] * 7 + [RECOVERY] * 3
    rows, lens = [], []
    for k, kind in enumerate(kinds):
        row, end = row_of([frame(ORIGINAL, 0, 50 + k, payload(800 + k, 12 + k)), 1 + k,
                           frame(kind, 0, 150 + k, payload(850 + k, 12 + k))], stride)
        rows.append(row)
        lens.append(end)
    dr = DevRows(L, rows, stride, lens)
    count = len(rows)
    recsOut, words, o = scan(L, dr.dev, stride, dr.lens, count, m)
    assert words == [2] * count
    recs = (PackedHead * (count * m)).from_address(o.out)
    wordsAt = (C.c_uint * count).from_address(o.out + count * m * REC)
    forged = {
        1: dict(Offset=stride - 8),                # Offset + HeaderBytes + DataBytes > stride
        2: dict(Offset=1 << 31),
        3: dict(DataBytes=stride),
        4: dict(Type=7),
        5: dict(TailBytes=1),                      # an original has no tail
        6: dict(Status=3),
        7: dict(TailBytes=7),                      # min(8, DataBytes) is 8 here
        8: dict(Flow=1 << 24),
    }
    for k, kw in forged.items():
        for name, v in kw.items():
            setattr(recs[k * m + 1], name, v)
    wordsAt[9] = m + 1                             # more records than the scan was given room for
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    results = (C.c_int * (count * m))(*([-1] * (count * m)))
    n = C.c_uint(99)
    assert L.sgpu_frames_recv_packed(decs, 1, o.out, m, dr.dev, stride, count, results, C.byref(n)) == INVALID
    res = [list(results[k * m:(k + 1) * m]) for k in range(count)]
    assert res[0] == [SUCCESS, SUCCESS]
    assert res[1:9] == [[SUCCESS, INVALID]] * 8
    assert res[9] == [INVALID, NEED_MORE]
    assert n.value == 10
    for k in range(9):
        assert L.sgpu_decoder_has(dec, 50 + k) == SUCCESS
    assert L.sgpu_decoder_has(dec, 150) == SUCCESS
    for k in range(1, 7):
        assert L.sgpu_decoder_has(dec, 150 + k) == NEED_MORE
    assert L.sgpu_decoder_has(dec, 59) == NEED_MORE
    assert L.sgpu_decoder_is_ready(dec) == NEED_MORE, "no recovery packet reached the decoder"
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    dr.free()
