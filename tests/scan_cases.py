"""sgpu_frames_scan_rows / sgpu_frames_recv_rows: the cases shared by
test_scan_cpu.py (the CPU test double, tests/hostsim) and test_scan_gpu.py
(k_scan on the MI355X), driven through the C ABI with ctypes.

Expected records come from sgpu_frames_parse and plain slices of the bytes a
case put into the rows; expected decoder state comes from sgpu_frames_recv
over a host copy of the same rows.  Every scan writes into records with one
guard record before and one after, pre-filled with 0xA5, and checks that the
guards are intact.
"""
import ctypes as C

import deliver_cases as D
import frame_cases as F
from deliver_cases import FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, SUCCESS, Rows, payload
from frame_cases import ORIGINAL, RECOVERY, Sender, header
from siamese_amd.binding import ROW_EMPTY, ROW_MALFORMED, ROW_OK, RowHead, bind_rows_abi

STAT_SCANS = 23
NSTATS = 24
REC = C.sizeof(RowHead)


class Frame(C.Structure):
    _fields_ = [("Type", C.c_uint), ("Flow", C.c_uint), ("PacketNum", C.c_uint), ("Offset", C.c_uint),
                ("Bytes", C.c_uint)]


def load(path):
    L = F.load(path)
    if getattr(L, "_scan_cases", False):
        return L
    # (the two symbols under test: an AttributeError here is the parent's answer)
    bind_rows_abi(L)
    L.sgpu_frames_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p]
    L.sgpu_decoder_has.argtypes = [C.c_void_p, C.c_uint]
    L._scan_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


def parse(L, raw):
    """(result, frames) of sgpu_frames_parse over raw."""
    out = (Frame * 4)()
    n = C.c_uint(0)
    r = L.sgpu_frames_parse(raw, len(raw), out, 4, C.byref(n))
    return r, [out[k] for k in range(n.value)]


def fields(h):
    return (h.FrameBytes, h.Status, h.Type, h.HeaderBytes, h.TailBytes, h.Flow, h.PacketNum, h.DataBytes,
            bytes(h.Head), bytes(h.Tail))


EMPTY = (0, ROW_EMPTY, 0, 0, 0, 0, 0, 0, bytes(4), bytes(8))
MALFORMED = (0, ROW_MALFORMED, 0, 0, 0, 0, 0, 0, bytes(4), bytes(8))


def expected(L, row):
    """The record of a well-formed row, from sgpu_frames_parse and slices."""
    r, fr = parse(L, row)
    assert r == SUCCESS and len(fr) == 1, "the case's own row must be one frame and zero padding"
    f = fr[0]
    data = row[f.Offset:f.Offset + f.Bytes]
    if f.Type == ORIGINAL:
        return (f.Offset + f.Bytes, ROW_OK, ORIGINAL, f.Offset, 0, f.Flow, f.PacketNum, f.Bytes, bytes(4), bytes(8))
    t = min(8, f.Bytes)
    return (f.Offset + f.Bytes, ROW_OK, RECOVERY, f.Offset, t, f.Flow, 0, f.Bytes,
            data[:4] + bytes(4 - len(data[:4])), bytes(8 - t) + data[len(data) - t:])


class Heads:
    """count records in pinned memory between two guard records, all 0xA5."""

    def __init__(self, L, count):
        self.L, self.count = L, count
        self.bytes = (count + 2) * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the records was written"
        assert raw[-REC:] == guard, "guard record after the records was written"
        return [RowHead.from_buffer_copy(raw, REC * (k + 1)) for k in range(self.count)]

    def untouched(self):
        return C.string_at(self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_host_free(self.base)


def scan(L, dev, stride, lens, count):
    """The records of one scan, guards checked: (records as field tuples, Heads)."""
    hd = Heads(L, count)
    t = L.sgpu_frames_scan_rows(dev, stride, lens, count, hd.out)
    assert t > 0, "sgpu_frames_scan_rows returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return [fields(h) for h in hd.fetch()], hd


class DevRows:
    """Host-built rows in a device allocation of exactly count * stride bytes
    (the last row ends where the allocation ends), lengths beside them."""

    def __init__(self, L, rows, stride, lens):
        assert all(len(r) == stride for r in rows) and stride % 16 == 0
        self.L, self.stride, self.count = L, stride, len(rows)
        blob = b"".join(rows)
        self.dev = L.sgpu_device_alloc(len(blob))
        self.lens = L.sgpu_device_alloc(4 * len(rows))
        assert self.dev and self.lens and self.dev % 16 == 0
        assert L.sgpu_h2d(self.dev, blob, len(blob)) == 0
        lraw = b"".join(int(v).to_bytes(4, "little") for v in lens)
        assert L.sgpu_h2d(self.lens, lraw, len(lraw)) == 0

    def free(self):
        self.L.sgpu_device_free(self.dev)
        self.L.sgpu_device_free(self.lens)


def frame_row(L, kind, flow, num, data, stride):
    """(row, frame bytes) of one framed packet, zero tail up to the stride."""
    fr = header(L, kind, flow, num, len(data)) + data
    assert len(fr) <= stride
    return fr + bytes(stride - len(fr)), len(fr)


def check_scan(L, rows, stride, lens, want, wantNoLens=None):
    """Scan host-built rows with and without their lengths."""
    dr = DevRows(L, rows, stride, lens)
    for lp, w in ((dr.lens, want), (None, want if wantNoLens is None else wantNoLens)):
        got, hd = scan(L, dr.dev, stride, lp, dr.count)
        for k in range(dr.count):
            assert got[k] == w[k], "row %d (%s lengths): %r, expected %r" % (k, "with" if lp else "without",
                                                                              got[k], w[k])
        hd.free()
    dr.free()


# 1 -------------------------------------------------------------------------
# data sizes on both sides of each prefix-width boundary of the frame's L
# (7 + n for originals, 4 + n for recovery packets: 0x7f/0x80, 0x3fff/0x4000,
# 0x1fffff/0x200000), the short recovery packets whose Head and Tail are
# partial, and a one-byte original
SMALL_ORIGINALS = [1, 120, 121, 16376, 16377]
SMALL_RECOVERY = [2, 3, 4, 5, 6, 7, 8, 9, 123, 124, 16379, 16380, 16381]
SMALL_STRIDE = 16400
BIG_ORIGINALS = [2097144, 2097145]
BIG_STRIDE = 2097168


def check_header_edges(path):
    L = load(path)
    for sizes, recs, stride in ((SMALL_ORIGINALS, SMALL_RECOVERY, SMALL_STRIDE), (BIG_ORIGINALS, [], BIG_STRIDE)):
        rows, lens = [], []
        for i, n in enumerate(sizes):
            num = PACKET_NUM_MAX if i == 0 else 1000 * i + 7
            row, used = frame_row(L, ORIGINAL, 0xABCDEF - i, num, payload(100 + i, n), stride)
            rows.append(row)
            lens.append(used)
        for i, n in enumerate(recs):
            row, used = frame_row(L, RECOVERY, 0x010203 + i, 0, payload(200 + i, n), stride)
            rows.append(row)
            lens.append(used)
        want = [expected(L, r) for r in rows]
        assert [w[0] for w in want] == lens
        if recs:
            # header = prefix (1, 2, 3 bytes) + 7 or 4
            assert sorted({w[3] for w in want}) == [5, 6, 7, 8, 9, 10]
            assert sorted({w[4] for w in want if w[2] == RECOVERY}) == [2, 3, 4, 5, 6, 7, 8]
        else:
            assert [w[3] for w in want] == [10, 11]
        check_scan(L, rows, stride, lens, want)


# 2 -------------------------------------------------------------------------
def check_tail_alignment(path):
    """Recovery rows whose data ends at every byte residue mod 16, with the
    tail in the row's first aligned word, in one later word and across two;
    the last row's frame fills it, at the end of the allocation."""
    L = load(path)
    stride = 64
    ends = list(range(17, 49)) + [stride]
    rows, lens = [], []
    for i, e in enumerate(ends):
        row, used = frame_row(L, RECOVERY, i, 0, payload(300 + i, e - 5), stride)
        assert used == e
        rows.append(row)
        lens.append(used)
    assert {e % 16 for e in ends} == set(range(16)) and lens[-1] == stride
    want = [expected(L, r) for r in rows]
    check_scan(L, rows, stride, lens, want)


# 3 -------------------------------------------------------------------------
def check_empty_and_stale(path):
    """Rows from sgpu_encoder_deliver_range with some originals absent: the
    lengths decide, and without them an old frame is a frame."""
    L = load(path)
    stride = 512
    sn = Sender(L, [300 + 7 * i for i in range(20)], seed=61)
    rows = Rows(L, 10, stride)
    res, queued = F.originals(L, sn.enc, 0, 10, 5, rows)
    assert res == [SUCCESS] * 10 and queued == 10
    assert L.sgpu_flush() == 0
    assert L.sgpu_encoder_remove_before(sn.enc, 14) == SUCCESS
    res, queued = F.originals(L, sn.enc, 10, 10, 5, rows)
    assert res == [NEED_MORE] * 4 + [SUCCESS] * 6 and queued == 6
    assert L.sgpu_flush() == 0
    raw, lens = rows.fetch()
    assert lens[:4] == [0] * 4 and all(lens[4:])

    def want(k):
        fr = header(L, ORIGINAL, 5, k, len(sn.data[k])) + sn.data[k]
        return expected(L, fr + bytes(stride - len(fr)))

    old = [want(k) for k in range(4)]
    new = [want(10 + k) for k in range(4, 10)]
    assert [raw[k][:old[k][0]] for k in range(4)] == [header(L, ORIGINAL, 5, k, len(sn.data[k])) + sn.data[k]
                                                       for k in range(4)], "the stale rows still hold their frames"
    got, hd = scan(L, rows.dst, stride, rows.lens, 10)
    assert got == [EMPTY] * 4 + new
    hd.free()
    got, hd = scan(L, rows.dst, stride, None, 10)
    assert got == old + new
    hd.free()
    # a row that starts with a zero byte: empty without lengths; with a
    # non-zero length its frame is an L of zero, which no length equals
    assert L.sgpu_h2d(rows.dst + 6 * stride, bytes(16), 16) == 0
    got, hd = scan(L, rows.dst, stride, None, 10)
    assert got == old + new[:2] + [EMPTY] + new[3:]
    hd.free()
    got, hd = scan(L, rows.dst, stride, rows.lens, 10)
    assert got == [EMPTY] * 4 + new[:2] + [MALFORMED] + new[3:]
    hd.free()
    rows.fetch()   # (the guard rows)
    rows.free()
    sn.free()


# 4 -------------------------------------------------------------------------
def check_malformed(path):
    """Each malformed row alone between good originals of flow 0."""
    L = load(path)
    stride = 64

    def good(num):
        return frame_row(L, ORIGINAL, 0, num, payload(400 + num, 20 + num), stride)

    def raw_row(b):
        return b[:stride] + bytes(stride - len(b[:stride]))

    fill = payload(499, 80)
    ok, okLen = frame_row(L, ORIGINAL, 0, 77, payload(477, 30), stride)
    # (row, length word, sgpu_frames_parse must reject it, status without lengths)
    bad = [
        # prefix + L = stride + 1
        (raw_row(header(L, RECOVERY, 0, 0, 60) + fill), stride + 1, True, ROW_MALFORMED),
        # a frame that is fine, and a length that is not its own
        (ok, okLen + 1, False, ROW_OK),
        # type 2
        (raw_row(bytes([24, 2, 0, 0, 0]) + fill[:20]), 25, True, ROW_MALFORMED),
        # L too small for the inner header: an original of no bytes, a recovery packet of none
        (raw_row(bytes([7, ORIGINAL, 0, 0, 0, 99, 0, 0])), 8, True, ROW_MALFORMED),
        (raw_row(bytes([4, RECOVERY, 0, 0, 0])), 5, True, ROW_MALFORMED),
        (raw_row(bytes([1, ORIGINAL])), 2, True, ROW_MALFORMED),
        # PacketNum above the maximum (sgpu_frames_parse leaves that to sgpu_frames_recv, which refuses it)
        (raw_row(bytes([27, ORIGINAL, 0, 0, 0, 0x00, 0x00, 0x40]) + fill[:20]), 28, False, ROW_MALFORMED),
        # non-canonical prefixes: wide ones that carry an L of zero ...
        (raw_row(bytes([0x80, 0x00, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20]), 29, True, ROW_MALFORMED),
        (raw_row(bytes([0xC0, 0x00, 0x00, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20]), 30, True, ROW_MALFORMED),
        (raw_row(bytes([0xE0, 0x00, 0x00, 0x00, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20]), 31, True, ROW_MALFORMED),
        # ... and an over-long one
        (raw_row(bytes([0xFF, 0xFF, 0xFF, 0xFF, ORIGINAL, 0, 0, 0, 1, 0, 0]) + fill[:20]), 31, True, ROW_MALFORMED),
    ]
    rows, lens, want, wantNoLens, isBad = [], [], [], [], []
    for i, (row, length, parseRejects, bare) in enumerate(bad):
        g, gl = good(i)
        rows += [g, row]
        lens += [gl, length]
        want += [expected(L, g), MALFORMED]
        wantNoLens += [expected(L, g), MALFORMED if bare == ROW_MALFORMED else expected(L, row)]
        isBad += [False, True]
        if parseRejects:
            r, fr = parse(L, row)
            assert r != SUCCESS and fr == [], "case %d: sgpu_frames_parse must reject this row" % i
    g, gl = good(len(bad))
    rows.append(g)
    lens.append(gl)
    want.append(expected(L, g))
    wantNoLens.append(want[-1])
    isBad.append(False)
    # (a wide prefix with a non-zero L is a frame to sgpu_frames_parse, and so to the scan)
    wide, wideLen = raw_row(bytes([0x80, 27, ORIGINAL, 0, 0, 0, 200, 0, 0]) + fill[:20]), 29
    assert parse(L, wide)[0] == SUCCESS
    rows.append(wide)
    lens.append(wideLen)
    want.append(expected(L, wide))
    wantNoLens.append(want[-1])
    isBad.append(False)
    count = len(rows)
    check_scan(L, rows, stride, lens, want, wantNoLens)

    dr = DevRows(L, rows, stride, lens)
    got, hd = scan(L, dr.dev, stride, dr.lens, count)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    results = (C.c_int * count)(*([-1] * count))
    n = C.c_uint(99)
    assert L.sgpu_frames_recv_rows(decs, 1, hd.out, dr.dev, stride, count, results, C.byref(n)) == INVALID
    assert list(results) == [INVALID if b else SUCCESS for b in isBad]
    assert n.value == isBad.count(False)
    for k in range(count):
        if not isBad[k]:
            assert L.sgpu_decoder_has(dec, want[k][6]) == SUCCESS
    assert L.sgpu_decoder_has(dec, 77) == NEED_MORE and L.sgpu_decoder_has(dec, 99) == NEED_MORE
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    hd.free()
    dr.free()


# 5 -------------------------------------------------------------------------
def delivered(L, dec, count, stride):
    back = Rows(L, count, stride)
    res, queued = D.deliver(L, dec, 0, count, back)
    assert res == [SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    got, lens = back.fetch()
    back.free()
    return [got[k][:lens[k]] for k in range(count)], [got[k][lens[k]:] for k in range(count)]


def check_parity(path):
    """frame_cases.check_round_trip's stream into two decoders: A through a
    host copy and sgpu_frames_recv, B through scan_rows -> gather_wait ->
    recv_rows on the same device rows."""
    L = load(path)
    lengths = [40 + (i * 97) % 1300 for i in range(24)]
    lost = (2, 5, 9, 17)
    nrec = 6
    stride = 1360
    sn = Sender(L, lengths, seed=51)
    nrows = len(lengths) - len(lost) + nrec
    rows = Rows(L, nrows, stride)
    at = 0
    runs, start = [], 0
    for k in sorted(lost) + [len(lengths)]:
        if k > start:
            runs.append((start, k - start))
        start = k + 1
    for first, n in runs:
        res, queued = F.originals(L, sn.enc, first, n, 0, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at)
        assert res == [SUCCESS] * n and queued == n
        at += n
    recs = sn.encode(nrec)
    assert F.recovery(L, recs, nrec, [0] * nrec, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at) == nrec
    assert at + nrec == nrows
    assert L.sgpu_flush() == 0

    # A: the host copy
    got, lens = rows.fetch()
    wire = b"".join(got)
    host = L.sgpu_host_alloc(len(wire))
    assert host
    C.memmove(host, wire, len(wire))
    decA = L.sgpu_decoder_create()
    resA = (C.c_int * nrows)(*([-1] * nrows))
    n = C.c_uint(0)
    assert L.sgpu_frames_recv((C.c_void_p * 1)(decA), 1, host, rows.dst, len(wire), resA, nrows,
                              C.byref(n)) == SUCCESS
    assert n.value == nrows

    # B: no payload byte crosses to the host
    decB = L.sgpu_decoder_create()
    s0 = stats(L)
    heads, hd = scan(L, rows.dst, stride, rows.lens, nrows)
    assert stats(L)[STAT_SCANS] - s0[STAT_SCANS] == nrows
    assert heads == [expected(L, r) for r in got]
    resB = (C.c_int * nrows)(*([-1] * nrows))
    m = C.c_uint(0)
    assert L.sgpu_frames_recv_rows((C.c_void_p * 1)(decB), 1, hd.out, rows.dst, stride, nrows, resB,
                                   C.byref(m)) == SUCCESS
    assert m.value == nrows
    assert list(resA) == list(resB) == [SUCCESS] * nrows

    assert L.sgpu_decoder_is_ready(decA) == L.sgpu_decoder_is_ready(decB) == SUCCESS
    counts = []
    for dec in (decA, decB):
        out, k = C.c_void_p(), C.c_uint(0)
        assert L.sgpu_decode(dec, C.byref(out), C.byref(k)) == SUCCESS
        counts.append(k.value)
    assert counts == [len(lost)] * 2
    a, atail = delivered(L, decA, len(lengths), 1344)
    b, btail = delivered(L, decB, len(lengths), 1344)
    assert a == b and atail == btail
    assert b == sn.data, "the delivered originals are the sender's"
    assert all(t == bytes(len(t)) for t in btail)
    for dec in (decA, decB):
        L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    L.sgpu_host_free(host)
    hd.free()
    rows.free()
    sn.free()


# 6 -------------------------------------------------------------------------
def check_many_flows(path, gpu):
    """64 senders frame into one buffer, flows interleaved row by row; one
    scan and one recv_rows over the decoders."""
    L = load(path)
    flows, size, stride = 64, 200, 256
    senders = [Sender(L, [size - i, size, 1 + i], seed=600 + i) for i in range(flows)]
    nrows = 3 * flows
    rows = Rows(L, nrows, stride)
    for i, sn in enumerate(senders):
        # original 1 is lost; originals 0 and 2 and one recovery packet travel
        for j, num in enumerate((0, 2)):
            at = j * flows + i
            res, queued = F.originals(L, sn.enc, num, 1, i, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at)
            assert res == [SUCCESS] and queued == 1
        at = 2 * flows + i
        assert F.recovery(L, sn.encode(1), 1, [i], rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at) == 1
    assert L.sgpu_flush() == 0
    L.sgpu_timing(1, 1, None, None)
    s0 = stats(L)
    heads, hd = scan(L, rows.dst, stride, rows.lens, nrows)
    assert stats(L)[STAT_SCANS] - s0[STAT_SCANS] == nrows
    ms = (C.c_double * 8)()
    L.sgpu_timing_kernels(ms, 8)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[7] > 0, "k_scan's device time is timing index 7"
    got, lens = rows.fetch()
    assert heads == [expected(L, r) for r in got]
    assert [h[5] for h in heads] == list(range(flows)) * 3

    # decoders for flows 0..61, slot 5 empty: flows 5, 62 and 63 have none
    ndec, hole = flows - 2, 5
    decs = (C.c_void_p * ndec)(*[None if i == hole else L.sgpu_decoder_create() for i in range(ndec)])
    homeless = {hole, flows - 2, flows - 1}
    results = (C.c_int * nrows)(*([-1] * nrows))
    n = C.c_uint(0)
    assert L.sgpu_frames_recv_rows(decs, ndec, hd.out, rows.dst, stride, nrows, results, C.byref(n)) == INVALID
    assert list(results) == [INVALID if (k % flows) in homeless else SUCCESS for k in range(nrows)]
    assert n.value == nrows - 3 * len(homeless)
    live = [i for i in range(ndec) if i != hole]
    for i in live:
        out, k = C.c_void_p(), C.c_uint(0)
        assert L.sgpu_decoder_is_ready(decs[i]) == SUCCESS
        assert L.sgpu_decode(decs[i], C.byref(out), C.byref(k)) == SUCCESS and k.value == 1
    back = Rows(L, 3 * flows, stride)
    for i in live:
        res, queued = D.deliver(L, decs[i], 0, 3, back, dst=back.dst + 3 * i * stride, lens=back.lens + 12 * i)
        assert res == [SUCCESS] * 3 and queued == 3
    assert L.sgpu_flush() == 0
    got, lens = back.fetch()
    for i in live:
        for k in range(3):
            D.check_row(got[3 * i + k], lens[3 * i + k], senders[i].data[k], "flow %d original %d" % (i, k))
    for i in live:
        L.sgpu_decoder_free(decs[i])
    assert L.sgpu_flush() == 0
    back.free()
    hd.free()
    rows.free()
    for sn in senders:
        sn.free()


# 7 -------------------------------------------------------------------------
def check_arguments(path):
    L = load(path)
    stride, count = 64, 4
    built = [frame_row(L, ORIGINAL, 0, k, payload(700 + k, 10 + k), stride) for k in range(count)]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    hd = Heads(L, count)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    assert L.sgpu_flush() == 0
    s0 = stats(L)

    def scan_args(**kw):
        a = dict(rows=dr.dev, stride=stride, lens=dr.lens, count=count, out=hd.out)
        a.update(kw)
        return L.sgpu_frames_scan_rows(a["rows"], a["stride"], a["lens"], a["count"], a["out"])

    rowArgs = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=dr.dev + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=72)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
    ]
    for what, kw in rowArgs + [("null records", dict(out=None)), ("records not 16-byte aligned", dict(out=hd.out + 8)),
                               ("lengths not 4-byte aligned", dict(lens=dr.lens + 2))]:
        assert scan_args(**kw) == -1, what
    assert hd.untouched()

    # records for the host call's checks
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    good = [fields(h) for h in hd.fetch()]
    assert good == [expected(L, r) for r, _ in built]
    s1 = stats(L)
    assert s1[STAT_SCANS] - s0[STAT_SCANS] == count, "only the one valid scan was queued"

    def recv_args(**kw):
        a = dict(decs=decs, heads=hd.out, rows=dr.dev, stride=stride, count=count)
        a.update(kw)
        n = C.c_uint(99)
        res = (C.c_int * count)(*([-1] * count))
        r = L.sgpu_frames_recv_rows(a["decs"], 1, a["heads"], a["rows"], a["stride"], a["count"], res, C.byref(n))
        return r, n.value, list(res)

    for what, kw in rowArgs + [("null decoders", dict(decs=None)), ("null records", dict(heads=None)),
                               ("records not 4-byte aligned", dict(heads=hd.out + 2))]:
        r, n, res = recv_args(**kw)
        assert (r, n, res) == (INVALID, 0, [-1] * count), what
    assert L.sgpu_frames_recv_rows(decs, 1, hd.out, dr.dev, stride, count, None, None) == INVALID, "null acceptedOut"
    for k in range(count):
        assert L.sgpu_decoder_has(dec, k) == NEED_MORE, "a refused call must not reach the decoder"

    # count == 0: a ticket that is complete, nothing scanned; nothing accepted
    for kw in (dict(count=0), dict(count=0, rows=None, lens=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    r, n, res = recv_args(count=0)
    assert (r, n) == (SUCCESS, 0)
    r, n, res = recv_args(count=0, decs=None, heads=None, rows=None)
    assert (r, n) == (SUCCESS, 0)
    assert L.sgpu_flush() == 0
    s2 = stats(L)
    assert (s2[0], s2[1], s2[STAT_SCANS]) == (s1[0], s1[1], s1[STAT_SCANS]), "nothing was queued by any of them"
    assert [fields(h) for h in hd.fetch()] == good

    # (the arguments were fine otherwise)
    r, n, res = recv_args()
    assert (r, n, res) == (SUCCESS, count, [SUCCESS] * count)
    assert L.sgpu_flush() == 0
    out, lens = delivered(L, dec, count, stride)
    assert out == [payload(700 + k, 10 + k) for k in range(count)]
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    hd.free()
    dr.free()


# 8 -------------------------------------------------------------------------
def check_forged(path):
    """Records are caller data: sgpu_frames_recv_rows refuses the ones no scan
    could have written, row by row, without touching a decoder."""
    L = load(path)
    stride = 64
    kinds = [ORIGINAL] * 8 + [RECOVERY] * 3
    built = [frame_row(L, kind, 0, 50 + k, payload(800 + k, 12 + k), stride) for k, kind in enumerate(kinds)]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    got, hd = scan(L, dr.dev, stride, dr.lens, len(built))
    assert got == [expected(L, r) for r, _ in built]
    recs = (RowHead * len(built)).from_address(hd.out)
    forged = {
        1: dict(DataBytes=stride),                 # HeaderBytes + DataBytes > stride
        2: dict(Type=7),
        3: dict(TailBytes=1),                      # an original has no tail
        4: dict(Status=3),
        5: dict(FrameBytes=recs[5].FrameBytes - 1),   # HeaderBytes + DataBytes > FrameBytes
        6: dict(HeaderBytes=7),                    # an original's header is 8 bytes at least
        7: dict(PacketNum=PACKET_NUM_MAX + 1),
        8: dict(TailBytes=9),
        9: dict(TailBytes=7),                      # min(8, DataBytes) is 8 here
        10: dict(Flow=1 << 24),
    }
    for k, kw in forged.items():
        for name, v in kw.items():
            setattr(recs[k], name, v)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * (1 << 8))(dec)
    results = (C.c_int * len(built))(*([-1] * len(built)))
    n = C.c_uint(99)
    assert L.sgpu_frames_recv_rows(decs, 1 << 8, hd.out, dr.dev, stride, len(built), results, C.byref(n)) == INVALID
    assert list(results) == [SUCCESS] + [INVALID] * 10
    assert n.value == 1
    assert L.sgpu_decoder_has(dec, 50) == SUCCESS
    for k in range(1, 8):
        assert L.sgpu_decoder_has(dec, 50 + k) == NEED_MORE
    assert L.sgpu_decoder_is_ready(dec) == NEED_MORE, "no recovery packet reached the decoder"
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    hd.free()
    dr.free()
