"""sgpu_encoder_deliver_range / sgpu_frames_deliver_recovery: the cases shared
by test_frame_cpu.py (the CPU test double, tests/hostsim) and
test_frame_gpu.py (k_frame on the MI355X), driven through the C ABI with
ctypes.

Expected bytes are built here from the originals each case feeds in and
sgpu_frame_write_header, or come from the library's older ways out
(sgpu_gather, sgpu_frames_send).  Every case frames into rows with one guard
row before and one after, lengths with a guard word on each side, everything
pre-filled with 0xA5 (deliver_cases.Rows), and checks that the guards are
intact.
"""
import ctypes as C

import deliver_cases as D
from deliver_cases import FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, SUCCESS, Rec, Rows, payload

ORIGINAL, RECOVERY = 0, 1
NONE = 0xffffffff          # SGPU_FRAME_NONE
FLOW = 0xABCDEF            # a 3-byte flow value
MAX_PACKET_BYTES = 0x1fffffff
STAT_FRAMES = 22
NSTATS = 23


def load(path):
    L = D.load(path)
    if getattr(L, "_frame_cases", False):
        return L
    # (the two symbols under test: an AttributeError here is the parent's answer)
    L.sgpu_encoder_deliver_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_frames_deliver_recovery.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_frames_send.restype = C.c_longlong
    L.sgpu_frames_send.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.sgpu_gather_wait.argtypes = [C.c_longlong]
    L.sgpu_frames_recv.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                   C.c_void_p]
    L.sgpu_host_alloc.restype = C.c_void_p
    L.sgpu_host_alloc.argtypes = [C.c_size_t]
    L.sgpu_host_free.argtypes = [C.c_void_p]
    L.sgpu_encoder_remove_before.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_decoder_is_ready.argtypes = [C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L._frame_cases = True
    return L


def header(L, kind, flow, num, n):
    out = (C.c_ubyte * 16)()
    h = L.sgpu_frame_write_header(kind, flow, num, n, out)
    assert 1 <= h <= 11
    return bytes(out[:h])


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


class Sender:
    """An encoder holding originals that were added from odd device addresses."""

    def __init__(self, L, lengths, seed=1):
        self.L = L
        self.data = []
        self.enc = L.sgpu_encoder_create()
        assert self.enc
        self.srcs = []
        self.seed = seed
        self.add(lengths)

    def add(self, lengths):
        L = self.L
        first = len(self.data)
        new = [payload(self.seed * 1000 + first + i, n) for i, n in enumerate(lengths)]
        # (an even pitch that is no multiple of 16 and an odd first offset:
        # every source address is odd, their low four bits differ)
        pitch = ((max(lengths) + 34) & ~15) + 2
        blob = bytearray(3 + pitch * len(lengths))
        for i, d in enumerate(new):
            blob[3 + i * pitch:3 + i * pitch + len(d)] = d
        src = L.sgpu_device_alloc(len(blob))
        assert src and L.sgpu_h2d(src, bytes(blob), len(blob)) == 0
        self.srcs.append(src)
        for i, d in enumerate(new):
            at = src + 3 + i * pitch
            assert at & 1
            num = C.c_uint(0)
            assert L.sgpu_encoder_add(self.enc, at, len(d), C.byref(num)) == SUCCESS and num.value == first + i
        self.data += new

    def encode(self, count):
        recs = (Rec * count)()
        made = C.c_uint(0)
        assert self.L.sgpu_encode_range(self.enc, recs, count, C.byref(made)) == SUCCESS
        assert made.value == count
        return recs

    def free(self):
        self.L.sgpu_encoder_free(self.enc)
        assert self.L.sgpu_flush() == 0   # (nothing queued still reads the sources)
        for s in self.srcs:
            self.L.sgpu_device_free(s)


def originals(L, enc, first, count, flow, rows, stride=None, dst=None, lens=None, want=SUCCESS):
    res = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    queued = C.c_uint(12345)
    r = L.sgpu_encoder_deliver_range(enc, first, count, flow, rows.dst if dst is None else dst,
                                     rows.stride if stride is None else stride,
                                     rows.lens if lens is None else lens, res, C.byref(queued))
    assert r == want, "sgpu_encoder_deliver_range returned %d, expected %d" % (r, want)
    return list(res)[:count], queued.value


def recovery(L, recs, count, flows, rows, stride=None, dst=None, lens=None, want=SUCCESS):
    queued = C.c_uint(12345)
    fl = None if flows is None else (C.c_uint * max(1, count))(*flows)
    r = L.sgpu_frames_deliver_recovery(count, recs, fl, rows.dst if dst is None else dst,
                                       rows.stride if stride is None else stride,
                                       rows.lens if lens is None else lens, C.byref(queued))
    assert r == want, "sgpu_frames_deliver_recovery returned %d, expected %d" % (r, want)
    return queued.value


def check_row(row, length, want, what):
    assert length == len(want), "%s: length %d, expected %d" % (what, length, len(want))
    assert row[:len(want)] == want, "%s: header or packet bytes differ" % what
    assert row[len(want):] == bytes(len(row) - len(want)), "%s: tail up to the stride is not zero" % what


# 1, 2 ----------------------------------------------------------------------
# payload lengths where the frame header (7 + n reaching 0x80, 0x4000) and the
# symbol prefix (n reaching 0x80, 0x4000) change width ...
EDGE_N = [1, 120, 121, 127, 128, 16376, 16377, 16383, 16384]
# ... and row contents T = h + n on the 16-byte lane, 1 KiB tile and 8 KiB
# chunk edges: h = 8 up to n = 120, 9 up to n = 16376
EDGE_T = [15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193]
EDGE_LENGTHS = EDGE_N + [t - (8 if t - 8 <= 120 else 9) for t in EDGE_T]
EDGE_STRIDE = 16400


def check_original_edges(path, framed):
    L = load(path)
    sn = Sender(L, EDGE_LENGTHS, seed=11)
    count = len(EDGE_LENGTHS)
    want = [(header(L, ORIGINAL, FLOW, k, len(d)) if framed else b"") + d for k, d in enumerate(sn.data)]
    if framed:
        assert sorted(len(w) for w in want[len(EDGE_N):]) == EDGE_T
        assert {len(w) - len(d) for w, d in zip(want, sn.data)} == {8, 9, 10}
    rows = Rows(L, count, EDGE_STRIDE)
    res, queued = originals(L, sn.enc, 0, count, FLOW if framed else NONE, rows)   # (same submission as the adds)
    assert res == [SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k, w in enumerate(want):
        check_row(got[k], lens[k], w, "original %d (%d bytes)" % (k, len(sn.data[k])))
    rows.free()
    sn.free()


# 3, 4 ----------------------------------------------------------------------
def footer_bytes(L, nOriginals, count):
    """FooterBytes of the first `count` recovery packets of a fresh encoder
    over nOriginals originals: the footer encodes the row's metadata, which
    does not depend on the originals' lengths."""
    sn = Sender(L, [32] * nOriginals, seed=2)
    recs = sn.encode(count)
    out = [recs[k].FooterBytes for k in range(count)]
    sn.free()
    return out


def prefix_bytes(n):
    return 1 if n < 0x80 else 2 if n < 0x4000 else 3


def longest_for(dataBytes, footer):
    """The longest original for which a recovery packet has DataBytes."""
    for p in (1, 2, 3):
        n = dataBytes - footer - p
        if n >= 1 and prefix_bytes(n) == p:
            return n
    raise AssertionError(dataBytes)


def sent_frames(L, recs, count, flows):
    """What sgpu_frames_send writes for the packets: one byte string each."""
    cap = sum(((recs[k].DataBytes + 8 + 15) & ~15) for k in range(count))
    pinned = L.sgpu_host_alloc(cap)
    assert pinned
    used = C.c_size_t(0)
    t = L.sgpu_frames_send(count, recs, (C.c_uint * count)(*flows), pinned, cap, C.byref(used))
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    raw = C.string_at(pinned, used.value)
    L.sgpu_host_free(pinned)
    out, at = [], 0
    for k in range(count):
        n = len(header(L, RECOVERY, flows[k], 0, recs[k].DataBytes)) + recs[k].DataBytes
        out.append(raw[at:at + n])
        assert raw[at + n:(at + n + 15) & ~15] == bytes(((at + n + 15) & ~15) - at - n)
        at = (at + n + 15) & ~15
    assert at == used.value
    return out


def check_recovery_framed(path):
    """Recovery packets encoded in the submission that frames them, against
    sgpu_frames_send of the same packets after it."""
    L = load(path)
    nOrig, per = 6, 3
    f0 = footer_bytes(L, nOrig, 1)[0]
    # 4 + DataBytes of each encoder's first packet on both sides of 0x80, 0x4000
    targets = [0x7f - 4, 0x80 - 4, 0x3fff - 4, 0x4000 - 4]
    senders, packs = [], []
    for i, want in enumerate(targets):
        longest = longest_for(want, f0)
        sn = Sender(L, [longest] + [1 + (longest * (k + 3)) // 11 for k in range(nOrig - 1)], seed=30 + i)
        senders.append(sn)
    senders.append(Sender(L, [777], seed=39))   # a window of one original: the Head path
    stride = 16400
    total = per * len(targets) + 1
    rows = Rows(L, total, stride)
    at = 0
    for i, sn in enumerate(senders):
        n = 1 if i == len(targets) else per
        recs = sn.encode(n)
        flows = [FLOW - 7 * i - k for k in range(n)]
        assert recovery(L, recs, n, flows, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at) == n
        packs.append((recs, n, flows, at))
        at += n
    assert at == total
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    firsts = [4 + packs[i][0][0].DataBytes for i in range(len(targets))]
    assert firsts == [0x7f, 0x80, 0x3fff, 0x4000], firsts
    assert packs[-1][0][0].DataBytes == 2 + 777 + packs[-1][0][0].FooterBytes
    for i, (recs, n, flows, at) in enumerate(packs):
        for k, w in enumerate(sent_frames(L, recs, n, flows)):
            assert w[:len(w) - recs[k].DataBytes] == header(L, RECOVERY, flows[k], 0, recs[k].DataBytes)
            check_row(got[at + k], lens[at + k], w, "encoder %d recovery packet %d" % (i, k))
    rows.free()
    for sn in senders:
        sn.free()


def check_recovery_bare(path):
    """flows == NULL: the bare packets, one of them filling its row."""
    L = load(path)
    stride = 1408
    f = footer_bytes(L, 6, 1)[0]
    a = Sender(L, [700, 13, 699, 250, 1, 480], seed=41)
    b = Sender(L, [longest_for(stride, f), 9, 100, 1000, 64, 333], seed=42)
    rows = Rows(L, 4, stride)
    ra = a.encode(3)
    rb = b.encode(1)
    assert recovery(L, ra, 3, None, rows) == 3
    # (SGPU_FRAME_NONE in a flow list is the same as no list)
    assert recovery(L, rb, 1, [NONE], rows, dst=rows.dst + 3 * stride, lens=rows.lens + 12) == 1
    assert L.sgpu_flush() == 0
    assert rb[0].DataBytes == stride, "the fourth packet must fill its row"
    got, lens = rows.fetch()
    for k, r in enumerate([ra[0], ra[1], ra[2], rb[0]]):
        check_row(got[k], lens[k], D.read(L, r.DeviceData, r.DataBytes), "recovery packet %d" % k)
    rows.free()
    a.free()
    b.free()


# 5 -------------------------------------------------------------------------
def check_round_trip(path):
    """Sender rows -> host copy -> sgpu_frames_recv -> decode -> every original."""
    L = load(path)
    lengths = [40 + (i * 97) % 1300 for i in range(24)]
    lost = (2, 5, 9, 17)
    nrec = 6
    stride = 1360
    sn = Sender(L, lengths, seed=51)
    nrows = len(lengths) - len(lost) + nrec
    rows = Rows(L, nrows, stride)
    at = 0
    # the surviving originals, run by run (flow 0: decoders[0])
    runs, start = [], 0
    for k in sorted(lost) + [len(lengths)]:
        if k > start:
            runs.append((start, k - start))
        start = k + 1
    for first, n in runs:
        res, queued = originals(L, sn.enc, first, n, 0, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at)
        assert res == [SUCCESS] * n and queued == n
        at += n
    recs = sn.encode(nrec)
    assert recovery(L, recs, nrec, [0] * nrec, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at) == nrec
    assert at + nrec == nrows
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert all(0 < v <= stride for v in lens)
    wire = b"".join(got)
    host = L.sgpu_host_alloc(len(wire))
    assert host
    C.memmove(host, wire, len(wire))
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    results = (C.c_int * nrows)(*([-1] * nrows))
    n = C.c_uint(0)
    assert L.sgpu_frames_recv(decs, 1, host, rows.dst, len(wire), results, nrows, C.byref(n)) == SUCCESS
    assert n.value == nrows and list(results) == [SUCCESS] * nrows
    assert L.sgpu_decoder_is_ready(dec) == SUCCESS
    out, m = C.c_void_p(), C.c_uint(0)
    assert L.sgpu_decode(dec, C.byref(out), C.byref(m)) == SUCCESS and m.value == len(lost)
    back = Rows(L, len(lengths), 1344)
    res, queued = D.deliver(L, dec, 0, len(lengths), back)
    assert res == [SUCCESS] * len(lengths) and queued == len(lengths)
    assert L.sgpu_flush() == 0
    got, lens = back.fetch()
    for k, d in enumerate(sn.data):
        D.check_row(got[k], lens[k], d, "original %d%s" % (k, " (lost)" if k in lost else ""))
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    L.sgpu_host_free(host)
    back.free()
    rows.free()
    sn.free()


# 6 -------------------------------------------------------------------------
def check_absent(path):
    L = load(path)
    lengths = [300 + 7 * i for i in range(20)]
    stride = 512
    sn = Sender(L, lengths, seed=61)
    rows = Rows(L, 10, stride)
    blank = bytes([FILL]) * stride

    def want(k):
        return header(L, ORIGINAL, 5, k, len(sn.data[k])) + sn.data[k]

    # past the newest packet
    s0 = stats(L)
    res, queued = originals(L, sn.enc, 15, 10, 5, rows)
    assert res == [SUCCESS] * 5 + [NEED_MORE] * 5 and queued == 5
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_FRAMES] - s0[STAT_FRAMES] == 10
    got, lens = rows.fetch()
    for k in range(10):
        if k < 5:
            check_row(got[k], lens[k], want(15 + k), "original %d" % (15 + k))
        else:
            assert lens[k] == 0 and got[k] == blank, "absent original %d: row touched or length set" % (15 + k)
    # the stream goes on: the same rows again, all present now
    sn.add([440 + 7 * i for i in range(5)])
    res, queued = originals(L, sn.enc, 15, 10, 5, rows)
    assert res == [SUCCESS] * 10 and queued == 10
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k in range(10):
        check_row(got[k], lens[k], want(15 + k), "original %d, second delivery" % (15 + k))
    # before the oldest packet
    rows.refill()
    assert L.sgpu_encoder_remove_before(sn.enc, 8) == SUCCESS
    s0 = stats(L)
    res, queued = originals(L, sn.enc, 4, 8, 5, rows)
    assert res == [NEED_MORE] * 4 + [SUCCESS] * 4 and queued == 4
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_FRAMES] - s0[STAT_FRAMES] == 8
    got, lens = rows.fetch()
    for k in range(8):
        if k < 4:
            assert lens[k] == 0 and got[k] == blank, "removed original %d: row touched or length set" % (4 + k)
        else:
            check_row(got[k], lens[k], want(4 + k), "original %d" % (4 + k))
    assert lens[8:] == [0xA5A5A5A5] * 2 and got[8:] == [blank] * 2
    rows.free()
    sn.free()


# 7 -------------------------------------------------------------------------
def check_arguments(path):
    L = load(path)
    sn = Sender(L, [1400, 200, 300, 400], seed=71)
    rs = Sender(L, [900, 200, 300, 400], seed=72)   # (its recovery packets fit the rows by far)
    recs = rs.encode(3)
    assert L.sgpu_flush() == 0
    rows = Rows(L, 4, 1408)
    assert all(8 + recs[k].DataBytes < rows.stride for k in range(3))
    s0 = stats(L)
    rowArgs = [
        ("null rows", dict(dst=0)),
        ("null lengths", dict(lens=0)),
        ("rows not 16-byte aligned", dict(dst=rows.dst + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=1400)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("lengths not 4-byte aligned", dict(lens=rows.lens + 2)),
    ]
    for what, kw in rowArgs:
        _, queued = originals(L, sn.enc, 1, 3, FLOW, rows, want=INVALID, **kw)
        assert queued == 0, what
        assert recovery(L, recs, 3, [1, 2, 3], rows, want=INVALID, **kw) == 0, what
    for what, kw in [("null encoder", dict(enc=None)), ("flow above 2^24 - 1", dict(flow=1 << 24)),
                     ("first packet number past the maximum", dict(first=PACKET_NUM_MAX + 1))]:
        _, queued = originals(L, kw.get("enc", sn.enc), kw.get("first", 1), 3, kw.get("flow", FLOW), rows,
                              want=INVALID)
        assert queued == 0, what
    # a row one byte too short: 9 + 1400 = 1408 + 1 framed, while the bare payload fits
    assert len(header(L, ORIGINAL, FLOW, 0, 1400)) + 1400 == rows.stride + 1
    _, queued = originals(L, sn.enc, 0, 4, FLOW, rows, want=INVALID)
    assert queued == 0
    # the recovery call: every packet is checked before any is queued
    assert recovery(L, None, 3, [1, 2, 3], rows, want=INVALID) == 0, "null packets"
    assert recovery(L, recs, 3, [1, 1 << 24, 3], rows, want=INVALID) == 0, "flow above 2^24 - 1"

    def spoiled(**kw):
        bad = (Rec * 3)()
        for k in range(3):
            C.memmove(C.byref(bad[k]), C.byref(recs[k]), C.sizeof(Rec))
        for name, v in kw.items():
            setattr(bad[1], name, v)   # (the one in the middle of the list)
        return bad

    for what, kw in [("null DeviceData", dict(DeviceData=None)), ("null Producer", dict(Producer=None)),
                     ("DataBytes zero", dict(DataBytes=0)), ("DataBytes too large", dict(DataBytes=MAX_PACKET_BYTES + 1))]:
        assert recovery(L, spoiled(**kw), 3, [1, 2, 3], rows, want=INVALID) == 0, what
        assert recovery(L, spoiled(**kw), 3, None, rows, want=INVALID) == 0, what
    # h + n == stride + 1 for the packet in the middle: framed (h = 6) and bare
    assert recovery(L, spoiled(DataBytes=rows.stride - 5), 3, [1, 2, 3], rows, want=INVALID) == 0
    assert recovery(L, spoiled(DataBytes=rows.stride + 1), 3, None, rows, want=INVALID) == 0
    # nothing was queued by any of them
    assert L.sgpu_flush() == 0
    s1 = stats(L)
    assert (s1[0], s1[1], s1[STAT_FRAMES]) == (s0[0], s0[1], s0[STAT_FRAMES])
    assert rows.untouched()
    # count == 0
    _, queued = originals(L, sn.enc, 0, 0, FLOW, rows)
    assert queued == 0
    _, queued = originals(L, sn.enc, 0, 0, FLOW, rows, dst=0, lens=0)
    assert queued == 0
    assert recovery(L, recs, 0, None, rows) == 0
    assert recovery(L, None, 0, None, rows, dst=0, lens=0) == 0
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_FRAMES] == s0[STAT_FRAMES] and rows.untouched()
    # (the arguments were fine otherwise)
    res, queued = originals(L, sn.enc, 1, 3, FLOW, rows)
    assert queued == 3
    assert recovery(L, recs, 1, [9], rows, dst=rows.dst + 3 * rows.stride, lens=rows.lens + 12) == 1
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k in range(3):
        check_row(got[k], lens[k], header(L, ORIGINAL, FLOW, 1 + k, len(sn.data[1 + k])) + sn.data[1 + k],
                  "original %d" % (1 + k))
    check_row(got[3], lens[3], header(L, RECOVERY, 9, 0, recs[0].DataBytes) + D.read(L, recs[0].DeviceData, recs[0].DataBytes),
              "recovery packet 0")
    rows.free()
    rs.free()
    sn.free()


# 8 -------------------------------------------------------------------------
def check_many_instances(path, gpu):
    """64 encoders framed by one launch of one submission, and a submission
    that carries nothing but a redelivery."""
    L = load(path)
    per, nrec, size, stride = 4, 2, 1400, 1424

    def run(n, framing):
        senders = [Sender(L, [size] * per, seed=800 + i) for i in range(n)]
        each = per + nrec
        rows = Rows(L, n * each, stride)
        s0 = stats(L)
        packs = []
        for i, sn in enumerate(senders):
            recs = sn.encode(nrec)
            packs.append(recs)
            if framing:
                at = i * each
                res, queued = originals(L, sn.enc, 0, per, i, rows, dst=rows.dst + at * stride, lens=rows.lens + 4 * at)
                assert res == [SUCCESS] * per and queued == per
                at += per
                assert recovery(L, recs, nrec, [i] * nrec, rows, dst=rows.dst + at * stride,
                                lens=rows.lens + 4 * at) == nrec
        assert L.sgpu_flush() == 0
        s1 = stats(L)
        if framing:
            got, lens = rows.fetch()
            for i, sn in enumerate(senders):
                for k in range(per):
                    check_row(got[i * each + k], lens[i * each + k], header(L, ORIGINAL, i, k, size) + sn.data[k],
                              "encoder %d original %d" % (i, k))
                for k in range(nrec):
                    r = packs[i][k]
                    check_row(got[i * each + per + k], lens[i * each + per + k],
                              header(L, RECOVERY, i, 0, r.DataBytes) + D.read(L, r.DeviceData, r.DataBytes),
                              "encoder %d recovery packet %d" % (i, k))
        else:
            assert rows.untouched()
        rows.free()
        for sn in senders:
            sn.free()
        return [b - a for a, b in zip(s0, s1)]

    one = [run(1, False), run(1, True)]
    many = [run(64, False), run(64, True)]
    for plain, framed in (one, many):
        assert plain[0] == framed[0] == 1, "one submission each"
        assert plain[STAT_FRAMES] == 0
    assert one[1][STAT_FRAMES] == per + nrec and many[1][STAT_FRAMES] == 64 * (per + nrec)
    assert one[1][1] - one[0][1] == 1, "the frames of a submission are one launch"
    assert many[1][1] - many[0][1] == one[1][1] - one[0][1], "64 encoders' frames take the launches of one"

    # a submission whose only work is a redelivery of originals already held
    sn = Sender(L, [64, 1400, 333], seed=88)
    assert L.sgpu_flush() == 0
    rows = Rows(L, 3, stride)
    L.sgpu_timing(1, 1, None, None)
    t0 = L.sgpu_enqueue()                # (nothing queued: the latest ticket)
    assert t0 >= 0
    res, queued = originals(L, sn.enc, 0, 3, FLOW, rows)
    assert res == [SUCCESS] * 3 and queued == 3
    t1 = L.sgpu_enqueue()
    assert t1 > t0, "a framing-only submission must take a ticket"
    assert L.sgpu_wait(t1) == 0
    got, lens = rows.fetch()
    for k, d in enumerate(sn.data):
        check_row(got[k], lens[k], header(L, ORIGINAL, FLOW, k, len(d)) + d, "original %d" % k)
    ms = (C.c_double * 7)()
    L.sgpu_timing_kernels(ms, 7)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[6] > 0, "k_frame's device time is timing index 6"
    rows.free()
    sn.free()
