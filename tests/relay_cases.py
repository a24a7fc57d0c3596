"""sgpu_decoder_deliver_frames: the cases shared by test_relay_cpu.py (the CPU
test double, tests/hostsim) and test_relay_gpu.py (k_relay on the MI355X),
driven through the C ABI with ctypes.

Expected rows are built here from the originals each case feeds in and
sgpu_frame_write_header, or are the rows sgpu_encoder_deliver_range wrote for
the same packets at the sender.  Every case relays into rows with one guard
row before and one after, lengths with a guard word on each side, everything
pre-filled with 0xA5 (deliver_cases.Rows), and checks that the guards are
intact.
"""
import ctypes as C

import deliver_cases as D
import frame_cases as F
import scan_cases as SC
from deliver_cases import DISABLED, FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, PENDING, SUCCESS, Rows, Stream
from frame_cases import FLOW, NONE, ORIGINAL, Sender, header

STAT_DELIVERS, STAT_FRAMES, STAT_RELAYS = 21, 22, 25
NSTATS = 26
TIMING_RELAY = 9


def load(path):
    L = SC.load(path)
    if getattr(L, "_relay_cases", False):
        return L
    # (the symbol under test: an AttributeError here is the parent's answer)
    L.sgpu_decoder_deliver_frames.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_encode.argtypes = [C.c_void_p, C.c_void_p]
    L._relay_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


def relay(L, dec, flow, first, count, rows, stride=None, dst=None, lens=None, want=SUCCESS):
    res = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    queued = C.c_uint(12345)
    r = L.sgpu_decoder_deliver_frames(dec, flow, first, count, rows.dst if dst is None else dst,
                                      rows.stride if stride is None else stride,
                                      rows.lens if lens is None else lens, res, C.byref(queued))
    assert r == want, "sgpu_decoder_deliver_frames returned %d, expected %d" % (r, want)
    return list(res)[:count], queued.value


def framed(L, flow, num, data):
    return header(L, ORIGINAL, flow, num, len(data)) + data


check_row = F.check_row


# 1 -------------------------------------------------------------------------
# payload lengths around every width change of the symbol's prefix (n reaching
# 0x80, 0x4000) and of the frame's (7 + n reaching 0x80, 0x4000) ...
EDGE_N = [1, 2, 7, 8, 9, 120, 121, 127, 128, 129, 16376, 16377, 16383, 16384, 16385]
# ... and rows whose contents hf + n end on the 16-byte lane, 1 KiB tile and
# 8 KiB chunk edges: hf = 8 up to n = 120, 9 up to n = 16376
EDGE_T = [15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193]
EDGE_LENGTHS = EDGE_N + [t - (8 if t - 8 <= 120 else 9) for t in EDGE_T]
EDGE_STRIDE = 16400


def check_edge_lengths(path):
    L = load(path)
    st = Stream(L, EDGE_LENGTHS, seed=11)
    count = len(EDGE_LENGTHS)
    want = [framed(L, FLOW, k, d) for k, d in enumerate(st.data)]
    assert sorted(len(w) for w in want[len(EDGE_N):]) == EDGE_T
    assert {len(w) - len(d) for w, d in zip(want, st.data)} == {8, 9, 10}
    rows = Rows(L, count, EDGE_STRIDE)
    res, queued = relay(L, st.dec, FLOW, 0, count, rows)
    assert res == [SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k, w in enumerate(want):
        check_row(got[k], lens[k], w, "packet %d (%d bytes)" % (k, len(st.data[k])))
    rows.free()
    st.free()


# 2 -------------------------------------------------------------------------
REC_LOST = (2, 5, 9)
# (symbol prefix, frame header) = (1, 8), (1, 9), (2, 9) for the lost ones
REC_LENGTHS = [dict(zip(REC_LOST, (120, 124, 128))).get(i, 40 + (i * 97) % 1300) for i in range(12)]
REC_STRIDE = 1408


def decode_lost(L, st, device, count):
    """The decode that queues the solve; nothing flushes it."""
    if device:
        r, _ = st.decode(device=True)
        assert r == PENDING
        assert L.sgpu_flush() == 0
        r, n = st.decode(device=True)
    else:
        r, n = st.decode()
    assert (r, n) == (SUCCESS, count), "the fixed loss set must decode: %d, %d packets" % (r, n)


def check_recovered(path, device):
    """Three of twelve originals recovered by a solve of the same submission
    as the relay (sgpu_decode), or through sgpu_decode_device."""
    L = load(path)
    st = Stream(L, REC_LENGTHS, lost=REC_LOST, recovery=4, seed=22)
    shapes = {(F.prefix_bytes(len(st.data[k])), len(header(L, ORIGINAL, 7, k, len(st.data[k])))) for k in REC_LOST}
    assert shapes == {(1, 8), (1, 9), (2, 9)}
    rows = Rows(L, 12, REC_STRIDE)
    decode_lost(L, st, device, len(REC_LOST))
    res, queued = relay(L, st.dec, 7, 0, 12, rows)   # (before any flush of the solve)
    assert res == [SUCCESS] * 12 and queued == 12
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], framed(L, 7, k, d), "packet %d%s" % (k, " (recovered)" if k in REC_LOST else ""))
    rows.free()
    st.free()


# 3, 4 ----------------------------------------------------------------------
HOP_LENGTHS = [dict(zip(REC_LOST, (120, 124, 128))).get(i, 40 + (i * 131) % 1290) for i in range(16)]
HOP_STRIDE = 1344


class Hop:
    """A sender, and a relay's decoder that received all of the sender's
    originals but REC_LOST and four of its recovery packets, has queued the
    solve and has not flushed it."""

    def __init__(self, L, seed):
        self.L = L
        self.sn = Sender(L, HOP_LENGTHS, seed=seed)
        self.count = len(HOP_LENGTHS)
        pitch = ((max(HOP_LENGTHS) + 34) & ~15) + 2   # (Sender.add's)
        self.dec = L.sgpu_decoder_create()
        assert self.dec
        for i, d in enumerate(self.sn.data):
            if i not in REC_LOST:
                assert L.sgpu_decoder_add_original(self.dec, i, self.sn.srcs[0] + 3 + i * pitch, len(d)) == SUCCESS
        self.recs = self.sn.encode(4)
        for k in range(4):
            assert L.sgpu_decoder_add_recovery(self.dec, C.byref(self.recs[k])) == SUCCESS
        out, n = C.c_void_p(), C.c_uint(0)
        assert L.sgpu_decode(self.dec, C.byref(out), C.byref(n)) == SUCCESS and n.value == len(REC_LOST)

    def free(self):
        self.L.sgpu_decoder_free(self.dec)
        self.sn.free()


def check_byte_identity(path):
    """The relay's rows are the sender's rows, byte for byte."""
    L = load(path)
    hop = Hop(L, seed=31)
    sent = Rows(L, hop.count, HOP_STRIDE)
    relayed = Rows(L, hop.count, HOP_STRIDE)
    res, queued = F.originals(L, hop.sn.enc, 0, hop.count, FLOW, sent)
    assert res == [SUCCESS] * hop.count and queued == hop.count
    res, queued = relay(L, hop.dec, FLOW, 0, hop.count, relayed)   # (the solve rides in this submission)
    assert res == [SUCCESS] * hop.count and queued == hop.count
    assert L.sgpu_flush() == 0
    a, alens = sent.fetch()
    b, blens = relayed.fetch()
    assert alens == blens, "the relay's lengths differ from the sender's"
    assert all(0 < v <= HOP_STRIDE for v in blens)
    for k in range(hop.count):
        assert a[k] == b[k], "packet %d%s: the relay's row differs from the sender's" % (
            k, " (recovered)" if k in REC_LOST else "")
    assert b"".join(a) == b"".join(b)
    sent.free()
    relayed.free()
    hop.free()


class Frame(C.Structure):
    _fields_ = [("Type", C.c_uint), ("Flow", C.c_uint), ("PacketNum", C.c_uint), ("Offset", C.c_uint),
                ("Bytes", C.c_uint)]


def check_second_hop(path):
    """The relay's rows into the next hop's decoder without a host copy of a
    payload, and the same buffer through sgpu_frames_parse on the host."""
    L = load(path)
    hop = Hop(L, seed=41)
    count, stride, flow = hop.count, HOP_STRIDE, 0
    rows = Rows(L, count, stride)
    res, queued = relay(L, hop.dec, flow, 0, count, rows)
    assert res == [SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    # the next hop: scan, then receive from the records
    heads, hd = SC.scan(L, rows.dst, stride, rows.lens, count)
    assert heads == [SC.expected(L, r) for r in got]
    nxt = L.sgpu_decoder_create()
    results = (C.c_int * count)(*([-1] * count))
    m = C.c_uint(0)
    assert L.sgpu_frames_recv_rows((C.c_void_p * 1)(nxt), 1, hd.out, rows.dst, stride, count, results,
                                   C.byref(m)) == SUCCESS
    assert m.value == count and list(results) == [SUCCESS] * count
    back, tails = SC.delivered(L, nxt, count, stride)
    assert back == hop.sn.data, "the next hop's packets are the source's"
    assert all(t == bytes(len(t)) for t in tails)
    # the same rows on the host
    wire = b"".join(got)
    out = (Frame * (count + 1))()
    n = C.c_uint(0)
    assert L.sgpu_frames_parse(wire, len(wire), out, count + 1, C.byref(n)) == SUCCESS
    assert n.value == count
    for k in range(count):
        f = out[k]
        assert (f.Type, f.Flow, f.PacketNum, f.Bytes) == (ORIGINAL, flow, k, len(hop.sn.data[k])), "frame %d" % k
        assert wire[f.Offset:f.Offset + f.Bytes] == hop.sn.data[k]
        assert f.Offset == k * stride + lens[k] - f.Bytes
    L.sgpu_decoder_free(nxt)
    assert L.sgpu_flush() == 0
    hd.free()
    rows.free()
    hop.free()


# 5 -------------------------------------------------------------------------
def check_absent(path):
    L = load(path)
    lengths = [300 + 7 * i for i in range(10)]
    lost = (3, 8)
    st = Stream(L, lengths, lost=lost, seed=33)
    rows = Rows(L, 10, 384)
    s0 = stats(L)
    res, queued = relay(L, st.dec, 5, 0, 10, rows)
    assert res == [NEED_MORE if k in lost else SUCCESS for k in range(10)]
    assert queued == 10 - len(lost)
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_RELAYS] - s0[STAT_RELAYS] == 10, "absent packets' items are counted"
    got, lens = rows.fetch()
    for k, d in enumerate(st.data):
        if k in lost:
            assert lens[k] == 0 and got[k] == bytes([FILL]) * 384, "absent packet %d: row touched or length set" % k
        else:
            check_row(got[k], lens[k], framed(L, 5, k, d), "packet %d" % k)
    # the stream fills in: the same buffer again, the rows of before unchanged
    for k in lost:
        assert L.sgpu_decoder_add_original(st.dec, k, st.at(k), lengths[k]) == SUCCESS
    res, queued = relay(L, st.dec, 5, 0, 10, rows)
    assert res == [SUCCESS] * 10 and queued == 10
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], framed(L, 5, k, d), "packet %d, second delivery" % k)
    # a range that starts in the stream and runs past its end
    rows.refill()
    res, queued = relay(L, st.dec, 5, 6, 8, rows)
    assert res == [SUCCESS] * 4 + [NEED_MORE] * 4 and queued == 4
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k in range(4):
        check_row(got[k], lens[k], framed(L, 5, 6 + k, st.data[6 + k]), "packet %d into row %d" % (6 + k, k))
    assert lens[4:8] == [0] * 4 and lens[8:] == [0xA5A5A5A5] * 2
    assert got[4:] == [bytes([FILL]) * 384] * 6
    rows.free()
    st.free()


# 6 -------------------------------------------------------------------------
def check_does_not_fit(path):
    """A recovered 1000-byte packet into rows of 1008: its frame is 1009 bytes.
    Decided on the device while the length is pending, refused by the call
    once it is known; the bare payload fits the same rows."""
    L = load(path)
    st = Stream(L, [100, 1000], lost=(1,), recovery=1, seed=44)
    assert len(framed(L, FLOW, 1, st.data[1])) == 1009
    rows = Rows(L, 2, 1008)
    bare = Rows(L, 2, 1008)
    assert st.decode() == (SUCCESS, 1)
    res, queued = relay(L, st.dec, FLOW, 0, 2, rows)
    assert res == [SUCCESS, SUCCESS] and queued == 2
    res, queued = D.deliver(L, st.dec, 0, 2, bare)   # (the same range, the same submission)
    assert res == [SUCCESS, SUCCESS] and queued == 2
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    check_row(got[0], lens[0], framed(L, FLOW, 0, st.data[0]), "the 100-byte packet")
    assert lens[1] == 0 and got[1] == bytes(1008), "the 1000-byte packet's row must be zero, its length 0"
    got, lens = bare.fetch()
    D.check_row(got[1], lens[1], st.data[1], "the bare 1000-byte packet, rows of 1008")
    # the length is known now
    rows.refill()
    s0 = stats(L)
    _, queued = relay(L, st.dec, FLOW, 0, 2, rows, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_RELAYS] == s0[STAT_RELAYS]
    assert rows.untouched()
    wide = Rows(L, 2, 1024)
    res, queued = relay(L, st.dec, FLOW, 0, 2, wide)
    assert res == [SUCCESS, SUCCESS] and queued == 2
    assert L.sgpu_flush() == 0
    got, lens = wide.fetch()
    check_row(got[0], lens[0], framed(L, FLOW, 0, st.data[0]), "the 100-byte packet, rows of 1024")
    check_row(got[1], lens[1], framed(L, FLOW, 1, st.data[1]), "the 1000-byte packet, rows of 1024")
    for x in (rows, bare, wide):
        x.free()
    st.free()


# 7 -------------------------------------------------------------------------
def dead_decoder(L):
    """A decoder that a corrupt recovered length prefix disabled: the sender
    summed a 1000-byte and a 2-byte original, the decoder was given 488 bytes
    as the first, so the prefix byte recovered for the second is
    0x02 ^ 0x83 ^ 0x81 = 0, a length of zero."""
    sn = Sender(L, [1000, 2], seed=75)
    rec = D.Rec()
    assert L.sgpu_encode(sn.enc, C.byref(rec)) == SUCCESS
    dec = L.sgpu_decoder_create()
    assert L.sgpu_decoder_add_original(dec, 0, sn.srcs[0] + 3, 488) == SUCCESS
    assert L.sgpu_decoder_add_recovery(dec, C.byref(rec)) == SUCCESS
    out, n = C.c_void_p(), C.c_uint(0)
    L.sgpu_decode(dec, C.byref(out), C.byref(n))
    assert L.sgpu_flush() == 0
    return sn, dec


def check_arguments(path):
    L = load(path)
    st = Stream(L, [1400, 200, 300, 400], seed=55)
    rows = Rows(L, 4, 1408)
    s0 = stats(L)
    bad = [
        ("null decoder", dict(dec=None)),
        ("null rows", dict(dst=0)),
        ("null lengths", dict(lens=0)),
        ("rows not 16-byte aligned", dict(dst=rows.dst + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=1400)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("lengths not 4-byte aligned", dict(lens=rows.lens + 2)),
        ("first packet number past the maximum", dict(first=PACKET_NUM_MAX + 1)),
        ("flow above 2^24 - 1", dict(flow=1 << 24)),
        ("SGPU_FRAME_NONE", dict(flow=NONE)),
    ]
    for what, kw in bad:
        dec = kw.pop("dec", st.dec)
        first = kw.pop("first", 1)
        flow = kw.pop("flow", FLOW)
        _, queued = relay(L, dec, flow, first, 3, rows, want=INVALID, **kw)
        assert queued == 0, what
    # a row one byte too short: 9 + 1400 = 1408 + 1 framed, while the bare payload fits
    assert len(framed(L, FLOW, 0, st.data[0])) == rows.stride + 1
    _, queued = relay(L, st.dec, FLOW, 0, 4, rows, want=INVALID)
    assert queued == 0
    bare = Rows(L, 4, 1408)
    res, queued = D.deliver(L, st.dec, 0, 4, bare)
    assert queued == 4
    # a decoder with a device matrix job pending
    job = Stream(L, REC_LENGTHS, lost=REC_LOST, recovery=4, seed=56)
    jrows = Rows(L, 12, REC_STRIDE)
    r, _ = job.decode(device=True)
    assert r == PENDING
    _, queued = relay(L, job.dec, FLOW, 0, 12, jrows, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert job.decode(device=True) == (SUCCESS, len(REC_LOST))
    assert L.sgpu_flush() == 0
    # nothing was queued by any of them
    assert stats(L)[STAT_RELAYS] == s0[STAT_RELAYS]
    assert rows.untouched() and jrows.untouched()
    # count == 0
    _, queued = relay(L, st.dec, FLOW, 0, 0, rows)
    assert queued == 0
    _, queued = relay(L, st.dec, FLOW, 0, 0, rows, dst=0, lens=0)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_RELAYS] == s0[STAT_RELAYS] and rows.untouched()
    # a dead decoder
    sn, dead = dead_decoder(L)
    _, queued = relay(L, dead, FLOW, 0, 2, rows, want=DISABLED)
    assert queued == 0
    _, queued = D.deliver(L, dead, 0, 2, rows, want=DISABLED)   # (as the bare call answers)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert rows.untouched()
    L.sgpu_decoder_free(dead)
    sn.free()
    # (the arguments were fine otherwise: the largest flow)
    res, queued = relay(L, st.dec, (1 << 24) - 1, 1, 3, rows)
    assert res == [SUCCESS] * 3 and queued == 3
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k in range(3):
        check_row(got[k], lens[k], framed(L, (1 << 24) - 1, 1 + k, st.data[1 + k]), "packet %d" % (1 + k))
    assert lens[3] == 0xA5A5A5A5
    for x in (rows, bare, jrows):
        x.free()
    job.free()
    st.free()


# 8 -------------------------------------------------------------------------
def check_many_instances(path, gpu):
    """64 decoders relayed by one launch of one submission, and a submission
    that carries nothing but relay items."""
    L = load(path)
    n, per, size, stride = 64, 8, 1400, 1424
    present = per - 1   # (each range runs one packet past its stream: an absent item)

    def run(relaying):
        streams = [Stream(L, [size] * present, seed=600 + i, pitch=1426) for i in range(n)]
        rows = Rows(L, n * per, stride)
        s0 = stats(L)
        if relaying:
            for i, st in enumerate(streams):
                res, queued = relay(L, st.dec, i, 0, per, rows, dst=rows.dst + i * per * stride,
                                    lens=rows.lens + 4 * i * per)
                assert res == [SUCCESS] * present + [NEED_MORE] and queued == present
        assert L.sgpu_flush() == 0
        s1 = stats(L)
        if relaying:
            got, lens = rows.fetch()
            for i, st in enumerate(streams):
                for k in range(present):
                    check_row(got[i * per + k], lens[i * per + k], framed(L, i, k, st.data[k]),
                              "decoder %d packet %d" % (i, k))
                assert lens[i * per + present] == 0 and got[i * per + present] == bytes([FILL]) * stride
        else:
            assert rows.untouched()
        rows.free()
        for st in streams:
            st.free()
        return [b - a for a, b in zip(s0, s1)]

    plain = run(False)
    with_r = run(True)
    assert plain[0] == with_r[0] == 1, "one submission each"
    assert plain[STAT_RELAYS] == 0 and with_r[STAT_RELAYS] == n * per, "absent items are counted"
    assert with_r[1] == plain[1] + 1, "the relay items of a submission are one launch"
    assert with_r[STAT_DELIVERS] == 0 and with_r[STAT_FRAMES] == 0

    # a submission whose only work is relay items
    lengths = [64, 1400, 333]
    st = Stream(L, lengths, seed=77)
    assert L.sgpu_flush() == 0           # the decoder's earlier work has completed
    rows = Rows(L, 3, stride)
    L.sgpu_timing(1, 1, None, None)
    s0 = stats(L)
    t0 = L.sgpu_enqueue()                # (nothing queued: the latest ticket)
    assert t0 >= 0
    res, queued = relay(L, st.dec, FLOW, 0, 3, rows)
    assert res == [SUCCESS] * 3 and queued == 3
    t1 = L.sgpu_enqueue()
    assert t1 > t0, "a relay-only submission must take a ticket"
    assert L.sgpu_wait(t1) == 0
    s1 = stats(L)
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[STAT_RELAYS] - s0[STAT_RELAYS]) == (1, 1, 3)
    assert s1[STAT_DELIVERS] == s0[STAT_DELIVERS] and s1[STAT_FRAMES] == s0[STAT_FRAMES]
    got, lens = rows.fetch()
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], framed(L, FLOW, k, d), "packet %d" % k)
    ms = (C.c_double * 10)()
    L.sgpu_timing_kernels(ms, 10)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_RELAY] > 0, "k_relay's device time is timing index 9"
        assert ms[5] == 0 and ms[6] == 0, "no k_deliver or k_frame launch carried these items"
    rows.free()
    st.free()
