"""sgpu_decoder_deliver_range: the cases shared by test_deliver_cpu.py (the
CPU test double, tests/hostsim) and test_deliver_gpu.py (k_deliver on the
MI355X), driven through the C ABI with ctypes.

Expected bytes are the originals each case feeds in.  Every case delivers into
rows with one guard row before and one after, lengths with a guard word on
each side, everything pre-filled with 0xA5, and checks that the guards are
intact.  Rows and lengths are read back with sgpu_gather.
"""
import ctypes as C
import random

SUCCESS, INVALID, NEED_MORE, DISABLED, PENDING = 0, 1, 2, 5, 6
FILL = 0xA5
PACKET_NUM_MAX = 0x3fffff


class Rec(C.Structure):
    _fields_ = [("DeviceData", C.c_void_p), ("DataBytes", C.c_uint), ("FooterBytes", C.c_uint),
                ("Footer", C.c_ubyte * 8), ("Head", C.c_ubyte * 4), ("Producer", C.c_void_p)]


class Orig(C.Structure):
    _fields_ = [("PacketNum", C.c_uint), ("DataBytes", C.c_uint), ("Data", C.c_void_p)]


_libs = {}


def load(path, device=-1):
    """The library at `path`, initialised once per process."""
    if path in _libs:
        return _libs[path]
    L = C.CDLL(path)
    for f in ("sgpu_encoder_create", "sgpu_decoder_create", "sgpu_device_alloc"):
        getattr(L, f).restype = C.c_void_p
    L.sgpu_enqueue.restype = C.c_longlong
    L.sgpu_wait.argtypes = [C.c_longlong]
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_device_free.argtypes = [C.c_void_p]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_encoder_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    L.sgpu_encoder_add_range.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint,
                                         C.c_void_p, C.c_void_p]
    L.sgpu_encode_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    L.sgpu_encoder_free.argtypes = [C.c_void_p]
    L.sgpu_decoder_free.argtypes = [C.c_void_p]
    L.sgpu_decoder_add_original.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    L.sgpu_decoder_add_original_range.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                                  C.c_uint, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_add_recovery.argtypes = [C.c_void_p, C.c_void_p]
    L.sgpu_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_deliver_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    L.sgpu_engine_stats.argtypes = [C.c_void_p]
    L.sgpu_engine_stats_ex.argtypes = [C.c_void_p, C.c_uint]
    assert L.sgpu_init(device) == 0
    _libs[path] = L
    return L


def payload(seed, n):
    return random.Random(seed).randbytes(n)


def read(L, dev, n):
    buf = (C.c_ubyte * n)()
    srcs = (C.c_void_p * 1)(dev)
    lens = (C.c_uint * 1)(n)
    assert L.sgpu_gather(1, srcs, lens, buf) == 0
    return bytes(buf)


class Rows:
    """count rows of `stride` bytes between two guard rows, count length
    words between two guard words (a 16-byte pad each side keeps the words'
    area aligned), all 0xA5."""

    def __init__(self, L, count, stride):
        self.L, self.count, self.stride = L, count, stride
        self.rowBytes = (count + 2) * stride
        self.lenBytes = 32 + 4 * count
        self.base = L.sgpu_device_alloc(self.rowBytes)
        self.lbase = L.sgpu_device_alloc(self.lenBytes)
        assert self.base and self.lbase
        self.dst = self.base + stride
        self.lens = self.lbase + 16
        self.refill()

    def refill(self):
        assert self.L.sgpu_h2d(self.base, bytes([FILL]) * self.rowBytes, self.rowBytes) == 0
        assert self.L.sgpu_h2d(self.lbase, bytes([FILL]) * self.lenBytes, self.lenBytes) == 0

    def fetch(self):
        """(rows, lengths) after checking the guards."""
        raw = read(self.L, self.base, self.rowBytes)
        lraw = read(self.L, self.lbase, self.lenBytes)
        s = self.stride
        guard = bytes([FILL]) * s
        assert raw[:s] == guard, "guard row before the rows was written"
        assert raw[-s:] == guard, "guard row after the rows was written"
        assert lraw[:16] == guard[:16] and lraw[-16:] == guard[:16], "guard words beside the lengths were written"
        rows = [raw[s * (k + 1):s * (k + 2)] for k in range(self.count)]
        lens = [int.from_bytes(lraw[16 + 4 * k:20 + 4 * k], "little") for k in range(self.count)]
        return rows, lens

    def untouched(self):
        rows, lens = self.fetch()
        return all(r == bytes([FILL]) * self.stride for r in rows) and all(v == 0xA5A5A5A5 for v in lens)

    def free(self):
        self.L.sgpu_device_free(self.base)
        self.L.sgpu_device_free(self.lbase)


def deliver(L, dec, first, count, rows, stride=None, dst=None, lens=None, want=SUCCESS):
    res = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    queued = C.c_uint(12345)
    r = L.sgpu_decoder_deliver_range(dec, first, count, rows.dst if dst is None else dst,
                                     rows.stride if stride is None else stride,
                                     rows.lens if lens is None else lens, res, C.byref(queued))
    assert r == want, "deliver_range returned %d, expected %d" % (r, want)
    return list(res)[:count], queued.value


def check_row(row, length, data, what):
    assert length == len(data), "%s: length %d, expected %d" % (what, length, len(data))
    assert row[:len(data)] == data, "%s: payload differs" % what
    assert row[len(data):] == bytes(len(row) - len(data)), "%s: tail up to the stride is not zero" % what


class Stream:
    """Originals in device memory at odd addresses; a decoder that received
    all but `lost`, and (with recovery > 0) an encoder's recovery packets.

    data: the payloads themselves (default: payload(seed * 1000 + i, n)).
    offsets: original i at byte offsets[i] of its pitch slot (default: 3 for
    all).  ranges: the encoder takes the originals by one
    sgpu_encoder_add_range call and the decoder each unbroken stretch of
    received ones by one sgpu_decoder_add_original_range call, both with a
    bytes[] array.  given: {index: bytes} the decoder is handed for those
    received originals in place of the encoder's (solve_cases.py: a damaged
    or shortened packet), from a buffer of their own, by a per-packet
    sgpu_decoder_add_original (a range call's ingest rides on the encoder's
    descriptor and would take the encoder's bytes)."""

    def __init__(self, L, lengths, lost=(), recovery=0, seed=1, pitch=None, data=None, offsets=None, ranges=False,
                 given=None):
        self.L = L
        self.given = dict(given or {})
        assert not (ranges and self.given), "an altered original goes in by a per-packet call"
        assert all(i not in lost and 0 < len(g) <= lengths[i] for i, g in self.given.items())
        self.data = data or [payload(seed * 1000 + i, n) for i, n in enumerate(lengths)]
        assert [len(d) for d in self.data] == list(lengths)
        count = len(lengths)
        self.offsets = offsets or [3] * count
        assert not (ranges and offsets), "a range has one stride"
        # (an even pitch that is no multiple of 16 and an odd first offset:
        # every source address is odd, their low four bits differ)
        self.pitch = pitch or ((max(lengths) + 34) & ~15) + 2
        assert all(o + n <= self.pitch for o, n in zip(self.offsets, lengths))
        blob = bytearray(max(self.offsets) + self.pitch * count)
        for i, d in enumerate(self.data):
            o = self.offsets[i] + i * self.pitch
            blob[o:o + len(d)] = d
        self.src = L.sgpu_device_alloc(len(blob))
        assert self.src and L.sgpu_h2d(self.src, bytes(blob), len(blob)) == 0
        # the decoder's own copies, at odd addresses like the encoder's
        self.alt = None
        if self.given:
            self.altAt = {}
            ablob = bytearray(3 + self.pitch * len(self.given))
            for k, (i, g) in enumerate(sorted(self.given.items())):
                self.altAt[i] = 3 + k * self.pitch
                ablob[self.altAt[i]:self.altAt[i] + len(g)] = g
            self.alt = L.sgpu_device_alloc(len(ablob))
            assert self.alt and L.sgpu_h2d(self.alt, bytes(ablob), len(ablob)) == 0
        lens = (C.c_uint * count)(*lengths)
        self.enc = None
        self.recs = None
        if recovery:
            self.enc = L.sgpu_encoder_create()
            if ranges:
                first, added = C.c_uint(99), C.c_uint(0)
                assert L.sgpu_encoder_add_range(self.enc, self.at(0), self.pitch, lens, 0, count, C.byref(first),
                                                C.byref(added)) == SUCCESS
                assert (first.value, added.value) == (0, count)
            else:
                for i, d in enumerate(self.data):
                    num = C.c_uint(0)
                    assert L.sgpu_encoder_add(self.enc, self.at(i), len(d), C.byref(num)) == SUCCESS
                    assert num.value == i
            self.recs = (Rec * recovery)()
            made = C.c_uint(0)
            assert L.sgpu_encode_range(self.enc, self.recs, recovery, C.byref(made)) == SUCCESS
            assert made.value == recovery
        self.dec = L.sgpu_decoder_create()
        assert self.dec
        if ranges:
            i = 0
            while i < count:
                j = i
                while j < count and j not in lost:
                    j += 1
                if j > i:
                    res = (C.c_int * (j - i))(*([-1] * (j - i)))
                    calls = C.c_uint(0)
                    assert L.sgpu_decoder_add_original_range(
                        self.dec, i, self.at(i), self.pitch, C.byref(lens, 4 * i), 0, j - i, res,
                        C.byref(calls)) == SUCCESS
                    assert calls.value == j - i and list(res) == [SUCCESS] * (j - i)
                i = j + 1
        else:
            for i, d in enumerate(self.data):
                if i in self.given:
                    assert L.sgpu_decoder_add_original(self.dec, i, self.alt + self.altAt[i],
                                                       len(self.given[i])) == SUCCESS
                elif i not in lost:
                    assert L.sgpu_decoder_add_original(self.dec, i, self.at(i), len(d)) == SUCCESS
        for k in range(recovery):
            assert L.sgpu_decoder_add_recovery(self.dec, C.byref(self.recs[k])) == SUCCESS

    def at(self, i):
        return self.src + self.offsets[i] + i * self.pitch

    def decode(self, device=False):
        out = C.c_void_p()
        n = C.c_uint(0)
        f = self.L.sgpu_decode_device if device else self.L.sgpu_decode
        return f(self.dec, C.byref(out), C.byref(n)), n.value

    def free(self):
        if self.enc:
            self.L.sgpu_encoder_free(self.enc)
        self.L.sgpu_decoder_free(self.dec)
        assert self.L.sgpu_flush() == 0   # (nothing queued still reads the sources)
        self.L.sgpu_device_free(self.src)
        if self.alt:
            self.L.sgpu_device_free(self.alt)


def stats(L):
    v = (C.c_uint64 * 22)()
    L.sgpu_engine_stats_ex(v, 22)
    return list(v)


# 1 -------------------------------------------------------------------------
EDGE_LENGTHS = [1, 2, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385]
EDGE_STRIDE = 16400


def check_edge_lengths(path):
    """Prefix widths 1, 2 and 3, the 16-byte lane edges, the 1 KiB tile edges
    and the 8 KiB chunk edge, received packets."""
    L = load(path)
    st = Stream(L, EDGE_LENGTHS, seed=11)
    assert all(st.at(i) & 1 for i in range(len(EDGE_LENGTHS)))
    rows = Rows(L, len(EDGE_LENGTHS), EDGE_STRIDE)
    res, queued = deliver(L, st.dec, 0, len(EDGE_LENGTHS), rows)
    assert res == [SUCCESS] * len(EDGE_LENGTHS) and queued == len(EDGE_LENGTHS)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens == EDGE_LENGTHS
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], d, "packet %d (%d bytes)" % (k, len(d)))
    rows.free()
    st.free()


# 2 -------------------------------------------------------------------------
REC_LENGTHS = [40 + (i * 97) % 1300 for i in range(12)]
REC_LOST = (2, 5, 9)
REC_STRIDE = 1408


def check_recovered(path, device):
    """Three of twelve originals recovered by a solve of the same submission
    as the delivery (sgpu_decode), or through sgpu_decode_device."""
    L = load(path)
    st = Stream(L, REC_LENGTHS, lost=REC_LOST, recovery=4, seed=22)
    rows = Rows(L, 12, REC_STRIDE)
    if device:
        r, _ = st.decode(device=True)
        assert r == PENDING
        assert L.sgpu_flush() == 0
        r, n = st.decode(device=True)
    else:
        r, n = st.decode()
    assert (r, n) == (SUCCESS, len(REC_LOST)), "the fixed loss set must decode: %d, %d packets" % (r, n)
    res, queued = deliver(L, st.dec, 0, 12, rows)   # (before any flush of the solve)
    assert res == [SUCCESS] * 12 and queued == 12
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens == REC_LENGTHS
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], d, "packet %d%s" % (k, " (recovered)" if k in REC_LOST else ""))
    rows.free()
    st.free()


# 3 -------------------------------------------------------------------------
def check_absent(path):
    L = load(path)
    lengths = [300 + 7 * i for i in range(10)]
    lost = (3, 8)
    st = Stream(L, lengths, lost=lost, seed=33)
    rows = Rows(L, 10, 384)
    res, queued = deliver(L, st.dec, 0, 10, rows)
    assert res == [NEED_MORE if k in lost else SUCCESS for k in range(10)]
    assert queued == 10 - len(lost)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k, d in enumerate(st.data):
        if k in lost:
            assert lens[k] == 0 and got[k] == bytes([FILL]) * 384, "absent packet %d: row touched or length set" % k
        else:
            check_row(got[k], lens[k], d, "packet %d" % k)
    # the stream fills in: the same buffer again, the rows of before unchanged
    for k in lost:
        assert L.sgpu_decoder_add_original(st.dec, k, st.at(k), lengths[k]) == SUCCESS
    res, queued = deliver(L, st.dec, 0, 10, rows)
    assert res == [SUCCESS] * 10 and queued == 10
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens == lengths
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], d, "packet %d, second delivery" % k)
    rows.free()
    st.free()


# 4 -------------------------------------------------------------------------
def check_too_long(path):
    """A recovered 1000-byte packet into rows of 512: decided on the device
    while its length is pending, refused by the call once it is known."""
    L = load(path)
    st = Stream(L, [100, 1000], lost=(1,), recovery=1, seed=44)
    rows = Rows(L, 2, 512)
    assert st.decode() == (SUCCESS, 1)
    res, queued = deliver(L, st.dec, 0, 2, rows)
    assert res == [SUCCESS, SUCCESS] and queued == 2
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    check_row(got[0], lens[0], st.data[0], "the 100-byte packet")
    assert lens[1] == 0 and got[1] == bytes(512), "the 1000-byte packet's row must be zero, its length 0"
    rows.refill()
    _, queued = deliver(L, st.dec, 0, 2, rows, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert rows.untouched()
    # (the packet itself is intact: it fits rows of 1008)
    wide = Rows(L, 2, 1008)
    deliver(L, st.dec, 0, 2, wide)
    assert L.sgpu_flush() == 0
    got, lens = wide.fetch()
    check_row(got[1], lens[1], st.data[1], "the 1000-byte packet, rows of 1008")
    wide.free()
    rows.free()
    st.free()


# 5 -------------------------------------------------------------------------
def check_arguments(path):
    L = load(path)
    st = Stream(L, [1400, 200, 300, 400], seed=55)
    rows = Rows(L, 4, 1408)
    small = Rows(L, 4, 512)
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
    ]
    for what, kw in bad:
        dec = kw.pop("dec", st.dec)
        first = kw.pop("first", 0)
        _, queued = deliver(L, dec, first, 4, rows, want=INVALID, **kw)
        assert queued == 0, what
    # a packet whose known length exceeds the stride
    _, queued = deliver(L, st.dec, 0, 4, small, want=INVALID)
    assert queued == 0
    # count == 0
    _, queued = deliver(L, st.dec, 0, 0, rows)
    assert queued == 0
    _, queued = deliver(L, st.dec, 0, 0, rows, dst=0, lens=0)
    assert queued == 0
    # a decoder with a device matrix job pending
    job = Stream(L, REC_LENGTHS, lost=REC_LOST, recovery=4, seed=56)
    jrows = Rows(L, 12, REC_STRIDE)
    r, _ = job.decode(device=True)
    assert r == PENDING
    _, queued = deliver(L, job.dec, 0, 12, jrows, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert job.decode(device=True) == (SUCCESS, len(REC_LOST))
    assert L.sgpu_flush() == 0
    assert rows.untouched() and small.untouched() and jrows.untouched()
    for x in (rows, small, jrows):
        x.free()
    job.free()
    st.free()


# 6 -------------------------------------------------------------------------
def check_many_instances(path):
    """64 decoders x 8 packets delivered by one launch of one submission."""
    L = load(path)
    n, per, size, stride = 64, 8, 1400, 1408

    def run(with_deliveries):
        streams = [Stream(L, [size] * per, seed=600 + i, pitch=1426) for i in range(n)]
        rows = Rows(L, n * per, stride)
        s0 = stats(L)
        if with_deliveries:
            for i, st in enumerate(streams):
                res, queued = deliver(L, st.dec, 0, per, rows, dst=rows.dst + i * per * stride,
                                      lens=rows.lens + 4 * i * per)
                assert res == [SUCCESS] * per and queued == per
        assert L.sgpu_flush() == 0
        s1 = stats(L)
        if with_deliveries:
            got, lens = rows.fetch()
            assert lens == [size] * (n * per)
            for i, st in enumerate(streams):
                for k in range(per):
                    check_row(got[i * per + k], lens[i * per + k], st.data[k], "decoder %d packet %d" % (i, k))
        else:
            assert rows.untouched()
        rows.free()
        for st in streams:
            st.free()
        return [b - a for a, b in zip(s0, s1)]

    plain = run(False)
    with_d = run(True)
    assert plain[0] == with_d[0] == 1, "one submission each"
    assert plain[21] == 0 and with_d[21] == n * per
    assert with_d[1] == plain[1] + 1, "the deliveries of a submission are one launch"


# 7 -------------------------------------------------------------------------
def check_delivery_only(path):
    """A submission whose only work is delivery items is still a submission."""
    L = load(path)
    lengths = [64, 1400, 333]
    st = Stream(L, lengths, seed=77)
    assert L.sgpu_flush() == 0           # the decoder's earlier work has completed
    rows = Rows(L, 3, 1408)
    t0 = L.sgpu_enqueue()                # (nothing queued: the latest ticket)
    assert t0 >= 0
    res, queued = deliver(L, st.dec, 0, 3, rows)
    assert res == [SUCCESS] * 3 and queued == 3
    t1 = L.sgpu_enqueue()
    assert t1 > t0, "a delivery-only submission must take a ticket"
    assert L.sgpu_wait(t1) == 0
    got, lens = rows.fetch()
    assert lens == lengths
    for k, d in enumerate(st.data):
        check_row(got[k], lens[k], d, "packet %d" % k)
    # the same through the inline flush path
    rows.refill()
    deliver(L, st.dec, 1, 2, rows)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    assert lens[:2] == lengths[1:] and lens[2] == 0xA5A5A5A5
    check_row(got[0], lens[0], st.data[1], "packet 1 into row 0")
    check_row(got[1], lens[1], st.data[2], "packet 2 into row 1")
    assert got[2] == bytes([FILL]) * 1408
    rows.free()
    st.free()
