"""sgpu_decoder_deliver_stream: the cases shared by test_stream_cpu.py (the CPU
test double, tests/hostsim) and test_stream_gpu.py (k_offsets and k_concat on
the MI355X), driven through the C ABI with ctypes.

Expected bytes are built here from the originals each case feeds in: the
concatenation of the payloads and their running sums (expect()).  Nothing
expected comes from the call under test.  Every case delivers to a destination
inside a larger allocation filled with 0xA5 (Dst): the bytes in front of
deviceDst and every byte from B to the allocation's end are checked untouched.
The offsets array (Offs) and the info record (relaypack_cases.Info) have a
16-byte guard on each side.
"""
import ctypes as C
import random

import deliver_cases as D
import relay_cases as R
import relaypack_cases as RP
from deliver_cases import DISABLED, FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, PENDING, SUCCESS, Rows, Stream
from relaypack_cases import Info
from siamese_amd.binding import bind_stream_abi

STAT_DELIVERS, STAT_RELAYS, STAT_PACKS, STAT_STREAMS = 21, 25, 26, 29
NSTATS = 30
TIMING_DELIVER, TIMING_OFFSETS, TIMING_CONCAT = 5, 13, 14
NTIMING = 15
WORD_FILL = 0xA5A5A5A5
FRONT = 64   # guard bytes in front of a destination, before its misalignment


def load(path):
    L = RP.load(path)
    if getattr(L, "_stream_cases", False):
        return L
    # (the symbol under test: an AttributeError here is the parent's answer)
    bind_stream_abi(L)
    L._stream_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


class Dst:
    """`size` destination bytes at misalignment `mis` (0..15) inside an
    allocation of FRONT + 16 + size + 64 bytes, all 0xA5."""

    def __init__(self, L, size, mis=0):
        assert 0 <= mis < 16
        self.L, self.size, self.mis = L, size, mis
        self.bytes = FRONT + 16 + size + 64
        self.base = L.sgpu_device_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.at = self.base + FRONT + mis
        self.refill()

    def refill(self):
        assert self.L.sgpu_h2d(self.base, bytes([FILL]) * self.bytes, self.bytes) == 0

    def check(self, want, what=""):
        """The allocation holds `want` at the destination and 0xA5 everywhere else."""
        raw = D.read(self.L, self.base, self.bytes)
        o = FRONT + self.mis
        assert raw[:o] == bytes([FILL]) * o, "%s: bytes in front of the destination were written" % what
        got = raw[o:o + len(want)]
        if got != want:
            k = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError("%s: stream byte %d of %d is %#x, expected %#x" % (what, k, len(want), got[k], want[k]))
        rest = raw[o + len(want):]
        if rest != bytes([FILL]) * len(rest):
            k = next(i for i in range(len(rest)) if rest[i] != FILL)
            raise AssertionError("%s: byte B + %d behind the stream was written" % (what, k))

    def untouched(self):
        return D.read(self.L, self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_device_free(self.base)


class Offs:
    """count + 1 offset words between two 16-byte guards, all 0xA5."""

    def __init__(self, L, count):
        self.L, self.count = L, count
        self.bytes = 32 + 4 * (count + 1)
        self.base = L.sgpu_device_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.at = self.base + 16
        self.refill()

    def refill(self):
        assert self.L.sgpu_h2d(self.base, bytes([FILL]) * self.bytes, self.bytes) == 0

    def fetch(self):
        raw = D.read(self.L, self.base, self.bytes)
        assert raw[:16] == bytes([FILL]) * 16 and raw[-16:] == bytes([FILL]) * 16, "guards beside the offsets"
        return [int.from_bytes(raw[16 + 4 * k:20 + 4 * k], "little") for k in range(self.count + 1)]

    def untouched(self):
        return self.fetch() == [WORD_FILL] * (self.count + 1)

    def free(self):
        self.L.sgpu_device_free(self.base)


def stream(L, dec, first, count, dst, capacity, offs, info, want=SUCCESS, queuedRef=True, res=True):
    """One call.  dst, offs and info are device addresses."""
    results = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    queued = C.c_uint(12345)
    r = L.sgpu_decoder_deliver_stream(dec, first, count, dst, capacity, offs, info, results if res else None,
                                      C.byref(queued) if queuedRef else None)
    assert r == want, "sgpu_decoder_deliver_stream returned %d, expected %d" % (r, want)
    return list(results)[:count], queued.value


def expect(data, capacity, count=None, invalid=None):
    """(stream bytes, the count + 1 offsets, the info record) for the leading
    present payloads `data` of a range of `count` packets; `invalid`: the
    index of a packet the device must find invalid."""
    count = len(data) if count is None else count
    off, offsets, d, stop = 0, [], 0, 0
    for k, x in enumerate(data):
        if k == invalid:
            stop = 1
            break
        if off + len(x) > capacity:
            stop = 2
            break
        offsets.append(off)
        off += len(x)
        d += 1
    offsets += [off] * (count + 1 - d)
    return b"".join(data[:d]), offsets, [d, off, stop, len(data)]


def check(dst, offs, info, data, capacity, count=None, invalid=None, what="", before=b""):
    """A destination after one call that appended behind `before`."""
    want, offsets, rec = expect(data, capacity, count, invalid)
    assert info.fetch() == rec, "%s: info %r, expected %r" % (what, info.fetch(), rec)
    assert offs.fetch() == offsets, "%s: offsets differ from the running sums" % what
    dst.check(before + want, what)
    return rec


class Call:
    """One queued call with buffers of its own, checked after the flush."""

    def __init__(self, L, dec, first, data, mis, capacity=None, count=None, what=""):
        self.data, self.what = data, what
        self.count = len(data) if count is None else count
        total = sum(len(x) for x in data)
        self.capacity = total if capacity is None else capacity
        self.dst, self.offs, self.info = Dst(L, max(total, self.capacity), mis), Offs(L, self.count), Info(L)
        res, queued = stream(L, dec, first, self.count, self.dst.at, self.capacity, self.offs.at, self.info.at)
        assert res == [SUCCESS] * len(data) + [NEED_MORE] * (self.count - len(data)) and queued == len(data), what

    def check(self):
        rec = check(self.dst, self.offs, self.info, self.data, self.capacity, self.count, what=self.what)
        for x in (self.dst, self.offs, self.info):
            x.free()
        return rec


# 1 -------------------------------------------------------------------------
SHIFT_SHORT = [1, 2, 3, 15, 16, 17, 31, 32, 33]
SHIFT_HS2 = [127, 128, 129]
SHIFT_HS3 = [16383, 16384, 16385]


def check_every_shift(path, lengths, misaligns):
    """One decoder's packets delivered once per misalignment of deviceDst, all
    calls in one submission: every (D - src) mod 16, packets inside one 16-byte
    word and packets that straddle two."""
    L = load(path)
    st = Stream(L, lengths, seed=sum(lengths))
    calls = [Call(L, st.dec, 0, st.data, m, what="lengths %r at misalignment %d" % (lengths, m)) for m in misaligns]
    assert L.sgpu_flush() == 0
    for c in calls:
        assert c.check() == [len(lengths), sum(lengths), 0, len(lengths)]
    st.free()


# 2 -------------------------------------------------------------------------
def check_chunk_edges(path):
    """8191, 8192, 8193 and 16385 bytes behind a 5-byte packet: the 8 KiB chunk
    and 1 KiB tile edges fall inside a packet at an odd destination."""
    L = load(path)
    lengths = [5, 8191, 8192, 8193, 16385]
    st = Stream(L, lengths, seed=92)
    calls = [Call(L, st.dec, 0, st.data, m, what="chunk edges at misalignment %d" % m) for m in (0, 9)]
    assert L.sgpu_flush() == 0
    for c in calls:
        c.check()
    st.free()


# 3 -------------------------------------------------------------------------
def small_lengths(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(1, 41) for _ in range(n)]


def check_scan_wave_edges(path):
    """1, 63, 64, 65 and 129 packets of 1 to 40 bytes: the scan's 64-position
    passes end before, at and after the range's end (position count, the one
    behind the last item, takes part).  With 129 the capacity puts the stop at
    item 0, 63, 64 and 128, one byte short (stop 2); and an exact fit (stop 0,
    B == capacity)."""
    L = load(path)
    for n in (1, 63, 64, 65, 129):
        lengths = small_lengths(400 + n, n)
        st = Stream(L, lengths, seed=400 + n)
        s0 = stats(L)
        calls = [Call(L, st.dec, 0, st.data, 5, what="%d packets, exact fit" % n),
                 Call(L, st.dec, 0, st.data, 11, capacity=sum(lengths) + 1000, what="%d packets, room to spare" % n)]
        stops = (0, 63, 64, 128) if n == 129 else (n - 1,)
        for j in stops:
            calls.append(Call(L, st.dec, 0, st.data, j & 15, capacity=sum(lengths[:j + 1]) - 1,
                              what="%d packets, one byte short at item %d" % (n, j)))
        assert L.sgpu_flush() == 0
        assert stats(L)[STAT_STREAMS] - s0[STAT_STREAMS] == n * len(calls)
        assert calls[0].check() == [n, sum(lengths), 0, n]
        assert calls[0].capacity == sum(lengths)
        assert calls[1].check() == [n, sum(lengths), 0, n]
        for j, c in zip(stops, calls[2:]):
            assert c.check() == [j, sum(lengths[:j]), 2, n]
        st.free()


# 4 -------------------------------------------------------------------------
def check_recovered(path, device):
    """Three of twelve originals recovered by a solve of the same submission as
    the stream (sgpu_decode), or through sgpu_decode_device: their lengths
    exist only on the device when the stream is queued."""
    L = load(path)
    st = Stream(L, R.REC_LENGTHS, lost=R.REC_LOST, recovery=4, seed=22)
    R.decode_lost(L, st, device, len(R.REC_LOST))
    c = Call(L, st.dec, 0, st.data, 13, what="three packets recovered in the submission")   # (before any flush)
    assert L.sgpu_flush() == 0
    assert c.check() == [12, sum(R.REC_LENGTHS), 0, 12]
    st.free()


# 5 -------------------------------------------------------------------------
def check_holes(path):
    L = load(path)
    lengths = [30 + 7 * i for i in range(10)]
    st = Stream(L, lengths, lost=(0, 5), seed=35)
    total = sum(lengths[1:])
    dst, offs, info = Dst(L, total, 7), Offs(L, 10), Info(L)
    # a hole at position 0: p = 0, every offset 0, nothing written
    res, queued = stream(L, st.dec, 0, 10, dst.at, total, offs.at, info.at)
    assert res == [NEED_MORE] * 10 and queued == 0
    assert L.sgpu_flush() == 0
    check(dst, offs, info, [], total, count=10, what="a hole at position 0")
    assert info.fetch() == [0, 0, 0, 0] and offs.fetch() == [0] * 11
    # a hole in the middle: packets 1..4 are the stream, 6..9 are behind the hole
    o9 = Offs(L, 9)
    info.refill()
    res, queued = stream(L, st.dec, 1, 9, dst.at, total, o9.at, info.at)
    assert res == [SUCCESS] * 4 + [NEED_MORE] * 5 and queued == 4
    assert L.sgpu_flush() == 0
    rec = check(dst, o9, info, st.data[1:5], total, count=9, what="a hole at packet 5")
    B = sum(lengths[1:5])
    assert rec == [4, B, 0, 4]
    # the hole fills: the receiver appends at its cursor, deviceDst + B
    assert L.sgpu_decoder_add_original(st.dec, 5, st.at(5), lengths[5]) == SUCCESS
    o5 = Offs(L, 5)
    info.refill()
    res, queued = stream(L, st.dec, 5, 5, dst.at + B, total - B, o5.at, info.at)
    assert res == [SUCCESS] * 5 and queued == 5
    assert L.sgpu_flush() == 0
    rec = check(dst, o5, info, st.data[5:], total - B, what="appended behind the hole", before=b"".join(st.data[1:5]))
    assert rec == [5, total - B, 0, 5]
    for x in (dst, offs, o9, o5, info):
        x.free()
    st.free()


# 6 -------------------------------------------------------------------------
def check_invalid_pending(path):
    """An invalid pending packet.  The technique of deliver_cases.check_too_long
    and relay_cases.check_does_not_fit -- a recovered packet longer than the
    row -- has no counterpart here, where no row bounds a packet: against a
    small capacity it gives stop 2, decided on the device while the length is
    pending and, unlike there, again once it is known (second half below).  A
    prefix that is invalid for this call comes from relay_cases.dead_decoder's
    decoder before its flush: the sender summed a 1000-byte and a 2-byte
    original, the decoder was given 488 bytes as the first, so the prefix byte
    recovered for the second is 0, a length of zero.  The stream queued beside
    that solve stops at it with stop 1, the 488 bytes before it delivered and
    nothing after.  (frames.h concat_plan's stop 1 is covered on its own in
    concat_plan_test.cpp.)"""
    L = load(path)
    sn = R.Sender(L, [1000, 2], seed=75)
    rec = D.Rec()
    assert L.sgpu_encode(sn.enc, C.byref(rec)) == SUCCESS
    dec = L.sgpu_decoder_create()
    assert L.sgpu_decoder_add_original(dec, 0, sn.srcs[0] + 3, 488) == SUCCESS
    assert L.sgpu_decoder_add_recovery(dec, C.byref(rec)) == SUCCESS
    out, n = C.c_void_p(), C.c_uint(0)
    L.sgpu_decode(dec, C.byref(out), C.byref(n))   # (queues the solve; nothing flushes it)
    dst, offs, info = Dst(L, 1024, 3), Offs(L, 2), Info(L)
    res, queued = stream(L, dec, 0, 2, dst.at, 1024, offs.at, info.at)
    assert res == [SUCCESS, SUCCESS] and queued == 2, "the packet being solved counts as present"
    assert L.sgpu_flush() == 0
    first = sn.data[0][:488]
    assert check(dst, offs, info, [first, b"??"], 1024, invalid=1, what="a recovered prefix of length zero") == \
        [1, 488, 1, 2]
    _, queued = stream(L, dec, 0, 2, dst.at, 1024, offs.at, info.at, want=DISABLED)
    assert queued == 0
    L.sgpu_decoder_free(dec)
    sn.free()
    for x in (dst, offs, info):
        x.free()
    # a recovered 1000-byte packet against 600 bytes: stop 2, pending and known
    st = Stream(L, [100, 1000], lost=(1,), recovery=1, seed=44)
    assert st.decode() == (SUCCESS, 1)
    a = Call(L, st.dec, 0, st.data, 1, capacity=600, what="a pending packet that does not fit")
    assert L.sgpu_flush() == 0
    assert a.check() == [1, 100, 2, 2]
    b = Call(L, st.dec, 0, st.data, 1, capacity=600, what="a known packet that does not fit")
    c = Call(L, st.dec, 0, st.data, 1, capacity=1100, what="the same packets, exact fit")
    assert L.sgpu_flush() == 0
    assert b.check() == [1, 100, 2, 2]
    assert c.check() == [2, 1100, 0, 2]
    st.free()


# 7 -------------------------------------------------------------------------
def check_jobs_one_submission(path, gpu):
    """3, 4 and 5 decoders streamed by one submission (four jobs to a workgroup
    of k_offsets) beside a sgpu_decoder_deliver_range of the same packets; and
    a submission that carries nothing but stream jobs."""
    L = load(path)
    streams = [Stream(L, small_lengths(500 + i, 30 + 7 * i) + [1400, 333], seed=500 + i) for i in range(5)]
    assert L.sgpu_flush() == 0
    ms = (C.c_double * NTIMING)()
    for nd in (3, 4, 5):
        s0 = stats(L)
        calls, rows = [], []
        for i in range(nd):
            st = streams[i]
            rw = Rows(L, len(st.data), 1408)
            res, queued = D.deliver(L, st.dec, 0, len(st.data), rw)
            assert res == [SUCCESS] * len(st.data) and queued == len(st.data)
            rows.append(rw)
            calls.append(Call(L, st.dec, 0, st.data, (3 * i + nd) & 15, what="%d jobs, job %d" % (nd, i)))
        assert L.sgpu_flush() == 0
        s1 = stats(L)
        items = sum(len(streams[i].data) for i in range(nd))
        assert s1[0] - s0[0] == 1 and s1[STAT_STREAMS] - s0[STAT_STREAMS] == items
        assert s1[STAT_DELIVERS] - s0[STAT_DELIVERS] == items
        for i, (c, rw) in enumerate(zip(calls, rows)):
            got, lens = rw.fetch()
            assert lens == [len(x) for x in streams[i].data]
            assert b"".join(got[k][:lens[k]] for k in range(len(lens))) == b"".join(c.data), \
                "the stream is the rows' payloads back to back"
            c.check()
            rw.free()
    # nothing but stream jobs
    L.sgpu_timing(1, 1, None, None)
    s0 = stats(L)
    t0 = L.sgpu_enqueue()
    calls = [Call(L, st.dec, 0, st.data, 2 * i + 1, what="stream jobs alone, job %d" % i) for i, st in enumerate(streams)]
    t1 = L.sgpu_enqueue()
    assert t1 > t0, "a submission of stream jobs alone must take a ticket"
    assert L.sgpu_wait(t1) == 0
    s1 = stats(L)
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 2), "one submission, the sum and the copy its only launches"
    assert s1[STAT_STREAMS] - s0[STAT_STREAMS] == sum(len(st.data) for st in streams)
    assert [s1[k] - s0[k] for k in (STAT_DELIVERS, 22, 23, 24, STAT_RELAYS, STAT_PACKS, 27, 28)] == [0] * 8
    for c in calls:
        c.check()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_OFFSETS] > 0 and ms[TIMING_CONCAT] > 0, "k_offsets and k_concat are timing indices 13 and 14"
        # ([0] is k_ingest, which also serves sgpu_gather: the checks above read the buffers back with it)
        assert list(ms)[1:TIMING_OFFSETS] == [0.0] * (TIMING_OFFSETS - 1), "an earlier timing index moved: %r" % list(ms)
    for st in streams:
        st.free()


# 8 -------------------------------------------------------------------------
def check_arguments(path):
    L = load(path)
    st = Stream(L, [1400, 200, 300, 400], seed=55)
    dst, offs, info = Dst(L, 4096, 5), Offs(L, 4), Info(L)
    s0 = stats(L)
    bad = [
        ("null decoder", dict(dec=None)),
        ("null queuedOut", dict(queuedRef=False)),
        ("null offsets", dict(offs=0)),
        ("null info", dict(info=0)),
        ("offsets not 4-byte aligned", dict(offs=offs.at + 2)),
        ("info not 16-byte aligned", dict(info=info.at + 4)),
        ("null destination with a capacity", dict(dst=0)),
        ("capacity of 4 GiB", dict(capacity=1 << 32)),
        ("more than 65535 packets", dict(count=65536)),
        ("first packet number past the maximum", dict(first=PACKET_NUM_MAX + 1)),
    ]
    for what, kw in bad:
        a = dict(dec=st.dec, first=1, count=3, dst=dst.at, capacity=4096, offs=offs.at, info=info.at)
        a.update(kw)
        _, queued = stream(L, a.pop("dec"), a.pop("first"), a.pop("count"), a.pop("dst"), a.pop("capacity"),
                           a.pop("offs"), a.pop("info"), want=INVALID, **a)
        assert queued == (12345 if what == "null queuedOut" else 0), what
    # a decoder with a device matrix job pending
    job = Stream(L, R.REC_LENGTHS, lost=R.REC_LOST, recovery=4, seed=56)
    r, _ = job.decode(device=True)
    assert r == PENDING
    _, queued = stream(L, job.dec, 0, 12, dst.at, 4096, offs.at, info.at, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert job.decode(device=True) == (SUCCESS, len(R.REC_LOST))
    assert L.sgpu_flush() == 0
    # nothing was queued by any of them
    assert stats(L)[STAT_STREAMS] == s0[STAT_STREAMS]
    assert dst.untouched() and offs.untouched() and info.untouched()
    # a dead decoder
    sn, dead = R.dead_decoder(L)
    _, queued = stream(L, dead, 0, 2, dst.at, 4096, offs.at, info.at, want=DISABLED)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert dst.untouched() and offs.untouched() and info.untouched()
    L.sgpu_decoder_free(dead)
    sn.free()
    # count == 0: offsets[0] = 0, a zero info record, nothing copied; with and without a destination
    for kw in (dict(dst=dst.at, capacity=4096), dict(dst=0, capacity=0)):
        _, queued = stream(L, st.dec, 0, 0, kw["dst"], kw["capacity"], offs.at, info.at)
        assert queued == 0
        assert L.sgpu_flush() == 0
        assert info.fetch() == [0, 0, 0, 0] and offs.fetch() == [0] + [WORD_FILL] * 4 and dst.untouched()
        offs.refill()
        info.refill()
    assert stats(L)[STAT_STREAMS] == s0[STAT_STREAMS]
    # (the arguments were fine otherwise: no results array, 65535 packets of which three exist,
    # the largest capacity; a capacity of zero is a full buffer, not an error)
    big = Offs(L, 65535)
    res, queued = stream(L, st.dec, 1, 65535, dst.at, (1 << 32) - 1, big.at, info.at, res=False)
    assert queued == 3
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_STREAMS] - s0[STAT_STREAMS] == 3
    check(dst, big, info, st.data[1:], 4096, count=65535, what="65535 packets, three present")
    dst.refill()
    info.refill()
    res, queued = stream(L, st.dec, 0, 4, 0, 0, offs.at, info.at)
    assert res == [SUCCESS] * 4 and queued == 4
    assert L.sgpu_flush() == 0
    assert info.fetch() == [0, 0, 2, 4] and offs.fetch() == [0] * 5 and dst.untouched()
    for x in (dst, offs, big, info):
        x.free()
    job.free()
    st.free()
