"""sgpu_gather / sgpu_gather_completed / sgpu_gather_async / sgpu_frames_send:
the cases shared by test_gather_cpu.py (the CPU test double, tests/hostsim) and
test_gather_gpu.py (k_ingest's table-less path on the MI355X), driven through
the siamese_gpu.h ABI with ctypes like frame_cases.py.

Every expected byte is a plain Python slice of a blob this file generated
(SHAKE-256 of a seed, no random generator) and uploaded with sgpu_h2d; nothing
is read back through the path under test.  A blob carries SLACK bytes of the
same noise on both sides of what the ranges may name, so the aligned 16-byte
words k_ingest loads around a range stay inside the allocation and a byte that
leaks in from them is not zero.  Every host output is pre-filled with 0xA5 and
has GUARD bytes behind the expected end, which must come back intact.

Frame headers are compared against sgpu_frame_write_header and against
pack_cases.frame, a Python writer of the wire format.
"""
import ctypes as C
import hashlib

import deliver_cases as D
import frame_cases as F
from deliver_cases import FILL, SUCCESS, Rec
from frame_cases import RECOVERY
from pack_cases import frame

GUARD = 64
SLACK = 48                 # (a multiple of 16: ranges keep the allocation's alignment)
CHUNK = 8192               # kIngestChunkBytes
WAVES = 4                  # kIngestWaves
MAX_FRAME_DATA = 4 << 20   # the framed case looks at packets up to here

# the 16-byte lane, kTileBytes (1 KiB), the two tiles of one loop trip, and
# kIngestChunkBytes once and twice
EDGES = [1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 16385]


def load(path):
    L = F.load(path)
    if getattr(L, "_gather_cases", False):
        return L
    L.sgpu_gather_completed.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_gather_async.restype = C.c_longlong
    L.sgpu_gather_async.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_frame_header_bytes.restype = C.c_uint
    L.sgpu_frame_header_bytes.argtypes = [C.c_uint, C.c_uint]
    L.sgpu_encode.argtypes = [C.c_void_p, C.c_void_p]
    L._gather_cases = True
    return L


def align16(n):
    return (n + 15) & ~15


def noise(seed, n):
    return hashlib.shake_256(b"gather:%d" % seed).digest(n)


class Blob:
    """`size` bytes of noise in device memory between two slacks of SLACK
    bytes; at(off) is the device address of byte off, cut(off, n) the bytes a
    range there must give."""

    def __init__(self, L, seed, size):
        self.L, self.size = L, size
        self.host = noise(seed, size + 2 * SLACK)
        self.dev = L.sgpu_device_alloc(len(self.host))
        assert self.dev and self.dev % 16 == 0
        assert L.sgpu_h2d(self.dev, self.host, len(self.host)) == 0

    def at(self, off):
        return self.dev + SLACK + off

    def cut(self, off, n):
        assert 0 <= off and off + n <= self.size, "a range must stay inside the blob"
        return self.host[SLACK + off:SLACK + off + n]

    def free(self):
        self.L.sgpu_device_free(self.dev)


class Out:
    """A host output of n bytes and GUARD more, all 0xA5: page-locked
    (sgpu_host_alloc) or ordinary memory."""

    def __init__(self, L, n, pinned=True):
        self.L, self.n, self.pinned = L, n, pinned
        if pinned:
            self.ptr = L.sgpu_host_alloc(n + GUARD)
            assert self.ptr
        else:
            self.buf = (C.c_ubyte * (n + GUARD))()
            self.ptr = C.addressof(self.buf)
        C.memset(self.ptr, FILL, n + GUARD)

    def check(self, parts, what):
        """parts: (label, expected bytes) back to back from the start; they
        fill the n bytes, and the guard behind them is untouched."""
        raw = C.string_at(self.ptr, self.n + GUARD)
        at = 0
        for label, want in parts:
            got = raw[at:at + len(want)]
            if got != want:
                k = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError("%s: %s differs at its byte %d of %d (output offset %d): got %s, expected %s" % (
                    what, label, k, len(want), at + k, got[k:k + 8].hex(), want[k:k + 8].hex()))
            at += len(want)
        assert at == self.n, "%s: the parts make %d bytes, the output has %d" % (what, at, self.n)
        assert raw[at:] == bytes([FILL]) * GUARD, "%s: bytes behind the expected end (%d) were written" % (what, at)

    def free(self):
        if self.pinned:
            self.L.sgpu_host_free(self.ptr)


class Ranges:
    """A list of (offset, bytes) ranges of one blob, as the three calls take
    and answer it."""

    def __init__(self, blob, ranges):
        self.blob, self.ranges = blob, list(ranges)
        self.count = len(self.ranges)
        n = max(1, self.count)
        self.srcs = (C.c_void_p * n)(*[blob.at(o) for o, _ in self.ranges])
        self.lens = (C.c_uint * n)(*[b for _, b in self.ranges])

    def label(self, i):
        o, n = self.ranges[i]
        return "range %d (%d bytes at alignment %d)" % (i, n, self.blob.at(o) & 15)

    def packed(self):
        """sgpu_gather: the ranges back to back."""
        return [(self.label(i), self.blob.cut(o, n)) for i, (o, n) in enumerate(self.ranges)]

    def padded(self):
        """sgpu_gather_completed / sgpu_gather_async: range i at the sum of
        align16(bytes[k]), zeros up to the next multiple of 16."""
        return [(self.label(i), self.blob.cut(o, n) + bytes(align16(n) - n)) for i, (o, n) in enumerate(self.ranges)]


def total(parts):
    return sum(len(w) for _, w in parts)


def run_gather(L, rg, what):
    want = rg.packed()
    out = Out(L, total(want), pinned=False)
    assert L.sgpu_gather(rg.count, rg.srcs, rg.lens, out.ptr) == 0, what
    out.check(want, what + ", sgpu_gather")
    out.free()


def run_completed(L, rg, what):
    want = rg.padded()
    out = Out(L, total(want))
    assert L.sgpu_gather_completed(rg.count, rg.srcs, rg.lens, out.ptr) == 0, what
    out.check(want, what + ", sgpu_gather_completed")
    out.free()


def run_async(L, rg, what):
    want = rg.padded()
    out = Out(L, total(want))
    t = L.sgpu_gather_async(rg.count, rg.srcs, rg.lens, out.ptr)
    assert t > 0, "%s: sgpu_gather_async returned %d" % (what, t)
    assert L.sgpu_gather_wait(t) == 0, what
    out.check(want, what + ", sgpu_gather_async")
    out.free()


WAYS = {"gather": run_gather, "completed": run_completed, "async": run_async}


# 1, 6 ----------------------------------------------------------------------
LONGEST = 3 * CHUNK + 5    # four chunks of the blockIdx.y grid, the last of 5 bytes


def alignment_ranges(blob_size):
    """Every source alignment 0..15 x every edge length, each at 16 k + a for
    a k of its own; an empty range first and after every seventh; the longest
    range in the middle, in a workgroup with 1-byte neighbours that leave its
    chunk grid at once; a 1-byte range last."""
    ranges = [(5, 0)]
    room = (blob_size - max(max(EDGES), LONGEST) - 16) // 16
    j = 0
    for a in range(16):
        for n in EDGES:
            ranges.append((16 * ((j * 37) % room) + a, n))
            j += 1
            if j % 7 == 0:
                ranges.append((16 * (j % room) + a, 0))
            if j == 8 * len(EDGES):
                ranges += [(16 * 3 + 9, 1), (16 * 11 + 7, LONGEST), (16 * 2 + 14, 1)]
    ranges.append((16 * 77 + 13, 1))
    return ranges


def check_alignment_lengths(path, way, gpu=False):
    """Case 1, and with gpu the path check (case 6): sgpu_gather's copy is
    k_ingest, timing index 0."""
    L = load(path)
    blob = Blob(L, 1, 48 << 10)
    ranges = alignment_ranges(blob.size)
    rg = Ranges(blob, ranges)
    seen = {(blob.at(o) & 15, n) for o, n in ranges if n}
    assert seen >= {(a, n) for a in range(16) for n in EDGES}
    assert max(n for _, n in ranges) >= 3 * CHUNK and ranges[-1][1] == 1
    assert any(ranges[i][1] == 0 and ranges[i - 1][1] and ranges[i + 1][1] for i in range(1, rg.count - 1))
    assert rg.count % WAVES, "the last workgroup must be partly empty"
    timed = gpu and way == "gather"
    ms0, ms1 = (C.c_double * 1)(), (C.c_double * 1)()
    if timed:
        L.sgpu_timing(1, 1, None, None)
        L.sgpu_timing_kernels(ms0, 1)
    WAYS[way](L, rg, "alignments x lengths")
    if timed:
        L.sgpu_timing_kernels(ms1, 1)
        L.sgpu_timing(0, 1, None, None)
        assert ms1[0] > ms0[0], "sgpu_gather did not run k_ingest (timing index 0: %r -> %r)" % (ms0[0], ms1[0])
    blob.free()


# 2 -------------------------------------------------------------------------
def header_steps(L):
    """[(n, h)]: the smallest n in [1, MAX_FRAME_DATA] at which a recovery
    frame's header has h bytes, for every h the library's function returns
    there (it does not decrease with n)."""

    def hb(n):
        return L.sgpu_frame_header_bytes(RECOVERY, n)

    steps = [(1, hb(1))]
    while steps[-1][1] != hb(MAX_FRAME_DATA):
        lo, hi = steps[-1][0], MAX_FRAME_DATA   # hb(lo) == the last h < hb(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if hb(mid) == steps[-1][1]:
                lo = mid
            else:
                hi = mid
        steps.append((hi, hb(hi)))
    return steps


def prefix_width(length):
    """The frame format's own statement of its length prefix (siamese_gpu.h,
    "Framed datagrams"): the fewest of 1-4 bytes, two flag bits in the first."""
    return 1 if length < 0x80 else 2 if length < 0x4000 else 3 if length < 0x200000 else 4


def check_framed(path):
    """Case 2: hand-built packets through sgpu_frames_send, every source
    alignment x every header length x the edge totals."""
    L = load(path)
    steps = header_steps(L)
    sizes = [h for _, h in steps]
    assert sizes == sorted(set(sizes)) and 5 <= sizes[0] and sizes[-1] <= 8, steps
    big = steps[-1][0] if steps[-1][0] > (1 << 16) else 0   # the longest header needs a packet this large
    blob = Blob(L, 2, (big + 64) if big else (40 << 10))

    def hb(n):
        return L.sgpu_frame_header_bytes(RECOVERY, n)

    # packet sizes n: both sides of every step of the header length; totals
    # h + n on the edges (a frame is at least 6 bytes: the total 1 does not
    # exist); and n itself on the edges
    small = set()
    for n, _ in steps[1:]:
        small |= {n - 1, n}
    for t in EDGES:
        small |= {n for n in range(max(1, t - 8), t - 4) if hb(n) + n == t}
    small |= set(EDGES)
    large = sorted(n for n in small if n > (1 << 16))
    small = sorted(n for n in small if n <= (1 << 16))
    assert {hb(n) + n for n in small} >= set(EDGES) - {1}
    packets = []   # (offset, n, flow)
    flows = [0, 1, (1 << 24) - 1]
    room = (blob.size - max(small) - 16) // 16
    j = 0
    for a in range(16):
        for n in small:
            packets.append((16 * ((j * 29) % room) + a, n, flows[j % 3]))
            j += 1
    for n in large:
        # (the longest header at every alignment; its neighbour below the step,
        # whose header length the small packets have at every alignment, at three)
        for a in (range(16) if hb(n) == sizes[-1] else (0, 5, 15)):
            packets.append((a, n, flows[j % 3]))
            j += 1
    assert {(blob.at(o) & 15, hb(n)) for o, n, _ in packets} == {(a, h) for a in range(16) for h in sizes}
    count = len(packets)
    recs = (Rec * count)()
    want = []
    for i, (o, n, flow) in enumerate(packets):
        recs[i].DeviceData = blob.at(o)
        recs[i].DataBytes = n
        data = blob.cut(o, n)
        fr = frame(RECOVERY, flow, 0, data, prefix_width(4 + n))
        h = len(fr) - n
        assert h == hb(n), "packet of %d bytes: the wire format says %d header bytes, the library %d" % (n, h, hb(n))
        assert fr[:h] == F.header(L, RECOVERY, flow, 0, n), "sgpu_frame_write_header(%d bytes, flow %#x)" % (n, flow)
        want.append(("frame %d (header %d + %d bytes from alignment %d, flow %#x)" % (i, h, n, blob.at(o) & 15, flow),
                     fr + bytes(align16(len(fr)) - len(fr))))
    cap = total(want)
    out = Out(L, cap)
    used = C.c_size_t(0)
    t = L.sgpu_frames_send(count, recs, (C.c_uint * count)(*[f for _, _, f in packets]), out.ptr, cap, C.byref(used))
    assert t > 0, "sgpu_frames_send returned %d" % t
    assert used.value == cap, "*bytesOut %d, expected %d" % (used.value, cap)
    assert L.sgpu_gather_wait(t) == 0
    out.check(want, "sgpu_frames_send")
    # one byte of capacity short: refused, nothing written
    C.memset(out.ptr, FILL, cap + GUARD)
    assert L.sgpu_frames_send(count, recs, (C.c_uint * count)(*[f for _, _, f in packets]), out.ptr, cap - 1,
                              C.byref(used)) == -1
    assert C.string_at(out.ptr, cap + GUARD) == bytes([FILL]) * (cap + GUARD)
    out.free()
    blob.free()


# 3 -------------------------------------------------------------------------
def short_ranges(count, blob_size, longest):
    """1..longest bytes at rotating alignments and places."""
    room = (blob_size - longest - 16) // 16
    return [(16 * ((i * 13) % room) + (i * 7 + 3) % 16, 1 + (i * 5) % longest) for i in range(count)]


def check_grid_counts(path):
    """Case 3: counts on both sides of a workgroup (kIngestWaves) and of a wave
    of workgroups, through the packed and the padded way out."""
    L = load(path)
    blob = Blob(L, 3, 4096)
    for count in (1, 3, 4, 5, 63, 64, 65):
        rg = Ranges(blob, short_ranges(count, blob.size, 40))
        for way in ("gather", "completed", "async"):
            WAYS[way](L, rg, "%d short ranges" % count)
    blob.free()


def check_many_ranges(path, count, way):
    """Case 3: Engine::gather unpacks in chunks of 2048 descriptors."""
    L = load(path)
    blob = Blob(L, 4, 4096)
    rg = Ranges(blob, short_ranges(count, blob.size, 17))
    assert {n for _, n in rg.ranges} == set(range(1, 18)) and {blob.at(o) & 15 for o, _ in rg.ranges} == set(range(16))
    WAYS[way](L, rg, "%d ranges of 1-17 bytes" % count)
    blob.free()


def check_nothing_to_move(path):
    """Case 3: count == 0, and calls whose ranges are all empty: 0 from
    sgpu_gather and sgpu_gather_completed, a ticket that can be waited for
    from sgpu_gather_async, nothing written.  (The empty calls come first and
    four times, one per slot of the gather ring: a slot that has never held
    bytes has no staging area yet.)"""
    L = load(path)
    blob = Blob(L, 5, 256)
    out = Out(L, 0)
    host = Out(L, 0, pinned=False)
    last = 0
    for k in range(4):
        rg = Ranges(blob, [(3 + k, 0), (20, 0), (37, 0)])
        t = L.sgpu_gather_async(rg.count, rg.srcs, rg.lens, out.ptr)
        assert t > last, "three empty ranges: sgpu_gather_async returned %d after ticket %d" % (t, last)
        last = t
        assert L.sgpu_gather_wait(t) == 0
        assert L.sgpu_gather_completed(rg.count, rg.srcs, rg.lens, out.ptr) == 0
        assert L.sgpu_gather(rg.count, rg.srcs, rg.lens, host.ptr) == 0
    rg = Ranges(blob, [])
    assert L.sgpu_gather(0, rg.srcs, rg.lens, host.ptr) == 0
    assert L.sgpu_gather(0, None, None, host.ptr) == 0
    t = L.sgpu_gather_async(0, rg.srcs, rg.lens, out.ptr)
    assert t > last, "count == 0: sgpu_gather_async returned %d after ticket %d" % (t, last)
    assert L.sgpu_gather_wait(t) == 0
    out.check([], "pinned output of calls that move nothing")
    host.check([], "host output of calls that move nothing")
    # (the ring is in order afterwards)
    run_async(L, Ranges(blob, [(1, 17), (2, 0), (35, 1)]), "after the empty calls")
    out.free()
    host.free()
    blob.free()


# 4 -------------------------------------------------------------------------
def check_slot_ring(path):
    """Case 4: nine gathers in flight over the four slots of the ring, one
    wait for the last."""
    L = load(path)
    blob = Blob(L, 6, 20 << 10)
    jobs, tickets = [], []
    for k in range(9):
        n = 3 + k   # (another count, other places and other lengths for every gather)
        room = (blob.size - 2 * CHUNK - 16) // 16
        rg = Ranges(blob, [(16 * ((i * 11 + 5 * k) % room) + (i + 3 * k) % 16,
                            [1, 17, 1025, CHUNK + 1 + k, 100 + k, 2 * CHUNK - k][(i + k) % 6]) for i in range(n)])
        want = rg.padded()
        jobs.append((rg, want, Out(L, total(want))))
    for rg, want, out in jobs:
        tickets.append(L.sgpu_gather_async(rg.count, rg.srcs, rg.lens, out.ptr))
    assert tickets[0] > 0 and all(b > a for a, b in zip(tickets, tickets[1:])), tickets
    assert L.sgpu_gather_wait(tickets[-1]) == 0
    for k, (rg, want, out) in enumerate(jobs):
        out.check(want, "gather %d of nine in flight" % k)
    assert L.sgpu_gather_wait(tickets[0]) == 0 and L.sgpu_gather_wait(tickets[-1]) == 0, "a landed ticket"
    for _, _, out in jobs:
        out.free()
    blob.free()


def check_staging_growth(path):
    """Case 4: a slot's staging area grows past its first 1 MiB, and again
    past 2 MiB, with small gathers before, between (in the other slots and,
    the last, in the grown one) and after; none is waited for before all are
    issued."""
    L = load(path)
    half = (512 << 10) + 1
    blob = Blob(L, 7, half + 32)
    small = [[(7, 100), (40, 1)], [(3, 17)], [(18, 1024), (1, 0), (9, 33)]]
    big3 = [(1, half), (3, half), (15, half)]
    big5 = [(5, half), (7, half), (9, half), (11, half), (13, half)]
    assert sum(align16(n) for _, n in big3) > (1 << 20) and sum(align16(n) for _, n in big5) > (2 << 20)
    # (gathers four apart share a slot: 1, 5 and 9)
    order = [small[0], big3, small[1], small[2], small[0], big5, small[1], small[2], small[0], small[1]]
    jobs, tickets = [], []
    for ranges in order:
        rg = Ranges(blob, ranges)
        want = rg.padded()
        jobs.append((rg, want, Out(L, total(want))))
    for rg, want, out in jobs:
        tickets.append(L.sgpu_gather_async(rg.count, rg.srcs, rg.lens, out.ptr))
    assert tickets[0] > 0 and all(b > a for a, b in zip(tickets, tickets[1:])), tickets
    assert L.sgpu_gather_wait(tickets[-1]) == 0
    for k, (rg, want, out) in enumerate(jobs):
        out.check(want, "gather %d (%d bytes) around the growing ones" % (k, out.n))
        out.free()
    blob.free()


# 5 -------------------------------------------------------------------------
def check_ordering(path):
    """Case 5: a recovery packet is gathered without a wait while the encoder
    that owns it is driven on.  The next sgpu_encode releases the packet's
    buffer and the submissions enqueued right behind the gather may rewrite
    it; the gather's reads are ordered before their device work, so it must
    still deliver the first packet's bytes.

    One-sided: a wrong byte here shows that the ordering was violated, a pass
    does not prove that it holds -- the device may simply have run the gather
    first, and the CPU test double is synchronous, where the case only pins
    the call sequence and the bytes."""
    L = load(path)
    sn = F.Sender(L, [4000 - 37 * i for i in range(16)], seed=91)
    for rnd in range(3):
        first = Rec()
        assert L.sgpu_encode(sn.enc, C.byref(first)) == SUCCESS
        assert L.sgpu_flush() == 0
        n = first.DataBytes
        assert n > 4000
        before = D.read(L, first.DeviceData, n)
        assert before != bytes(n)
        out = Out(L, align16(n))
        srcs, lens = (C.c_void_p * 1)(first.DeviceData), (C.c_uint * 1)(n)
        t = L.sgpu_gather_async(1, srcs, lens, out.ptr)
        assert t > 0
        subs = []
        for _ in range(2):   # (the first releases the buffer, the second may be handed it)
            nxt = Rec()
            assert L.sgpu_encode(sn.enc, C.byref(nxt)) == SUCCESS
            subs.append(L.sgpu_enqueue())
            assert subs[-1] >= 0
        assert L.sgpu_gather_wait(t) == 0
        assert L.sgpu_wait(subs[-1]) == 0
        out.check([("the first packet of round %d" % rnd, before + bytes(align16(n) - n))], "gather before the next encode")
        out.free()
    sn.free()
