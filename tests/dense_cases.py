"""sgpu_frames_scan_dense / sgpu_frames_recv_dense: the cases shared by
test_dense_cpu.py (the CPU test double, tests/hostsim) and test_dense_gpu.py
(k_walkd, k_rowsum and k_compact on the MI355X), driven through the C ABI with
ctypes.

The yardstick is existing code, never the code under test: the expected dense
buffer of every case is built here (dense_from_packed) from the bytes
sgpu_frames_scan_packed writes for the same rows with the same maxFrames, which
test_pack_* pin against sgpu_frames_parse, and the whole pinned buffer is
compared byte for byte -- info, the words, the starts, the padding and the zero
tail -- between two guard records pre-filled with 0xA5.  For routing a second
set of decoders is fed by sgpu_frames_recv_packed, and the two sets must agree.

The row counts at which k_rowsum's carry scheme takes another path come from
the kernel's constants in siamese_amd/csrc/ops.h (kernel_constants).
"""
import ctypes as C
import os
import random
import re
import struct

import deliver_cases as D
import pack_cases as P
import scan_cases as K
from deliver_cases import FILL, INVALID, NEED_MORE, SUCCESS, payload
from frame_cases import ORIGINAL, RECOVERY, Sender
from pack_cases import REC, frame, row_of
from scan_cases import DevRows
from siamese_amd.binding import PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, PackedHead, bind_dense_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_DENSE = 36
NSTATS = 37
TIMING_WALK, TIMING_ROWSUM, TIMING_COMPACT, NTIMING = 8, 15, 16, 17
DECODER_STATS = 11


def kernel_constants():
    """k_walkd's, k_rowsum's and k_compact's launch constants, read from ops.h."""
    with open(os.path.join(ROOT, "siamese_amd", "csrc", "ops.h")) as f:
        src = f.read()

    def value(name):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m, "%s not found in ops.h" % name
        return int(m.group(1))

    return dict(walk=value("kWalkThreads"), threads=value("kRowsumThreads"), rows=value("kRowsumRows"),
                compact=value("kCompactThreads"))


KC = kernel_constants()
WAVE_ROWS = 64 * KC["rows"]             # the rows of one wave of a k_rowsum pass
PASS_ROWS = KC["threads"] * KC["rows"]  # the rows of one pass: the carry crosses here
BASE_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257]
EDGE_COUNTS = sorted(set(BASE_COUNTS + [b + d for b in (KC["walk"], WAVE_ROWS, PASS_ROWS, 2 * PASS_ROWS)
                                        for d in (-1, 0, 1)]))


def load(path):
    L = P.load(path)
    if getattr(L, "_dense_cases", False):
        return L
    # (the four symbols under test: an AttributeError here is the parent's answer)
    bind_dense_abi(L)
    L.sgpu_decoder_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    L._dense_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


def records_offset(count):
    return (16 + 4 * count + 4 * (count + 1) + 15) & ~15


def packed_raw(L, dev, stride, lens, count, m):
    """The bytes sgpu_frames_scan_packed writes for these rows (guards checked)."""
    o = P.Out(L, count, m)
    t = L.sgpu_frames_scan_packed(dev, stride, lens, count, m, o.out)
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    o.fetch()
    raw = C.string_at(o.out, o.total)
    o.free()
    return raw


def packed_words(raw, count, m):
    w0 = count * m * REC
    return list(struct.unpack_from("<%dI" % count, raw, w0))


def dense_from_packed(raw, count, m, maxRecords):
    """The dense buffer the issue's contract asks for, from the packed scan's
    bytes: (buffer, T, W, c)."""
    words = packed_words(raw, count, m)
    ns = [w & PACKED_COUNT_MASK for w in words]
    assert max(ns) <= m
    starts = [0]
    for n in ns:
        starts.append(starts[-1] + n)
    T = starts[count]
    c = max(k for k in range(count + 1) if starts[k] <= maxRecords)
    W = starts[c]
    head = struct.pack("<4I", T, W, c, 0) + struct.pack("<%dI" % count, *words) + \
        struct.pack("<%dI" % (count + 1), *starts)
    head += bytes(records_offset(count) - len(head))
    recs = b"".join(raw[k * m * REC:(k * m + ns[k]) * REC] for k in range(c))
    assert len(recs) == W * REC
    return head + recs + bytes((maxRecords - W) * REC), T, W, c


class Out:
    """A dense scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxRecords):
        self.L = L
        self.total = L.sgpu_frames_dense_bytes(count, maxRecords)
        assert self.total == records_offset(count) + maxRecords * REC
        assert L.sgpu_frames_dense_records(count) == records_offset(count)
        self.bytes = self.total + 2 * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the output was written"
        assert raw[-REC:] == guard, "guard record after the records was written"
        return raw[REC:-REC]

    def untouched(self):
        return C.string_at(self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_host_free(self.base)


def scan(L, dev, stride, lens, count, m, maxRecords):
    """(the output's bytes, Out) of one dense scan."""
    o = Out(L, count, maxRecords)
    t = L.sgpu_frames_scan_dense(dev, stride, lens, count, m, maxRecords, o.out)
    assert t > 0, "sgpu_frames_scan_dense returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return o.fetch(), o


def first_difference(got, want, count):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    part = ("info" if at < 16 else "row words" if at < 16 + 4 * count else
            "starts" if at < 16 + 4 * (2 * count + 1) else "padding" if at < records_offset(count) else
            "record %d" % ((at - records_offset(count)) // REC))
    return "first difference at byte %d (%s): %r, expected %r" % (at, part, got[at:at + 8], want[at:at + 8])


def check_dense(L, dev, stride, lens, count, m, maxRecords=None, raw=None):
    """One dense scan against the packed scan of the same rows; maxRecords None:
    the total (at least maxFrames).  Returns (T, W, c, the output's bytes)."""
    raw = raw or packed_raw(L, dev, stride, lens, count, m)
    if maxRecords is None:
        maxRecords = max(m, sum(w & PACKED_COUNT_MASK for w in packed_words(raw, count, m)))
    want, T, W, c = dense_from_packed(raw, count, m, maxRecords)
    got, o = scan(L, dev, stride, lens, count, m, maxRecords)
    o.free()
    assert got == want, "count %d, maxFrames %d, maxRecords %d: %s" % (count, m, maxRecords,
                                                                        first_difference(got, want, count))
    return T, W, c, got


def small_frame(rnd, num):
    if rnd.randrange(4) == 0:
        return frame(RECOVERY, num & 0xff, 0, rnd.randbytes(rnd.randrange(1, 10)))
    return frame(ORIGINAL, num & 0xff, num & 0x3fffff, rnd.randbytes(rnd.randrange(1, 4)))


def mixed_rows(count, stride, m, seed, fill=None):
    """count rows of 0..m frames each (fill: that many in every row), at gaps of
    0..2 bytes: (rows, lens, frames per row)."""
    rnd = random.Random(seed)
    rows, lens, ns = [], [], []
    for k in range(count):
        n = rnd.randrange(m + 1) if fill is None else fill
        parts = []
        for j in range(n):
            parts += [rnd.randrange(3), small_frame(rnd, k * m + j)]
        row, end = row_of(parts, stride)
        rows.append(row)
        lens.append(end)
        ns.append(n)
    return rows, lens, ns


# 1 -------------------------------------------------------------------------
def check_row_counts(path, count):
    """A fixed-seed mix of 0..maxFrames frames per row at one row count, with and
    without the length words, at maxRecords = T and at its maximum."""
    L = load(path)
    stride, m = 64, 4
    rows, lens, ns = mixed_rows(count, stride, m, 1000 + count)
    dr = DevRows(L, rows, stride, lens)
    for lp in (dr.lens, None):
        raw = packed_raw(L, dr.dev, stride, lp, count, m)
        T, W, c, _ = check_dense(L, dr.dev, stride, lp, count, m, raw=raw)
        assert (T, W, c) == (sum(ns), sum(ns), count)
    check_dense(L, dr.dev, stride, dr.lens, count, m, maxRecords=count * m)
    dr.free()


# 2 -------------------------------------------------------------------------
def check_degenerate(path):
    """Every row empty, every row full, and a single full row among empty ones
    at the first and last position and on both sides of each wave and workgroup
    boundary of the three kernels.  The rows always hold their frames: a zero
    length word is what makes a row empty, so the stale frames must stay hidden."""
    L = load(path)
    stride, m = 64, 4
    count = PASS_ROWS + 70
    rows, lens, ns = mixed_rows(count, stride, m, 77, fill=m)
    dr = DevRows(L, rows, stride, lens)
    # every row full, with and without the lengths
    for lp in (dr.lens, None):
        T, W, c, _ = check_dense(L, dr.dev, stride, lp, count, m)
        assert (T, W, c) == (count * m, count * m, count)

    def set_lens(live):
        lraw = b"".join((lens[k] if k in live else 0).to_bytes(4, "little") for k in range(count))
        assert L.sgpu_h2d(dr.lens, lraw, len(lraw)) == 0

    # every row empty
    set_lens(())
    T, W, c, got = check_dense(L, dr.dev, stride, dr.lens, count, m)
    assert (T, W, c) == (0, 0, count) and got[records_offset(count):] == bytes(m * REC)
    # one full row
    at = [0, 63, 64, KC["walk"] - 1, KC["walk"], WAVE_ROWS - 1, WAVE_ROWS, KC["threads"] - 1, KC["threads"],
          PASS_ROWS - 1, PASS_ROWS, count - 1]
    for k in at:
        set_lens((k,))
        T, W, c, got = check_dense(L, dr.dev, stride, dr.lens, count, m)
        assert (T, W, c) == (m, m, count), "the full row at %d" % k
        starts = struct.unpack_from("<%dI" % (count + 1), got, 16 + 4 * count)
        assert starts[k] == 0 and starts[k + 1] == m
    dr.free()


# 3 -------------------------------------------------------------------------
def check_cut(path):
    """Rows are all or nothing at maxRecords = maxFrames, T, T - 1 and in the
    middle of a wave; the rescan loop from row c reproduces the one-shot result."""
    L = load(path)
    stride, m, count = 64, 4, 200
    rows, lens, ns = mixed_rows(count, stride, m, 31)
    full = mixed_rows(1, stride, m, 32, fill=m)   # the last row is full: at T - 1 it drops out whole
    rows[-1], lens[-1], ns[-1] = full[0][0], full[1][0], m
    dr = DevRows(L, rows, stride, lens)
    raw = packed_raw(L, dr.dev, stride, dr.lens, count, m)
    starts = [sum(ns[:k]) for k in range(count + 1)]
    T = starts[count]
    cutRow = next(k for k in range(100, count) if ns[k] >= 2)   # a row of the second wave
    mid = starts[cutRow] + 1                                    # ... cut between its records
    for maxRecords in (m, T, T - 1, mid):
        gotT, W, c, got = check_dense(L, dr.dev, stride, dr.lens, count, m, maxRecords=maxRecords, raw=raw)
        assert gotT == T and W <= maxRecords and W == starts[c]
        assert c == count or starts[c + 1] > maxRecords, "c is the largest value with start[c] <= maxRecords"
        assert c >= 1
        tail = got[records_offset(count) + W * REC:]
        assert tail == bytes(len(tail)), "the slots of the rows that dropped out are zero"
    assert check_dense(L, dr.dev, stride, dr.lens, count, m, maxRecords=T - 1, raw=raw)[2] == count - 1
    assert check_dense(L, dr.dev, stride, dr.lens, count, m, maxRecords=mid, raw=raw)[2] == cutRow

    # the rescan loop
    oneT, oneW, oneC, one = check_dense(L, dr.dev, stride, dr.lens, count, m, maxRecords=T, raw=raw)
    assert oneC == count
    wantWords = one[16:16 + 4 * count]
    wantRecs = one[records_offset(count):records_offset(count) + T * REC]
    for room in (m, 37, 64):
        done, words, recs, scans = 0, b"", b"", 0
        while done < count:
            left = count - done
            maxRecords = min(room, left * m)
            _, W, c, got = check_dense(L, dr.dev + done * stride, stride, dr.lens + 4 * done, left, m,
                                       maxRecords=maxRecords)
            assert c >= 1
            words += got[16:16 + 4 * c]
            recs += got[records_offset(left):records_offset(left) + W * REC]
            done += c
            scans += 1
        assert scans > 1 and (words, recs) == (wantWords, wantRecs), "room for %d records per scan" % room
    dr.free()


# 4 -------------------------------------------------------------------------
def flag_rows(stride, m):
    """Rows whose words carry flags, between good ones: (rows, lens, expected words)."""
    good = [frame(ORIGINAL, 0, 10 + k, payload(20 + k, 3 + k)) for k in range(m + 1)]
    rows, lens, words = [], [], []

    def add(parts, word, length=None):
        row, end = row_of(parts, stride)
        rows.append(row)
        lens.append(end if length is None else length)
        words.append(word)

    add(good[:2], 2)
    add(good[:2] + [1, bytes([24, 2, 0, 0, 0]) + payload(5, 20)], 2 | PACKED_MALFORMED)   # type 2 after good ones
    add(good[:3], 3)
    add(good[:m + 1], m | PACKED_MORE)
    add(good[:m], m)
    add(good[:2], PACKED_MALFORMED, length=stride + 16)                                   # deviceLens[k] > stride
    add(good[:1], 1)
    add([bytes([1, ORIGINAL])], PACKED_MALFORMED)                                          # malformed at once
    add(good[1:3], 2)
    return rows, lens, words


def recv(L, decs, out, m, maxRecords, dev, stride, count):
    res = (C.c_int * maxRecords)(*([-1] * maxRecords))
    nrows, n = C.c_uint(12345), C.c_uint(12345)
    r = L.sgpu_frames_recv_dense(decs, len(decs), out, m, maxRecords, dev, stride, count, res, C.byref(nrows),
                                 C.byref(n))
    return r, list(res), nrows.value, n.value


def check_flags(path):
    """A malformed frame after good ones, SGPU_PACKED_MORE at maxFrames and a
    length above the stride: the words are the packed scan's, the good frames
    before the stop are in the dense list and reach the decoder."""
    L = load(path)
    stride, m = 128, 4
    rows, lens, words = flag_rows(stride, m)
    count = len(rows)
    dr = DevRows(L, rows, stride, lens)
    raw = packed_raw(L, dr.dev, stride, dr.lens, count, m)
    assert packed_words(raw, count, m) == words, "the case's own expectation of the packed scan"
    T, W, c, got = check_dense(L, dr.dev, stride, dr.lens, count, m, raw=raw)
    assert (T, W, c) == (sum(w & PACKED_COUNT_MASK for w in words), T, count)
    # routing: packed and dense side by side
    decA, decB = L.sgpu_decoder_create(), L.sgpu_decoder_create()
    po = P.Out(L, count, m)
    C.memmove(po.out, raw, len(raw))
    resA = (C.c_int * (count * m))(*([-1] * (count * m)))
    nA = C.c_uint(0)
    # (the rows repeat packets 10.., so some frames are duplicates: whatever the packed path says of them)
    rA = L.sgpu_frames_recv_packed((C.c_void_p * 1)(decA), 1, po.out, m, dr.dev, stride, count, resA, C.byref(nA))
    assert rA != SUCCESS
    o = Out(L, count, T)
    C.memmove(o.out, got, len(got))
    r, resB, nrows, nB = recv(L, (C.c_void_p * 1)(decB), o.out, m, T, dr.dev, stride, count)
    assert (r, nrows, nB) == (rA, count, nA.value)
    flatA = [resA[k * m + j] for k in range(count) for j in range(words[k] & PACKED_COUNT_MASK)]
    assert resB == flatA
    for num in range(10, 10 + m + 2):
        assert L.sgpu_decoder_has(decA, num) == L.sgpu_decoder_has(decB, num)
    assert decoder_stats(L, decA) == decoder_stats(L, decB)
    assert L.sgpu_decoder_has(decB, 10) == SUCCESS and L.sgpu_decoder_has(decB, 10 + m) == NEED_MORE
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(decA)
    L.sgpu_decoder_free(decB)
    assert L.sgpu_flush() == 0
    po.free()
    o.free()
    dr.free()


def decoder_stats(L, dec):
    v = (C.c_uint64 * DECODER_STATS)()
    assert L.sgpu_decoder_stats(dec, v, DECODER_STATS) == SUCCESS
    return list(v)


# 5 -------------------------------------------------------------------------
def header_offset_rows(stride):
    """pack_cases.check_header_offsets' rows: a second frame of each type at each
    offset 16..31, with prefixes of 1 to 4 bytes."""
    first = frame(ORIGINAL, 0x030201, 9, payload(1, 5))
    rows, lens = [], []
    for kind in (ORIGINAL, RECOVERY):
        for off in range(16, 32):
            for width in (1, 2, 3, 4):
                second = frame(kind, 0xABCDEF - off, 1000 + off, payload(10 * off + width, 20 + width), width)
                row, end = row_of([first, off - len(first), second], stride)
                rows.append(row)
                lens.append(end)
    last = frame(ORIGINAL, 7, 77, payload(3, stride - 16 - 9), 2)
    row, end = row_of([first, 3, last], stride)
    assert end == stride
    return rows + [row], lens + [end]


def recovery_tail_rows(stride):
    """pack_cases.check_recovery_tails' rows: recovery frames of D = 1..9 and 24
    bytes whose last byte lies at each position of an aligned word."""
    first = frame(ORIGINAL, 1, 2, payload(4, 5))
    rows, lens = [], []
    for base in (32, 48):
        for d in P.TAIL_D:
            for e in list(range(1, 16)) + [16]:
                end = base + e
                start = end - 5 - d
                parts = [first, start - len(first)] if start >= 16 else [start]
                row, used = row_of(parts + [frame(RECOVERY, 0x00FACE, 0, payload(100 * d + e, d))], stride)
                assert used == end
                rows.append(row)
                lens.append(end)
    return rows, lens


def check_record_content(path):
    """Headers at every byte offset of a 16-byte word and recovery heads and
    tails of 1..9 and 24 bytes: what the dense walk shares with k_walk."""
    L = load(path)
    for (rows, lens), stride, m in ((header_offset_rows(128), 128, 3), (recovery_tail_rows(64), 64, 2)):
        dr = DevRows(L, rows, stride, lens)
        for lp in (dr.lens, None):
            T, W, c, got = check_dense(L, dr.dev, stride, lp, len(rows), m)
            assert c == len(rows) and T >= len(rows)
        dr.free()


# 6 -------------------------------------------------------------------------
def check_routing(path):
    """Three flows' originals and recovery packets packed by hand, several to a
    row with rows of 0 to 3 frames: decoders A through scan_packed ->
    recv_packed, B through scan_dense -> recv_dense with the rescan loop."""
    L = load(path)
    stride, m = 512, 8
    lengths = [30 + (i * 37) % 90 for i in range(10)]
    lost = {0: (1, 6), 1: (0,), 2: (3, 4, 8)}
    senders = [Sender(L, lengths, seed=170 + f) for f in range(3)]
    frames = [P.wire_frames(L, senders[f], f, [k for k in range(10) if k not in lost[f]], len(lost[f]) + 1)
              for f in range(3)]
    order = []
    for i in range(max(len(x) for x in frames)):
        order += [x[i] for x in frames if i < len(x)]
    rnd = random.Random(16)
    rows, lens, at = [], [], 0
    while at < len(order):
        n = rnd.randrange(4)
        parts = []
        for fr in order[at:at + n]:
            if sum(p if isinstance(p, int) else len(p) for p in parts) + 5 + len(fr) > stride:
                break
            parts += [rnd.randrange(6), fr]
        at += len(parts) // 2
        row, end = row_of(parts, stride)
        rows.append(row)
        lens.append(end)
    count = len(rows)
    dr = DevRows(L, rows, stride, lens)
    total = len(order)

    def decoders():
        return (C.c_void_p * 3)(*[L.sgpu_decoder_create() for _ in range(3)])

    decA, decB = decoders(), decoders()
    raw = packed_raw(L, dr.dev, stride, dr.lens, count, m)
    words = packed_words(raw, count, m)
    assert sum(words) == total and 0 in words
    po = P.Out(L, count, m)
    C.memmove(po.out, raw, len(raw))
    resA = (C.c_int * (count * m))(*([-1] * (count * m)))
    nA = C.c_uint(0)
    assert L.sgpu_frames_recv_packed(decA, 3, po.out, m, dr.dev, stride, count, resA, C.byref(nA)) == SUCCESS
    flatA = [resA[k * m + j] for k in range(count) for j in range(words[k])]

    s0 = stats(L)
    done, flatB, nB, scanned = 0, [], 0, 0
    room = max(m, total // 3)
    while done < count:
        left = count - done
        maxRecords = min(room, left * m)
        got, o = scan(L, dr.dev + done * stride, stride, dr.lens + 4 * done, left, m, maxRecords)
        scanned += left
        r, res, c, n = recv(L, decB, o.out, m, maxRecords, dr.dev + done * stride, stride, left)
        T, W, cc, _ = struct.unpack_from("<4I", got, 0)
        assert (r, c) == (SUCCESS, cc) and c >= 1
        assert res[W:] == [NEED_MORE] * (maxRecords - W), "slots from W on"
        flatB += res[:W]
        nB += n
        done += c
        o.free()
    assert stats(L)[STAT_DENSE] - s0[STAT_DENSE] == scanned > count
    assert flatB == flatA == [SUCCESS] * total and nB == nA.value == total
    for f in range(3):
        for num in range(10):
            want = NEED_MORE if num in lost[f] else SUCCESS
            assert L.sgpu_decoder_has(decA[f], num) == L.sgpu_decoder_has(decB[f], num) == want
        assert decoder_stats(L, decA[f]) == decoder_stats(L, decB[f])
        for dec in (decA[f], decB[f]):
            out, k = C.c_void_p(), C.c_uint(0)
            assert L.sgpu_decoder_is_ready(dec) == SUCCESS
            assert L.sgpu_decode(dec, C.byref(out), C.byref(k)) == SUCCESS and k.value == len(lost[f])
        a, atail = K.delivered(L, decA[f], 10, 128)
        b, btail = K.delivered(L, decB[f], 10, 128)
        assert a == b == senders[f].data and atail == btail
        assert decoder_stats(L, decA[f]) == decoder_stats(L, decB[f])
    assert L.sgpu_flush() == 0
    for f in range(3):
        L.sgpu_decoder_free(decA[f])
        L.sgpu_decoder_free(decB[f])
    assert L.sgpu_flush() == 0
    po.free()
    dr.free()
    for sn in senders:
        sn.free()


# 7 -------------------------------------------------------------------------
def check_arguments(path, gpu):
    """Every refusal with nothing queued and the counter unchanged; count == 0;
    the counter and the timing entries of the one scan that was queued."""
    L = load(path)
    stride, count, m = 64, 4, 2
    built = [row_of([frame(ORIGINAL, 0, k, payload(700 + k, 10 + k)), 3, frame(ORIGINAL, 0, 10 + k, payload(5, 4))],
                    stride) for k in range(count)]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    maxRecords = count * m
    o = Out(L, count, maxRecords)
    dec = L.sgpu_decoder_create()
    decs = (C.c_void_p * 1)(dec)
    assert L.sgpu_flush() == 0
    s0 = stats(L)
    assert L.sgpu_frames_dense_bytes(3, 0) == 0 and L.sgpu_frames_dense_bytes(3, 3 * 256 + 1) == 0
    assert L.sgpu_frames_dense_bytes(0, 1) == 0
    assert L.sgpu_frames_dense_bytes(3, 3 * 256) == 48 + 3 * 256 * 32
    assert [L.sgpu_frames_dense_records(n) for n in (0, 1, 2, 3, 4, 5)] == [32, 32, 48, 48, 64, 64]

    def scan_args(**kw):
        a = dict(rows=dr.dev, stride=stride, lens=dr.lens, count=count, m=m, r=maxRecords, out=o.out)
        a.update(kw)
        return L.sgpu_frames_scan_dense(a["rows"], a["stride"], a["lens"], a["count"], a["m"], a["r"], a["out"])

    rowArgs = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=dr.dev + 8)),
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
                               ("lengths not 4-byte aligned", dict(lens=dr.lens + 2)),
                               ("a packed output above 4 GiB", dict(count=1 << 19, m=256, r=256)),
                               # (36 bytes a row packed, 40 dense: the packed output fits 4 GiB, the dense one does not)
                               ("an output of 4 GiB", dict(count=119304647, m=1, r=119304647))]:
        assert scan_args(**kw) == -1, what
    assert L.sgpu_flush() == 0
    assert o.untouched()
    s1 = stats(L)
    assert (s1[0], s1[1], s1[STAT_DENSE], s1[P.STAT_WALKS]) == (s0[0], s0[1], s0[STAT_DENSE], s0[P.STAT_WALKS])

    L.sgpu_timing(1, 1, None, None)
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_WALK] > 0 and ms[TIMING_ROWSUM] > 0 and ms[TIMING_COMPACT] > 0
        assert ms[7] == 0 and ms[12] == 0, "the dense walk is counted under k_walk's entry"
    got = o.fetch()
    want, T, W, c = dense_from_packed(packed_raw(L, dr.dev, stride, dr.lens, count, m), count, m, maxRecords)
    assert got == want and (T, W, c) == (8, 8, 4)
    s2 = stats(L)
    assert s2[STAT_DENSE] - s1[STAT_DENSE] == count, "only the one valid scan was counted"

    def recv_args(**kw):
        a = dict(decs=decs, heads=o.out, rows=dr.dev, stride=stride, count=count, m=m, r=maxRecords, rowsOut=True)
        a.update(kw)
        n, nrows = C.c_uint(99), C.c_uint(99)
        res = (C.c_int * maxRecords)(*([-1] * maxRecords))
        r = L.sgpu_frames_recv_dense(a["decs"], 1, a["heads"], a["m"], a["r"], a["rows"], a["stride"], a["count"],
                                     res, C.byref(nrows) if a["rowsOut"] else None, C.byref(n))
        return r, n.value, nrows.value if a["rowsOut"] else 0, list(res)

    for what, kw in rowArgs + [("null decoders", dict(decs=None)), ("null output", dict(heads=None)),
                               ("output not 4-byte aligned", dict(heads=o.out + 2)),
                               ("null rowsOut", dict(rowsOut=False))]:
        assert recv_args(**kw) == (INVALID, 0, 0, [-1] * maxRecords), what
    assert L.sgpu_frames_recv_dense(decs, 1, o.out, m, maxRecords, dr.dev, stride, count, None, None, None) == INVALID
    for k in range(count):
        assert L.sgpu_decoder_has(dec, k) == NEED_MORE, "a refused call must not reach the decoder"

    # count == 0: a ticket that is complete, nothing scanned, nothing written; nothing accepted
    before = C.string_at(o.base, o.bytes)
    for kw in (dict(count=0), dict(count=0, r=0), dict(count=0, rows=None, lens=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    assert recv_args(count=0)[:3] == (SUCCESS, 0, 0)
    assert recv_args(count=0, decs=None, heads=None, rows=None)[:3] == (SUCCESS, 0, 0)
    assert L.sgpu_flush() == 0
    s3 = stats(L)
    assert (s3[0], s3[1], s3[STAT_DENSE]) == (s2[0], s2[1], s2[STAT_DENSE]), "nothing was queued by any of them"
    assert C.string_at(o.base, o.bytes) == before

    # (the arguments were fine otherwise)
    assert recv_args() == (SUCCESS, maxRecords, count, [SUCCESS] * maxRecords)
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    dr.free()


# 8 (the CPU double only) ----------------------------------------------------
def check_forged(path):
    """The dense output is caller data: sgpu_frames_recv_dense refuses what no
    scan could have written, routes nothing behind the first start that fails,
    and never touches a record it has not checked (dense_forged_test.cpp runs
    the same forgeries under the sanitizers)."""
    L = load(path)
    stride, m, count = 128, 2, 6
    rows, lens = [], []
    for k in range(count):
        row, end = row_of([frame(ORIGINAL, 0, 50 + k, payload(800 + k, 12 + k)), 1 + k,
                           frame(ORIGINAL, 0, 150 + k, payload(850 + k, 12 + k))], stride)
        rows.append(row)
        lens.append(end)
    dr = DevRows(L, rows, stride, lens)
    maxRecords = count * m
    good, o = scan(L, dr.dev, stride, dr.lens, count, m, maxRecords)
    startAt = 16 + 4 * count
    recAt = records_offset(count)

    def word(at, v):
        return lambda b: b.__setitem__(slice(at, at + 4), struct.pack("<I", v))

    # (what is forged, rows routed before the refusal, frames accepted)
    cases = [
        ("decreasing starts", word(startAt + 4 * 3, 3), 2, 4),
        ("start[0] != 0", word(startAt, 1), 0, 0),
        ("a start difference that disagrees with its word", word(startAt + 4 * 2, 3), 1, 2),
        ("a word that disagrees with its start difference", word(16 + 4 * 4, 1), 4, 8),
        ("c > count", word(8, count + 1), 0, 0),
        ("W > maxRecords", word(4, maxRecords + 1), 0, 0),
        ("W != start[c]", word(4, maxRecords - 1), 5, 10),
        ("a start above W", word(startAt + 4 * count, maxRecords + 2), 5, 10),
    ]
    for what, forge, rowsDone, accepted in cases:
        b = bytearray(good)
        forge(b)
        C.memmove(o.out, bytes(b), len(b))
        dec = L.sgpu_decoder_create()
        r, res, nrows, n = recv(L, (C.c_void_p * 1)(dec), o.out, m, maxRecords, dr.dev, stride, count)
        assert (r, nrows, n) == (INVALID, rowsDone, accepted), "%s: %r" % (what, (r, nrows, n))
        assert res[:accepted] == [SUCCESS] * accepted and res[accepted:] == [NEED_MORE] * (maxRecords - accepted), what
        for k in range(count):
            want = SUCCESS if k < rowsDone else NEED_MORE
            assert L.sgpu_decoder_has(dec, 50 + k) == L.sgpu_decoder_has(dec, 150 + k) == want, what
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
    # a word whose count exceeds maxFrames: a malformed row, none of its records used (as sgpu_frames_recv_packed)
    b = bytearray(good)
    word(16, m + 1)(b)
    C.memmove(o.out, bytes(b), len(b))
    dec = L.sgpu_decoder_create()
    r, res, nrows, n = recv(L, (C.c_void_p * 1)(dec), o.out, m, maxRecords, dr.dev, stride, count)
    assert (r, nrows, n) == (INVALID, count, maxRecords - m)
    assert res == [NEED_MORE] * m + [SUCCESS] * (maxRecords - m)
    assert L.sgpu_decoder_has(dec, 50) == NEED_MORE and L.sgpu_decoder_has(dec, 51) == SUCCESS
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    # a record whose Offset + HeaderBytes + DataBytes passes the stride: that record alone
    b = bytearray(good)
    word(recAt + 3 * REC, stride - 8)(b)
    C.memmove(o.out, bytes(b), len(b))
    dec = L.sgpu_decoder_create()
    r, res, nrows, n = recv(L, (C.c_void_p * 1)(dec), o.out, m, maxRecords, dr.dev, stride, count)
    assert (r, nrows, n) == (INVALID, count, maxRecords - 1)
    assert res == [SUCCESS] * 3 + [INVALID] + [SUCCESS] * (maxRecords - 4)
    assert L.sgpu_decoder_has(dec, 151) == NEED_MORE and L.sgpu_decoder_has(dec, 152) == SUCCESS
    assert L.sgpu_flush() == 0
    L.sgpu_decoder_free(dec)
    assert L.sgpu_flush() == 0
    o.free()
    dr.free()
