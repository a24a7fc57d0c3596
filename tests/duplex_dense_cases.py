"""sgpu_frames_scan_duplex_dense / sgpu_frames_recv_duplex_dense: the cases
shared by test_duplex_dense_cpu.py (the CPU test double, tests/hostsim) and
test_duplex_dense_gpu.py (k_ackwalkd, k_rowsum2, k_compact and k_slots on the
MI355X), driven through the C ABI with ctypes.

The yardstick is existing code, never the code under test: the expected buffer
of every case is built here (dense_from_duplex) from the bytes
sgpu_frames_scan_duplex writes for the same rows with the same maxFrames,
ackSlots and ackBytes, which test_ack_walk.py and the ARQ tests pin against
arq_cases.model_row, and the whole pinned buffer is compared byte for byte --
info, the words, both start tables, both paddings, the records, the slots and
the zero tails -- between two guard records pre-filled with 0xA5.  For routing
a twin set of decoders and encoders is fed by sgpu_frames_recv_duplex, and the
two sets must agree.

The row counts at which the kernels take another path come from their constants
in siamese_amd/csrc/ops.h (kernel_constants).
"""
import ctypes as C
import hashlib
import os
import random
import re
import struct
import time

import arq_cases as A
import dense_cases as DN
import pack_cases as P
from arq_cases import ACK, Pair, ack_frame
from deliver_cases import FILL, INVALID, NEED_MORE, SUCCESS, Rows, payload
from frame_cases import ORIGINAL, RECOVERY
from pack_cases import REC, frame, row_of
from scan_cases import DevRows
from siamese_amd.binding import (PACKED_ACKS_DROPPED, PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, ROW_OK,
                                 ROW_TRUNCATED, PackedHead, bind_duplex_dense_abi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_DUPLEX, STAT_DENSE, STAT_DUPLEX_DENSE, NSTATS = 27, 36, 39, 40
TIMING_WALK, TIMING_ACKWALK, TIMING_ROWSUM, TIMING_COMPACT, TIMING_ROWSUM2, TIMING_SLOTS, NTIMING = 8, 12, 15, 16, 17, 18, 19


def kernel_constants():
    """k_ackwalkd's, k_rowsum2's and k_slots' launch constants, read from ops.h."""
    with open(os.path.join(ROOT, "siamese_amd", "csrc", "ops.h")) as f:
        src = f.read()

    def value(name):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m, "%s not found in ops.h" % name
        return int(m.group(1))

    return dict(walk=value("kAckWalkdThreads"), threads=value("kRowsum2Threads"), rows=value("kRowsum2Rows"),
                slots=value("kSlotsThreads"))


KC = kernel_constants()
WAVE_ROWS = 64 * KC["rows"]             # the rows of one wave of a k_rowsum2 pass
PASS_ROWS = KC["threads"] * KC["rows"]  # the rows of one pass: the carry crosses here
BASE_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257]
EDGE_COUNTS = sorted(set(BASE_COUNTS + [b + d for b in (KC["walk"], WAVE_ROWS, PASS_ROWS, 2 * PASS_ROWS)
                                        for d in (-1, 0, 1)]))


def load(path):
    L = A.load(path)
    if getattr(L, "_duplex_dense_cases", False):
        return L
    # (the five symbols under test: an AttributeError here is the parent's answer)
    bind_duplex_dense_abi(L)
    L._duplex_dense_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


def align16(n):
    return (n + 15) & ~15


def records_offset(count):
    return align16(16 + 4 * count + 4 * (count + 1))


def acks_offset(count, maxRecords):
    return records_offset(count) + maxRecords * REC


def slots_offset(count, maxRecords):
    return acks_offset(count, maxRecords) + align16(4 * (count + 1))


def duplex_raw(L, dev, stride, lens, count, m, s, ab):
    """The bytes sgpu_frames_scan_duplex writes for these rows (guards checked)."""
    _, _, _, o = A.scan(L, dev, stride, lens, count, m, s, ab)
    raw = o.raw
    o.free()
    return raw


class Parts:
    """A duplex scan's output taken apart: per row the word, the record count,
    the records' bytes, the slots it uses and those slots' bytes."""

    def __init__(self, raw, count, m, s, ab):
        self.words = list(struct.unpack_from("<%dI" % count, raw, count * m * REC))
        self.ns = [w & PACKED_COUNT_MASK for w in self.words]
        assert max(self.ns) <= m
        soff = align16(count * m * REC + 4 * count)
        self.recs, self.aks, self.slots = [], [], []
        for k in range(count):
            r = raw[k * m * REC:(k * m + self.ns[k]) * REC]
            acks = sum(1 for j in range(self.ns[k]) if r[j * REC + 5] == ACK)   # (Type is byte 5 of a record)
            a = min(acks, s)
            self.recs.append(r)
            self.aks.append(a)
            self.slots.append(raw[soff + k * s * ab:soff + (k * s + a) * ab])
        self.starts, self.astarts = [0], [0]
        for k in range(count):
            self.starts.append(self.starts[-1] + self.ns[k])
            self.astarts.append(self.astarts[-1] + self.aks[k])


def dense_from_duplex(raw, count, m, s, ab, maxRecords, maxAcks):
    """The buffer the contract asks for, from the duplex scan's bytes:
    (buffer, T, W, c, WA)."""
    p = raw if isinstance(raw, Parts) else Parts(raw, count, m, s, ab)
    T = p.starts[count]
    c = max(k for k in range(count + 1) if p.starts[k] <= maxRecords and p.astarts[k] <= maxAcks)
    W, WA = p.starts[c], p.astarts[c]
    head = struct.pack("<4I", T, W, c, WA) + struct.pack("<%dI" % count, *p.words) + \
        struct.pack("<%dI" % (count + 1), *p.starts)
    head += bytes(records_offset(count) - len(head))
    recs = b"".join(p.recs[:c])
    assert len(recs) == W * REC
    at = struct.pack("<%dI" % (count + 1), *p.astarts)
    at += bytes(align16(len(at)) - len(at))
    slots = b"".join(p.slots[:c])
    assert len(slots) == WA * ab
    return head + recs + bytes((maxRecords - W) * REC) + at + slots + bytes((maxAcks - WA) * ab), T, W, c, WA


class Out:
    """A dense duplex scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxRecords, maxAcks, ab):
        self.L = L
        self.total = L.sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ab)
        assert self.total == slots_offset(count, maxRecords) + maxAcks * ab
        assert L.sgpu_frames_duplex_dense_acks(count, maxRecords) == acks_offset(count, maxRecords)
        assert L.sgpu_frames_duplex_dense_slots(count, maxRecords) == slots_offset(count, maxRecords)
        self.bytes = self.total + 2 * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the output was written"
        assert raw[-REC:] == guard, "guard record after the slots was written"
        return raw[REC:-REC]

    def untouched(self):
        return C.string_at(self.base, self.bytes) == bytes([FILL]) * self.bytes

    def free(self):
        self.L.sgpu_host_free(self.base)


def scan(L, dev, stride, lens, count, m, s, ab, maxRecords, maxAcks):
    """(the output's bytes, Out) of one dense duplex scan."""
    o = Out(L, count, maxRecords, maxAcks, ab)
    t = L.sgpu_frames_scan_duplex_dense(dev, stride, lens, count, m, s, ab, maxRecords, maxAcks, o.out)
    assert t > 0, "sgpu_frames_scan_duplex_dense returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return o.fetch(), o


def first_difference(got, want, count, maxRecords):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    ro, ao, so = records_offset(count), acks_offset(count, maxRecords), slots_offset(count, maxRecords)
    part = ("info" if at < 16 else "row words" if at < 16 + 4 * count else
            "starts" if at < 16 + 4 * (2 * count + 1) else "padding" if at < ro else
            "record %d" % ((at - ro) // REC) if at < ao else
            "ack starts" if at < ao + 4 * (count + 1) else "ack padding" if at < so else
            "slot byte %d" % (at - so))
    return "first difference at byte %d (%s): %r, expected %r" % (at, part, got[at:at + 8], want[at:at + 8])


def check_dd(L, dev, stride, lens, count, m, s, ab, maxRecords=None, maxAcks=None, parts=None):
    """One dense duplex scan against the duplex scan of the same rows;
    maxRecords, maxAcks None: the totals (at least maxFrames, ackSlots).
    Returns (T, W, c, WA, the output's bytes)."""
    p = parts or Parts(duplex_raw(L, dev, stride, lens, count, m, s, ab), count, m, s, ab)
    if maxRecords is None:
        maxRecords = max(m, p.starts[count])
    if maxAcks is None:
        maxAcks = max(s, p.astarts[count])
    want, T, W, c, WA = dense_from_duplex(p, count, m, s, ab, maxRecords, maxAcks)
    got, o = scan(L, dev, stride, lens, count, m, s, ab, maxRecords, maxAcks)
    o.free()
    assert got == want, "count %d, maxFrames %d, ackSlots %d, ackBytes %d, maxRecords %d, maxAcks %d: %s" % (
        count, m, s, ab, maxRecords, maxAcks, first_difference(got, want, count, maxRecords))
    return T, W, c, WA, got


def small_frame(rnd, num):
    if rnd.randrange(4) == 0:
        return frame(RECOVERY, num & 0xff, 0, rnd.randbytes(rnd.randrange(1, 6)))
    return frame(ORIGINAL, num & 0xff, num & 0x3fffff, rnd.randbytes(rnd.randrange(1, 4)))


def mixed_rows(count, stride, m, s, seed, acks=True):
    """count rows of 0..m frames each, 0..s + 1 of them acks (never more than
    the row's frames) at random places, at gaps of 0..2 bytes:
    (rows, lens, frames per row, acks per row)."""
    rnd = random.Random(seed)
    rows, lens, ns, aks = [], [], [], []
    for k in range(count):
        n = rnd.randrange(m + 1)
        a = min(n, rnd.randrange(s + 2)) if acks else 0
        where = set(rnd.sample(range(n), a))
        parts = []
        for j in range(n):
            fr = ack_frame(k & 0xff, rnd.randbytes(rnd.randrange(1, 6))) if j in where else small_frame(rnd, k * m + j)
            parts += [rnd.randrange(3), fr]
        row, end = row_of(parts, stride)
        rows.append(row)
        lens.append(end)
        ns.append(n)
        aks.append(a)
    return rows, lens, ns, aks


# 1 -------------------------------------------------------------------------
def check_row_counts(path, count):
    """A fixed-seed mix of 0..maxFrames frames and 0..ackSlots + 1 acks per row
    at one row count, with and without the length words, at the totals and at
    both maxima."""
    L = load(path)
    stride, m, s, ab = 64 + 16 * (count % 5), 4, 2, 16
    rows, lens, ns, aks = mixed_rows(count, stride, m, s, 2000 + count)
    dr = DevRows(L, rows, stride, lens)
    for lp in (dr.lens, None):
        T, W, c, WA, _ = check_dd(L, dr.dev, stride, lp, count, m, s, ab)
        assert (T, W, c, WA) == (sum(ns), sum(ns), count, sum(min(a, s) for a in aks))
    check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords=count * m, maxAcks=count * s)
    dr.free()


# 2 -------------------------------------------------------------------------
def check_ack_free(path):
    """Rows without an ack: up to the end of the records the output is
    sgpu_frames_scan_dense's byte for byte, WA = 0, every astart word is 0 and
    every slot is zero."""
    L = load(path)
    DN.load(path)
    stride, m, s, ab = 64, 4, 2, 16
    for count in (1, 70, KC["walk"] + 3):
        rows, lens, ns, _ = mixed_rows(count, stride, m, s, 300 + count, acks=False)
        dr = DevRows(L, rows, stride, lens)
        for maxRecords in sorted({max(m, sum(ns)), max(m, sum(ns) // 2)}):
            maxAcks = min(count * s, s + 3)
            T, W, c, WA, got = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords, maxAcks)
            dense, o = DN.scan(L, dr.dev, stride, dr.lens, count, m, maxRecords)
            o.free()
            assert got[:len(dense)] == dense, "the dense scan's bytes"
            assert len(dense) == L.sgpu_frames_dense_bytes(count, maxRecords) == acks_offset(count, maxRecords)
            assert WA == 0 and got[len(dense):] == bytes(len(got) - len(dense)), "astart words and slots are zero"
        dr.free()


# 3 -------------------------------------------------------------------------
def check_cut(path):
    """Rows are all or nothing under both budgets: maxRecords binds first,
    maxAcks binds first, both at the same row, ack-free rows behind a spent ack
    budget, trailing frameless rows, the minimum; the rescan loop from row c
    reproduces the one-shot result."""
    L = load(path)
    stride, m, s, ab, count = 96, 4, 2, 16, 200
    rows, lens, ns, aks = mixed_rows(count, stride, m, s, 41)
    dr = DevRows(L, rows, stride, lens)
    p = Parts(duplex_raw(L, dr.dev, stride, dr.lens, count, m, s, ab), count, m, s, ab)
    assert p.ns == ns and p.aks == [min(a, s) for a in aks], "the case's own expectation of the duplex scan"
    st, ast = p.starts, p.astarts
    T, TA = st[count], ast[count]

    def cut(maxRecords, maxAcks, wantC):
        gT, W, c, WA, got = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords, maxAcks, parts=p)
        assert (gT, W, WA, c) == (T, st[c], ast[c], wantC), (maxRecords, maxAcks, c, wantC)
        assert c == count or st[c + 1] > maxRecords or ast[c + 1] > maxAcks
        return got

    rowR = next(k for k in range(100, count) if ns[k] >= 2)                  # a row in the middle
    cut(st[rowR] + 1, count * s, rowR)                                      # maxRecords binds first
    rowA = next(k for k in range(70, count) if p.aks[k] >= 1 and ns[k] >= 1)
    cut(count * m, ast[rowA + 1] - 1, rowA)                                 # maxAcks binds first
    cut(st[rowA + 1] - 1, ast[rowA + 1] - 1, rowA)                          # both at the same row
    cut(T, TA, count)
    cut(m, count * s, max(k for k in range(count + 1) if st[k] <= m))
    cut(count * m, s, max(k for k in range(count + 1) if ast[k] <= s))
    dr.free()

    # ack-free rows after the ack budget is spent complete, up to the next row with an ack; trailing
    # frameless rows are included
    data = [frame(ORIGINAL, 1, k, payload(k, 3)) for k in range(8)]
    hand = [[ack_frame(1, b"ab"), data[0]], [data[1]], [], [data[2], data[3]], [ack_frame(2, b"c")], [data[4]], [], []]
    built = [row_of(q, stride) for q in hand]
    dh = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    assert check_dd(L, dh.dev, stride, dh.lens, 8, m, 1, ab, maxRecords=32, maxAcks=1)[1:4] == (5, 4, 1)
    assert check_dd(L, dh.dev, stride, dh.lens, 8, m, 1, ab, maxRecords=32, maxAcks=2)[1:4] == (7, 8, 2)
    assert check_dd(L, dh.dev, stride, dh.lens, 8, m, 1, ab, maxRecords=7, maxAcks=2)[1:4] == (7, 8, 2)
    assert check_dd(L, dh.dev, stride, dh.lens, 8, m, 1, ab, maxRecords=6, maxAcks=2)[1:4] == (6, 5, 2)
    # the minimum: one row completes
    full = [[ack_frame(1, b"x"), ack_frame(1, b"y"), data[0], data[1]], [data[2]], [ack_frame(3, b"z")]]
    built = [row_of(q, stride) for q in full]
    df = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    assert check_dd(L, df.dev, stride, df.lens, 3, m, 2, ab, maxRecords=m, maxAcks=2)[1:4] == (4, 1, 2)
    dh.free()
    df.free()

    # the rescan loop
    dr = DevRows(L, rows, stride, lens)
    _, _, oneC, _, one = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, T, max(s, TA), parts=p)
    assert oneC == count
    ro, so = records_offset(count), slots_offset(count, T)
    want = (one[16:16 + 4 * count], one[ro:ro + T * REC], one[so:so + TA * ab])
    for room, aroom in ((m, s), (37, 64), (64, 5)):
        done, words, recs, slots, scans = 0, b"", b"", b"", 0
        while done < count:
            left = count - done
            mr, ma = min(room, left * m), min(aroom, left * s)
            _, W, c, WA, got = check_dd(L, dr.dev + done * stride, stride, dr.lens + 4 * done, left, m, s, ab, mr, ma)
            assert c >= 1
            words += got[16:16 + 4 * c]
            recs += got[records_offset(left):records_offset(left) + W * REC]
            slots += got[slots_offset(left, mr):slots_offset(left, mr) + WA * ab]
            done += c
            scans += 1
        assert scans > 1 and (words, recs, slots) == want, "room for %d records and %d slots per scan" % (room, aroom)
    dr.free()


def check_cut_far(path):
    """The cut behind the first wave and the first pass of k_rowsum2: maxRecords
    binds in the second pass, maxAcks in the second wave of the first, and each
    binds first in turn with the other close behind in another wave, so c, W and
    WA are reduced over lanes, waves and carries that are not all complete."""
    L = load(path)
    stride, m, s, ab = 64, 4, 2, 16
    count = PASS_ROWS + WAVE_ROWS + 40
    rows, lens, ns, aks = mixed_rows(count, stride, m, s, 59)
    dr = DevRows(L, rows, stride, lens)
    p = Parts(duplex_raw(L, dr.dev, stride, dr.lens, count, m, s, ab), count, m, s, ab)
    st, ast = p.starts, p.astarts
    far, wave2, last = PASS_ROWS + 5, WAVE_ROWS + 70, PASS_ROWS + WAVE_ROWS + 3
    for maxRecords, maxAcks, bound in ((st[far], count * s, far), (count * m, ast[wave2], wave2),
                                       (st[last], ast[far], far), (st[wave2], ast[last], wave2)):
        T, W, c, WA, _ = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords, maxAcks, parts=p)
        # (rows without a frame or an ack behind the bound still complete: c is the last row before one that adds)
        assert bound <= c < count and (W, WA) == (st[c], ast[c]) and (W == st[bound] or WA == ast[bound])
        assert st[c + 1] > maxRecords or ast[c + 1] > maxAcks
    dr.free()


# 4 -------------------------------------------------------------------------
def check_flags(path):
    """SGPU_PACKED_MORE, MALFORMED and ACKS_DROPPED survive in the row words; a
    long ack is truncated into its slot; an ack past ackSlots has a record, no
    slot and no share in astart; a row that turns malformed behind an ack keeps
    that ack's slot; a length above the stride and a zero length."""
    L = load(path)
    stride, m, s, ab = 128, 4, 1, 16
    good = [frame(ORIGINAL, 0, 10 + k, payload(20 + k, 3 + k)) for k in range(m + 1)]
    long_msg = payload(9, ab + 1)
    hand = [
        (good[:2], None, 2, 0),
        (good[:m + 1], None, m | PACKED_MORE, 0),
        (good[:2] + [1, bytes([24, 3, 0, 0, 0]) + payload(5, 20)], None, 2 | PACKED_MALFORMED, 0),
        ([ack_frame(4, long_msg), good[0]], None, 2 | PACKED_ACKS_DROPPED, 1),
        ([ack_frame(1, b"first"), good[0], ack_frame(1, b"second")], None, 3 | PACKED_ACKS_DROPPED, 1),
        ([good[0], ack_frame(6, b"kept"), 2, bytes([1, ORIGINAL])], None, 2 | PACKED_MALFORMED, 1),
        (good[:2], stride + 16, PACKED_MALFORMED, 0),
        ([ack_frame(7, b"hidden"), good[1]], 0, 0, 0),
        (good[1:3], None, 2, 0),
    ]
    built = [row_of(q, stride) for q, _, _, _ in hand]
    lens = [n if h[1] is None else h[1] for (_, n), h in zip(built, hand)]
    count = len(hand)
    dr = DevRows(L, [r for r, _ in built], stride, lens)
    p = Parts(duplex_raw(L, dr.dev, stride, dr.lens, count, m, s, ab), count, m, s, ab)
    assert p.words == [h[2] for h in hand] and p.aks == [h[3] for h in hand], "the case's own expectation"
    T, W, c, WA, got = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, parts=p)
    assert (W, c, WA) == (T, count, 3)
    so, ro = slots_offset(count, max(m, T)), records_offset(count)
    assert got[so:so + 3 * ab] == long_msg[:ab] + b"first" + bytes(ab - 5) + b"kept" + bytes(ab - 4)
    rec = lambda i: P.fields(PackedHead.from_buffer_copy(got, ro + i * REC))
    assert rec(p.starts[3])[1:3] == (ROW_TRUNCATED, ACK) and rec(p.starts[3])[7] == ab + 1
    assert rec(p.starts[4])[1] == ROW_OK and rec(p.starts[4] + 2)[1:3] == (ROW_TRUNCATED, ACK)
    assert rec(p.starts[4] + 2)[6] == 1, "PacketNum is the ack's number within its row"
    # cut in the middle: the same flags in the words, fewer rows complete
    T2, W2, c2, WA2, _ = check_dd(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords=max(m, T), maxAcks=2, parts=p)
    assert (c2, WA2) == (5, 2)
    dr.free()


# 5 -------------------------------------------------------------------------
def slot_rows(ab, stride):
    """Messages that start at every byte 0..15 of a 16-byte word, of 1, 15, 16,
    17, ackBytes - 1, ackBytes and ackBytes + 1 bytes; every third row holds a
    second and a third ack, every fifth an original first."""
    rows, lens = [], []
    sizes = sorted({1, 15, 16, 17, ab - 1, ab, ab + 1})
    i = 0
    for size in sizes:
        for gap in range(16):
            parts = [gap, ack_frame(gap, payload(1000 * size + gap, size), 2)]
            if i % 3 == 0:
                parts += [i % 4, ack_frame(1, payload(i, 2)), ack_frame(2, payload(i + 1, 5))]
            if i % 5 == 0:
                parts = [frame(ORIGINAL, 3, i, payload(i, 4))] + parts
            row, end = row_of(parts, stride)
            rows.append(row)
            lens.append(end)
            i += 1
    return rows, lens


def check_slot_content(path):
    """ackBytes 16, 64 and 1024 with ackSlots 1, 2 and maxFrames."""
    L = load(path)
    m = 4
    for ab in (16, 64, 1024):
        stride = ab + 80
        rows, lens = slot_rows(ab, stride)
        dr = DevRows(L, rows, stride, lens)
        for s in (1, 2, m):
            T, W, c, WA, got = check_dd(L, dr.dev, stride, dr.lens, len(rows), m, s, ab)
            assert c == len(rows) and WA >= len(rows)
            # and with room for two thirds of the slots
            check_dd(L, dr.dev, stride, dr.lens, len(rows), m, s, ab, maxRecords=T, maxAcks=max(s, 2 * WA // 3))
        dr.free()


# 6 -------------------------------------------------------------------------
def recv(L, decs, encs, out, m, s, ab, maxRecords, maxAcks, dev, stride, count):
    res = (C.c_int * maxRecords)(*([-1] * maxRecords))
    nxt = (C.c_uint * maxRecords)(*([0xEEEE] * maxRecords))
    nrows, n = C.c_uint(12345), C.c_uint(12345)
    r = L.sgpu_frames_recv_duplex_dense(decs, len(decs) if decs else 0, encs, len(encs) if encs else 0, out, m, s, ab,
                                        maxRecords, maxAcks, dev, stride, count, res, nxt, C.byref(nrows), C.byref(n))
    return r, list(res), list(nxt), nrows.value, n.value


def encoder_stats(L, enc):
    v = (C.c_uint64 * 9)()
    assert L.sgpu_encoder_stats(enc, v, 9) == SUCCESS
    return list(v)


class Side:
    """Two sender/receiver pairs (flows 0 and 1) and a third decoder for the
    originals in the rows: the instances one recv call feeds."""

    def __init__(self, L, data):
        self.L = L
        self.pairs = [Pair(L, data), Pair(L, data)]
        for p in self.pairs:
            for i in range(len(data)):
                assert p.add(i) == (SUCCESS, i)
            for i in (0, 1, 3):
                assert p.recv(i) == SUCCESS
        self.extra = Pair(L, data)
        self.decs = (C.c_void_p * 1)(self.extra.dec)
        self.encs = (C.c_void_p * 2)(self.pairs[0].enc, self.pairs[1].enc)

    def state(self):
        return ([encoder_stats(self.L, p.enc) for p in self.pairs], DN.decoder_stats(self.L, self.extra.dec),
                [self.L.sgpu_decoder_has(self.extra.dec, i) for i in range(6)])

    def free(self):
        for p in self.pairs + [self.extra]:
            p.free()


def check_routing(path):
    """Twin sets of decoders and encoders: one fed by sgpu_frames_recv_duplex,
    the other by the new pair with the rescan loop, on the same rows."""
    L = load(path)
    DN.load(path)
    data = [payload(40 + i, 30 + i) for i in range(6)]
    one, two = Side(L, data), Side(L, data)
    r, _, msg = one.pairs[0].ack(32)
    assert r == SUCCESS and len(msg) <= 16
    stride, m, s, ab = 160, 3, 1, 16
    hand = [[ack_frame(0, msg), frame(ORIGINAL, 0, 4, data[4])],
            [],
            [frame(ORIGINAL, 0, 5, data[5]), ack_frame(1, msg), ack_frame(0, msg)],   # the second ack: no slot
            [ack_frame(2, msg)],                                                    # no encoder for flow 2
            [],
            [ack_frame(1, msg + bytes(20))],                                        # longer than ackBytes
            [frame(ORIGINAL, 0, 2, data[2]), 3, bytes([1, ORIGINAL])]]              # malformed behind a good frame
    built = [row_of(q, stride) for q in hand]
    count = len(hand)
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    _, words, _, o = A.scan(L, dr.dev, stride, dr.lens, count, m, s, ab)
    rA, resA, nxtA, accA = A.recv(L, one.decs, one.encs, o, dr.dev, stride, count)
    o.free()
    ns = [w & PACKED_COUNT_MASK for w in words]
    flatA = [resA[k * m + j] for k in range(count) for j in range(ns[k])]
    flatN = [nxtA[k * m + j] for k in range(count) for j in range(ns[k])]
    assert rA == INVALID and accA == 5
    s0 = stats(L)
    done, flatB, flatM, accB, rB, scanned = 0, [], [], 0, SUCCESS, 0
    while done < count:
        left = count - done
        mr, ma = min(m, left * m), min(s, left * s)   # the minimum: at least one row per scan
        got, ob = scan(L, dr.dev + done * stride, stride, dr.lens + 4 * done, left, m, s, ab, mr, ma)
        scanned += left
        r, res, nxt, c, n = recv(L, two.decs, two.encs, ob.out, m, s, ab, mr, ma, dr.dev + done * stride, stride, left)
        T, W, cc, WA = struct.unpack_from("<4I", got, 0)
        assert c == cc >= 1 and res[W:] == [NEED_MORE] * (mr - W)
        flatB += res[:W]
        flatM += nxt[:W]
        accB += n
        rB = rB if rB != SUCCESS else r
        done += c
        ob.free()
    assert stats(L)[STAT_DUPLEX_DENSE] - s0[STAT_DUPLEX_DENSE] == scanned > count
    assert (rB, flatB, flatM, accB) == (rA, flatA, flatN, accA)
    assert one.state() == two.state()
    assert L.sgpu_flush() == 0
    dr.free()
    one.free()
    two.free()


def check_loop(path):
    """One round of arq_cases.check_loop's shape through the new pair: 8 flows'
    k_frame rows, lost ones zeroed by their length, and behind them the
    decoders' ack rows of the round before, in one buffer of rows through
    sgpu_frames_scan_duplex_dense and sgpu_frames_recv_duplex_dense with the
    rescan loop; the originals reach the decoders and every encoder learns its
    flow's first lost packet; after the RTO the encoders' retransmission rows,
    several frames to a row, go through the same pair back into the decoders,
    and every original is there byte for byte."""
    L = load(path)
    flows, n, stride = 8, 12, 1232
    pairs = []
    for f in range(flows):
        data = [payload(7000 + 100 * f + i, A.variable_bytes(100 * f + i)) for i in range(n)]
        p = Pair(L, data)
        for i in range(n):
            assert p.add(i) == (SUCCESS, i)
        pairs.append(p)
    decs = (C.c_void_p * flows)(*[p.dec for p in pairs])
    encs = (C.c_void_p * flows)(*[p.enc for p in pairs])
    s, ab = 1, 48

    def through(dev, lens, count, m, room, aroom, allowed=(SUCCESS,)):
        done, acc, nexts = 0, 0, {}
        while done < count:
            left = count - done
            mr, ma = min(room, left * m), min(aroom, left * s)
            got, o = scan(L, dev + done * stride, stride, lens + 4 * done, left, m, s, ab, mr, ma)
            r, res, nxt, c, k = recv(L, decs, encs, o.out, m, s, ab, mr, ma, dev + done * stride, stride, left)
            assert r in allowed and c >= 1
            T, W, cc, WA = struct.unpack_from("<4I", got, 0)
            ro = records_offset(left)
            for i in range(W):
                h = PackedHead.from_buffer_copy(got, ro + i * REC)
                if h.Type == ACK:
                    nexts[h.Flow] = nxt[i]
            acc += k
            done += c
            o.free()
        return acc, nexts

    # forward: one original per row, all flows in one buffer, and room for the acks behind them
    buf = Rows(L, flows * n + flows, stride)
    lost = set()
    ch = A.Pcg(11, 5)
    for f, p in enumerate(pairs):
        q = C.c_uint(0)
        assert L.sgpu_encoder_deliver_range(p.enc, 0, n, f, buf.dst + f * n * stride, stride, buf.lens + 4 * f * n,
                                            None, C.byref(q)) == SUCCESS and q.value == n
        lost |= {f * n + i for i in range(1, n) if ch.next() % 100 < 30}
    assert L.sgpu_flush() == 0 and len(lost) >= flows
    for k in lost:   # the channel: a lost row's length word says so
        assert L.sgpu_h2d(buf.lens + 4 * k, bytes(4), 4) == 0
    acc, nexts = through(buf.dst, buf.lens, flows * n, 2, 40, 4)
    assert acc == flows * n - len(lost) and nexts == {}
    # back: one ack row per flow behind the data rows, and the whole buffer again (the data rows are duplicates
    # now, which the decoders say of each; the acks reach the encoders)
    fl = (C.c_uint * flows)(*range(flows))
    q = C.c_uint(0)
    back, blens = buf.dst + flows * n * stride, buf.lens + 4 * flows * n
    assert L.sgpu_decoders_ack_frames(decs, flows, fl, 48, back, stride, blens, None, C.byref(q)) == SUCCESS
    assert q.value == flows and L.sgpu_flush() == 0
    acc, nexts = through(back, blens, flows, 2, 3, 3)
    assert acc == flows
    for f in range(flows):
        firstLost = min(i for i in range(1, n + 1) if i == n or f * n + i in lost)
        assert nexts[f] == firstLost, "flow %d" % f
    time.sleep(A.RTO_SLEEP)
    # retransmissions: rows of several frames, through the new pair back into the decoders
    maxRows = n
    re = Rows(L, flows * maxRows, stride)
    sent = 0
    for f, p in enumerate(pairs):
        nums = (C.c_uint * n)()
        nr, nf = C.c_uint(0), C.c_uint(0)
        assert L.sgpu_encoder_retransmit_frames(p.enc, f, n, re.dst + f * maxRows * stride, stride, maxRows,
                                                re.lens + 4 * f * maxRows, nums, C.byref(nr), C.byref(nf)) == SUCCESS
        assert set(nums[:nf.value]) >= {i for i in range(n) if f * n + i in lost}
        sent += nf.value
    assert L.sgpu_flush() == 0 and sent >= len(lost)
    # (a retransmission of a packet that did arrive is a duplicate; room for 16 records makes the loop rescan)
    acc, nexts = through(re.dst, re.lens, flows * maxRows, 8, 16, 2, allowed=(SUCCESS, A.DUPLICATE))
    assert acc == sent and nexts == {}
    assert L.sgpu_flush() == 0
    # every original is there, byte for byte
    out = Rows(L, flows * n, stride)
    for f, p in enumerate(pairs):
        q = C.c_uint(0)
        res = (C.c_int * n)()
        assert L.sgpu_decoder_deliver_range(p.dec, 0, n, out.dst + f * n * stride, stride, out.lens + 4 * f * n, res,
                                            C.byref(q)) == SUCCESS
        assert q.value == n, "flow %d: %d of %d originals arrived" % (f, q.value, n)
    assert L.sgpu_flush() == 0
    got, lens = out.fetch()
    for f, p in enumerate(pairs):
        for i in range(n):
            k = f * n + i
            assert hashlib.sha256(got[k][:lens[k]]).digest() == hashlib.sha256(p.data[i]).digest(), (f, i)
    for r in (buf, re, out):
        r.free()
    for p in pairs:
        p.free()


# 7 -------------------------------------------------------------------------
def check_arguments(path, gpu):
    """Every refusal with nothing queued and the counters unchanged; count == 0;
    the counter and the timing entries of the one scan that was queued."""
    L = load(path)
    DN.load(path)
    stride, count, m, s, ab = 64, 4, 2, 1, 16
    built = [row_of([frame(ORIGINAL, 0, k, payload(700 + k, 10 + k)), 3, ack_frame(0, payload(5, 4))], stride)
             for k in range(count)]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    maxRecords, maxAcks = count * m, count * s
    o = Out(L, count, maxRecords, maxAcks, ab)
    p = Pair(L, [payload(1, 20)])
    decs, encs = (C.c_void_p * 1)(p.dec), (C.c_void_p * 1)(p.enc)
    assert L.sgpu_flush() == 0
    s0 = stats(L)
    B = L.sgpu_frames_duplex_dense_bytes
    assert B(3, 0, 3, 16) == 0 and B(3, 3 * 256 + 1, 3, 16) == 0 and B(3, 3, 0, 16) == 0
    assert B(3, 3, 3 * 256 + 1, 16) == 0 and B(0, 1, 1, 16) == 0
    assert B(3, 3, 3, 0) == 0 and B(3, 3, 3, 8) == 0 and B(3, 3, 3, 24) == 0 and B(3, 3, 3, 1040) == 0
    assert B(3, 6, 3, 16) == 48 + 6 * 32 + 16 + 3 * 16
    assert B(1 << 20, 1 << 27, 1 << 20, 1024) == 0, "an output of 4 GiB or more (the records alone)"
    assert B(1 << 20, 1 << 26, 1 << 20, 1024) == 32 + (8 << 20) + (2 << 30) + (4 << 20) + 16 + (1 << 30)
    assert L.sgpu_frames_duplex_dense_acks(3, 0) == 0 and L.sgpu_frames_duplex_dense_slots(3, 0) == 0
    assert L.sgpu_frames_duplex_dense_acks(3, 6) == 48 + 192 and L.sgpu_frames_duplex_dense_slots(3, 6) == 48 + 192 + 16
    assert L.sgpu_frames_duplex_dense_slots(4, 6) == 64 + 192 + 32

    # the 4 GiB edge of the output with maxRecords = maxAcks = count and ackBytes 16
    edge = (1 << 32) // 60 - 4
    while slots_offset(edge, edge) + 16 * edge < 1 << 32:
        edge += 1
    assert B(edge - 1, edge - 1, edge - 1, 16) == slots_offset(edge - 1, edge - 1) + 16 * (edge - 1) < 1 << 32
    assert B(edge, edge, edge, 16) == 0 and L.sgpu_frames_duplex_bytes(edge, 1, 1, 16) < 1 << 32

    def scan_args(**kw):
        a = dict(rows=dr.dev, stride=stride, lens=dr.lens, count=count, m=m, s=s, b=ab, r=maxRecords, a=maxAcks,
                 out=o.out)
        a.update(kw)
        return L.sgpu_frames_scan_duplex_dense(a["rows"], a["stride"], a["lens"], a["count"], a["m"], a["s"], a["b"],
                                               a["r"], a["a"], a["out"])

    shared = [
        ("null rows", dict(rows=None)),
        ("rows not 16-byte aligned", dict(rows=dr.dev + 8)),
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
    for what, kw in shared + [("null output", dict(out=None)), ("output not 16-byte aligned", dict(out=o.out + 8)),
                              ("lengths not 4-byte aligned", dict(lens=dr.lens + 2)),
                              ("a duplex output above 4 GiB", dict(count=1 << 19, m=256, s=1, r=256, a=1)),
                              # (52 bytes a row duplex, 60 dense -- word, start, record, astart, slot: at the first
                              # count whose dense output reaches 4 GiB the duplex output still fits)
                              ("an output of 4 GiB", dict(count=edge, m=1, s=1, r=edge, a=edge))]:
        assert scan_args(**kw) == -1, what
    assert L.sgpu_flush() == 0
    assert o.untouched()
    s1 = stats(L)
    watched = (0, 1, STAT_DUPLEX_DENSE, STAT_DENSE, STAT_DUPLEX, P.STAT_WALKS)
    assert [s1[i] for i in watched] == [s0[i] for i in watched]

    L.sgpu_timing(1, 1, None, None)
    t = scan_args()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_ACKWALK] > 0 and ms[TIMING_ROWSUM2] > 0 and ms[TIMING_COMPACT] > 0 and ms[TIMING_SLOTS] > 0
        assert ms[TIMING_WALK] == 0 and ms[TIMING_ROWSUM] == 0, "the walk counts under [12], the sum under [17]"
    got = o.fetch()
    raw = duplex_raw(L, dr.dev, stride, dr.lens, count, m, s, ab)
    want, T, W, c, WA = dense_from_duplex(raw, count, m, s, ab, maxRecords, maxAcks)
    assert got == want and (T, W, c, WA) == (8, 8, 4, 4)
    s2 = stats(L)
    assert s2[STAT_DUPLEX_DENSE] - s1[STAT_DUPLEX_DENSE] == count, "only the one valid scan was counted"
    assert s2[STAT_DENSE] == s1[STAT_DENSE] and s2[STAT_DUPLEX] - s1[STAT_DUPLEX] == count   # (duplex_raw's scan)
    # the other scans leave [39], [17] and [18] alone
    L.sgpu_timing(1, 1, None, None)
    duplex_raw(L, dr.dev, stride, dr.lens, count, m, s, ab)
    dn, od = DN.scan(L, dr.dev, stride, dr.lens, count, m, maxRecords)
    od.free()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    assert ms[TIMING_ROWSUM2] == 0 and ms[TIMING_SLOTS] == 0
    assert stats(L)[STAT_DUPLEX_DENSE] == s2[STAT_DUPLEX_DENSE]
    s2 = stats(L)

    def recv_args(**kw):
        a = dict(decs=decs, encs=encs, heads=o.out, rows=dr.dev, stride=stride, count=count, m=m, s=s, b=ab,
                 r=maxRecords, a=maxAcks, rowsOut=True)
        a.update(kw)
        n, nrows = C.c_uint(99), C.c_uint(99)
        res = (C.c_int * maxRecords)(*([-1] * maxRecords))
        r = L.sgpu_frames_recv_duplex_dense(a["decs"], 1, a["encs"], 1, a["heads"], a["m"], a["s"], a["b"], a["r"],
                                            a["a"], a["rows"], a["stride"], a["count"], res, None,
                                            C.byref(nrows) if a["rowsOut"] else None, C.byref(n))
        return r, n.value, nrows.value if a["rowsOut"] else 0, list(res)

    for what, kw in shared + [("null decoders", dict(decs=None)), ("null encoders", dict(encs=None)),
                              ("null output", dict(heads=None)), ("output not 4-byte aligned", dict(heads=o.out + 2)),
                              ("null rowsOut", dict(rowsOut=False))]:
        assert recv_args(**kw) == (INVALID, 0, 0, [-1] * maxRecords), what
    assert L.sgpu_frames_recv_duplex_dense(decs, 1, encs, 1, o.out, m, s, ab, maxRecords, maxAcks, dr.dev, stride,
                                           count, None, None, None, None) == INVALID
    for k in range(count):
        assert L.sgpu_decoder_has(p.dec, k) == NEED_MORE, "a refused call must not reach the decoder"
    assert p.enc_stats()[6] == 0, "a refused call must not reach the encoder"

    # count == 0: a ticket that is complete, nothing scanned, nothing written; nothing accepted
    before = C.string_at(o.base, o.bytes)
    for kw in (dict(count=0), dict(count=0, r=0, a=0), dict(count=0, rows=None, lens=None, out=None)):
        t0 = scan_args(**kw)
        assert t0 > t and L.sgpu_gather_wait(t0) == 0
    assert recv_args(count=0)[:3] == (SUCCESS, 0, 0)
    assert recv_args(count=0, heads=None, rows=None)[:3] == (SUCCESS, 0, 0)
    assert L.sgpu_flush() == 0
    s3 = stats(L)
    assert [s3[i] for i in watched] == [s2[i] for i in watched], "nothing was queued by any of them"
    assert C.string_at(o.base, o.bytes) == before

    # (the arguments were fine otherwise: the originals are accepted, the acks are no messages of a decoder)
    r, n, nrows, res = recv_args()
    assert nrows == count and res[0::2] == [SUCCESS] * count and n >= count
    assert L.sgpu_flush() == 0
    p.free()
    o.free()
    dr.free()


# 8 (the CPU double only) ----------------------------------------------------
def check_forged(path):
    """The output is caller data: sgpu_frames_recv_duplex_dense refuses what no
    scan could have written, routes nothing behind the first start of either
    table that fails and reads no slot outside the row's own
    (duplex_dense_forged_test.cpp runs the same forgeries under the sanitizers)."""
    L = load(path)
    stride, m, s, ab, count = 128, 2, 1, 16, 6
    data = [payload(800 + i, 12 + i) for i in range(2 * count)]
    snd = Pair(L, data)   # the encoder the acks go to; its decoder states the ack message
    for i in range(2 * count):
        assert snd.add(i) == (SUCCESS, i)
    assert snd.recv(0) == SUCCESS and snd.recv(2) == SUCCESS
    r, _, msg = snd.ack(16)
    assert r == SUCCESS and len(msg) <= ab
    rows, lens = [], []
    for k in range(count):
        row, end = row_of([frame(ORIGINAL, 0, 50 + k, payload(800 + k, 12 + k)), 1 + k, ack_frame(0, msg)], stride)
        rows.append(row)
        lens.append(end)
    dr = DevRows(L, rows, stride, lens)
    maxRecords, maxAcks = count * m, count * s
    good, o = scan(L, dr.dev, stride, dr.lens, count, m, s, ab, maxRecords, maxAcks)
    startAt, recAt = 16 + 4 * count, records_offset(count)
    ackAt = acks_offset(count, maxRecords)

    def word(at, v):
        return lambda b: b.__setitem__(slice(at, at + 4), struct.pack("<I", v))

    def record(i, **kw):
        def edit(b):
            h = PackedHead.from_buffer_copy(b, recAt + i * REC)
            for f, v in kw.items():
                setattr(h, f, v)
            b[recAt + i * REC:recAt + (i + 1) * REC] = bytes(h)
        return edit

    # (what is forged, rows routed before the refusal, frames accepted)
    cases = [
        ("nothing forged", lambda b: None, count, 2 * count),
        ("c > count", word(8, count + 1), 0, 0),
        ("W > maxRecords", word(4, maxRecords + 1), 0, 0),
        ("WA > maxAcks", word(12, maxAcks + 1), 0, 0),
        ("W != start[c]", word(4, maxRecords - 1), 5, 10),
        ("WA != astart[c]", word(12, maxAcks - 1), 5, 10),
        ("start[0] != 0", word(startAt, 1), 0, 0),
        ("astart[0] != 0", word(ackAt, 1), 0, 0),
        ("decreasing starts", word(startAt + 4 * 3, 3), 2, 4),
        ("decreasing astarts", word(ackAt + 4 * 3, 1), 2, 4),
        ("an astart step that disagrees with the row's ack records", word(ackAt + 4 * 2, 3), 1, 2),
        ("an astart step for a row whose ack record became an original", record(5, Type=ORIGINAL), 2, 4),
        ("a word count above maxFrames", word(16, m + 1), count, 2 * count - 2),
        ("an ack record with PacketNum 1", record(3, PacketNum=1), 1, 2),
        ("an ack record with Status 4", record(3, Status=4), count, 2 * count - 1),
        ("an ack record truncated without cause", record(3, Status=ROW_TRUNCATED), count, 2 * count - 1),
        ("an ack record whose DataBytes exceeds its slot", record(3, DataBytes=ab + 1), count, 2 * count - 1),
    ]
    for what, forge, rowsDone, accepted in cases:
        b = bytearray(good)
        forge(b)
        C.memmove(o.out, bytes(b), len(b))
        rcv, dec = Pair(L, data), L.sgpu_decoder_create()
        for i in range(2 * count):
            assert rcv.add(i) == (SUCCESS, i)
        r, res, nxt, nrows, n = recv(L, (C.c_void_p * 1)(dec), (C.c_void_p * 1)(rcv.enc), o.out, m, s, ab, maxRecords,
                                     maxAcks, dr.dev, stride, count)
        assert (r, nrows, n) == (SUCCESS if what == "nothing forged" else INVALID, rowsDone, accepted), \
            "%s: %r" % (what, (r, nrows, n))
        assert rcv.enc_stats()[6] <= accepted
        assert L.sgpu_flush() == 0
        L.sgpu_decoder_free(dec)
        rcv.free()
    assert L.sgpu_flush() == 0
    o.free()
    dr.free()
    snd.free()
