"""ARQ on the batch ABI: sgpu_decoder_ack / sgpu_encoder_acknowledge /
sgpu_encoder_retransmit, ack and retransmission rows (sgpu_decoders_ack_frames,
sgpu_encoder_retransmit_frames) and the duplex scan (sgpu_frames_scan_duplex,
sgpu_frames_recv_duplex): the cases shared by test_arq_cpu.py (the CPU test
double, tests/hostsim) and test_arq_gpu.py (k_ackwalk and k_frame on the
MI355X), driven through the C ABI with ctypes.

Expected acknowledgements, results and retransmissions come from the reference
library (oracle/_ref) through siamese_amd.binding, driven by the same call
sequence.  Expected duplex records come from model_row, a restatement of
frames.h ack_walk (which tests/ack_walk_test.cpp pins on its own), and for
rows without an ack from sgpu_frames_scan_packed over the same rows.  Every
scan writes between two guard records pre-filled with 0xA5.
"""
import ctypes as C
import hashlib
import time

import deliver_cases as D
import pack_cases as P
from deliver_cases import DISABLED, FILL, INVALID, NEED_MORE, SUCCESS, Orig, Rows, payload, read
from frame_cases import ORIGINAL, RECOVERY, header
from pack_cases import frame, prefix, row_of
from scan_cases import DevRows
from siamese_amd.binding import (PACKED_COUNT_MASK, PACKED_MALFORMED, PACKED_MORE, ROW_OK, PackedHead,
                                 bind_duplex_abi, SiameseLib, ROW_TRUNCATED, PACKED_ACKS_DROPPED, FRAME_ACK)

ACK = FRAME_ACK
REC = C.sizeof(PackedHead)
ZERO = P.ZERO
STAT_DUPLEX, STAT_ACKS, NSTATS = 27, 28, 29
TIMING_ACKWALK = 12
RTO_SLEEP = 0.65   # past the initial 500 ms RTO, as api_fuzz.run_arq sleeps


def load(path):
    L = P.load(path)
    if getattr(L, "_arq_cases", False):
        return L
    # (the symbols under test: an AttributeError here is the parent's answer)
    bind_duplex_abi(L)
    L._arq_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


# ---- the stream of the parity cases (harness/scenario.h's rule) --------------
class Pcg:
    """PCG-XSH-RR 64/32 as harness/scenario.h seeds it."""

    def __init__(self, y, x=0):
        self.state, self.inc = 0, ((y << 1) | 1) & (2 ** 64 - 1)
        self.next()
        self.state = (self.state + x) & (2 ** 64 - 1)
        self.next()

    def next(self):
        s = self.state
        self.state = (s * 6364136223846793005 + self.inc) & (2 ** 64 - 1)
        xs = (((s >> 18) ^ s) >> 27) & 0xffffffff
        r = s >> 59
        return ((xs >> r) | (xs << ((32 - r) & 31))) & 0xffffffff


def variable_bytes(i):
    """2..1199 bytes (scenario.h variable_bytes)."""
    return 2 + Pcg(i, 24124).next() % (1200 - 2)


STREAM = 40
LOSS_PCT = 25


def stream(seed):
    """(payloads, lost flags) of one case: 40 variable-size originals."""
    data = [payload(seed * 100 + i, variable_bytes(seed * STREAM + i)) for i in range(STREAM)]
    ch = Pcg(seed, 77)
    lost = [ch.next() % 100 < LOSS_PCT for _ in range(STREAM)]
    lost[0] = False
    assert any(lost) and all(2 <= len(d) <= 1199 for d in data)
    return data, lost


class Pair:
    """A batch encoder and decoder fed from device memory."""

    def __init__(self, L, data):
        self.L, self.data = L, data
        self.pitch = 1216
        blob = bytearray(self.pitch * len(data))
        for i, d in enumerate(data):
            blob[i * self.pitch:i * self.pitch + len(d)] = d
        self.src = L.sgpu_device_alloc(len(blob))
        assert self.src and L.sgpu_h2d(self.src, bytes(blob), len(blob)) == 0
        self.enc, self.dec = L.sgpu_encoder_create(), L.sgpu_decoder_create()
        assert self.enc and self.dec

    def add(self, i):
        num = C.c_uint(0)
        r = self.L.sgpu_encoder_add(self.enc, self.src + i * self.pitch, len(self.data[i]), C.byref(num))
        return r, num.value

    def recv(self, i):
        return self.L.sgpu_decoder_add_original(self.dec, i, self.src + i * self.pitch, len(self.data[i]))

    def ack(self, limit):
        buf = C.create_string_buffer(limit)
        used = C.c_uint(0)
        r = self.L.sgpu_decoder_ack(self.dec, buf, limit, C.byref(used))
        return r, used.value, buf.raw[:used.value]

    def acknowledge(self, msg, n=None):
        nxt = C.c_uint(0)
        r = self.L.sgpu_encoder_acknowledge(self.enc, msg, len(msg) if n is None else n, C.byref(nxt))
        return r, nxt.value

    def retransmit(self):
        p = Orig()
        r = self.L.sgpu_encoder_retransmit(self.enc, C.byref(p))
        return r, p

    def enc_stats(self):
        v = (C.c_uint64 * 9)()
        assert self.L.sgpu_encoder_stats(self.enc, v, 9) == SUCCESS
        return list(v)

    def dec_stats(self):
        v = (C.c_uint64 * 11)()
        assert self.L.sgpu_decoder_stats(self.dec, v, 11) == SUCCESS
        return list(v)

    def free(self):
        self.L.sgpu_encoder_free(self.enc)
        self.L.sgpu_decoder_free(self.dec)
        assert self.L.sgpu_flush() == 0
        self.L.sgpu_device_free(self.src)


def bad_acks(msg):
    """Stale, duplicate and malformed variants of an acknowledgement."""
    out = [("duplicate", msg), ("empty ranges", msg[:1])]
    if len(msg) > 2:
        out.append(("range cut", msg[:len(msg) - 1]))
        out.append(("range past the buffer", msg[:2] + b"\xff"))
    out.append(("cut head", b"\xc0"))
    out.append(("cut head 2", b"\x80"))
    return out


# 1 -------------------------------------------------------------------------
def check_parity(path, ref_path, limit, seed=3):
    """One call sequence through the batch ABI and the reference: every ack
    message, every result, nextExpected, the Ack statistics and, past the RTO,
    the retransmitted packet numbers in order, with the device bytes."""
    L = load(path)
    ref = SiameseLib(ref_path)
    data, lost = stream(seed)
    p = Pair(L, data)
    renc, rdec = ref.Encoder(), ref.Decoder()
    first = None
    for i in range(STREAM):
        r, num = p.add(i)
        assert (r, num) == renc.add_raw(data[i]) == (SUCCESS, i)
        if not lost[i]:
            assert p.recv(i) == rdec.add_original(i, data[i]) == SUCCESS
        if i % 4 == 3:
            r, used, msg = p.ack(limit)
            wr, wmsg = rdec.ack(limit)
            assert r == wr == SUCCESS and msg == wmsg and used == len(wmsg), \
                "ack after %d adds: %r (%d), reference %r" % (i + 1, msg.hex(), r, wmsg.hex())
            assert p.acknowledge(msg) == renc.ack(wmsg)
            first = first or msg
    assert L.sgpu_flush() == 0
    # stale (the first message again), duplicate and malformed ones
    for what, m in [("stale", first)] + bad_acks(msg):
        got, want = p.acknowledge(m), renc.ack(m)
        assert got[0] == want[0] and (got[0] != SUCCESS or got == want), "%s ack: %r, reference %r" % (what, got, want)
    # (the malformed ones may have changed the loss list: the last good one again)
    assert p.acknowledge(msg) == renc.ack(wmsg)
    assert p.enc_stats()[6:8] == renc.stats()[6:8], "encoder Ack statistics"
    assert p.dec_stats()[4:6] == rdec.stats()[4:6], "decoder Ack statistics"
    time.sleep(RTO_SLEEP)
    # (both loops at once and nothing slow in between: a packet sent again is due again an RTO later)
    got, want = [], []
    for _ in range(STREAM + 1):
        r, q = p.retransmit()
        wr, w = renc.retransmit()
        assert r == wr
        if r != SUCCESS:
            assert r == NEED_MORE
            break
        got.append((q.PacketNum, q.Data, q.DataBytes))
        want.append(w)
    assert [g[0] for g in got] == [w[0] for w in want] and got, "retransmitted %r, reference %r" % (got, want)
    assert {g[0] for g in got} >= {i for i in range(STREAM) if lost[i]}
    for (num, dev, n), w in zip(got, want):
        assert n == len(w[1]) and read(L, dev, n) == data[num] == w[1], "the device bytes of packet %d" % num
    assert p.enc_stats()[4:6] == renc.stats()[4:6], "Retransmit statistics"
    p.free()


def check_arq_arguments(path):
    L = load(path)
    data = [payload(1, 50)]
    p = Pair(L, data)
    buf = C.create_string_buffer(64)
    used = C.c_uint(9)
    assert L.sgpu_decoder_ack(None, buf, 64, C.byref(used)) == INVALID
    assert L.sgpu_decoder_ack(p.dec, None, 64, C.byref(used)) == INVALID
    assert L.sgpu_decoder_ack(p.dec, buf, 64, None) == INVALID
    assert L.sgpu_decoder_ack(p.dec, buf, 15, C.byref(used)) == INVALID
    assert L.sgpu_decoder_ack(p.dec, buf, 16, C.byref(used)) == NEED_MORE and used.value == 0
    nxt = C.c_uint(0)
    assert L.sgpu_encoder_acknowledge(None, b"\0", 1, C.byref(nxt)) == INVALID
    assert L.sgpu_encoder_acknowledge(p.enc, None, 1, C.byref(nxt)) == INVALID
    assert L.sgpu_encoder_acknowledge(p.enc, b"\0", 0, C.byref(nxt)) == INVALID
    assert L.sgpu_encoder_acknowledge(p.enc, b"\0", 1, None) == INVALID
    o = Orig()
    assert L.sgpu_encoder_retransmit(None, C.byref(o)) == INVALID
    assert L.sgpu_encoder_retransmit(p.enc, None) == INVALID
    assert L.sgpu_encoder_retransmit(p.enc, C.byref(o)) == NEED_MORE
    v = (C.c_uint64 * 9)()
    assert L.sgpu_encoder_stats(None, v, 9) == INVALID and L.sgpu_encoder_stats(p.enc, None, 9) == INVALID
    assert L.sgpu_encoder_stats(p.enc, v, 0) == INVALID
    assert L.sgpu_decoder_stats(None, v, 9) == INVALID and L.sgpu_decoder_stats(p.dec, None, 9) == INVALID
    out = (C.c_ubyte * 64)()
    assert L.sgpu_frame_write_ack(1, b"ab", 2, out, 64) == 7 and bytes(out[:7]) == b"\x06\x02\x01\x00\x00ab"
    assert L.sgpu_frame_write_ack(1, b"ab", 2, out, 6) == 0
    assert L.sgpu_frame_write_ack(1, b"ab", 0, out, 64) == 0
    assert L.sgpu_frame_write_ack(1 << 24, b"ab", 2, out, 64) == 0
    assert L.sgpu_frame_write_ack(1, None, 2, out, 64) == 0 and L.sgpu_frame_write_ack(1, b"ab", 2, None, 64) == 0
    big = bytes(200)
    assert L.sgpu_frame_write_ack(5, big, 200, (C.c_ubyte * 256)(), 256) == 206   # a 2-byte prefix
    # the two-type calls keep refusing type 2
    assert L.sgpu_frame_header_bytes(ACK, 5) == 0 and L.sgpu_frame_write_header(ACK, 1, 0, 5, out) == 0
    r, fr = P.parse(L, ack_frame(1, b"abc") + bytes(8))
    assert r == INVALID and fr == []
    p.free()


def ack_frame(flow, msg, width=1):
    return prefix(4 + len(msg), width) + bytes([ACK]) + flow.to_bytes(3, "little") + msg


def write_ack(L, flow, msg):
    out = (C.c_ubyte * (len(msg) + 8))()
    n = L.sgpu_frame_write_ack(flow, msg, len(msg), out, len(msg) + 8)
    assert n
    return bytes(out[:n])


# 2 -------------------------------------------------------------------------
def check_ack_rows(path):
    """sgpu_decoders_ack_frames: rows = sgpu_frame_write_ack(flow, message) plus
    a zero tail; a decoder without packets gets a zero length and an untouched
    row; arguments."""
    L = load(path)
    data, lost = stream(5)
    pairs = [Pair(L, data) for _ in range(3)]
    for k, p in enumerate(pairs[:2]):
        for i in range(8 + 20 * k):
            if not lost[i]:
                assert p.recv(i) == SUCCESS
    stride, limit = 80, 64
    rows = Rows(L, 3, stride)
    decs = (C.c_void_p * 3)(pairs[0].dec, pairs[2].dec, pairs[1].dec)
    flows = (C.c_uint * 3)(0xABCDEF, 7, 0)
    res = (C.c_int * 3)(-1, -1, -1)
    q = C.c_uint(99)
    before = stats(L)
    args = lambda **kw: [kw.get("decs", decs), kw.get("count", 3), kw.get("flows", flows), kw.get("limit", limit),
                         kw.get("dst", rows.dst), kw.get("stride", stride), kw.get("lens", rows.lens), res,
                         C.byref(q)]
    for bad in (dict(decs=None), dict(flows=None), dict(limit=15), dict(dst=None), dict(dst=rows.dst + 8),
                dict(stride=72), dict(stride=0), dict(lens=None), dict(lens=rows.lens + 2),
                dict(flows=(C.c_uint * 3)(1, 1 << 24, 2)), dict(decs=(C.c_void_p * 3)(pairs[0].dec, None, None)),
                dict(limit=76)):   # 1 + 4 + 76 > 80
        assert L.sgpu_decoders_ack_frames(*args(**bad)) == INVALID and q.value == 0, bad
    assert L.sgpu_decoders_ack_frames(*args(limit=75)) == SUCCESS   # exactly fits
    assert L.sgpu_flush() == 0
    rows.refill()
    assert stats(L)[STAT_ACKS] - before[STAT_ACKS] == 2
    want = [pairs[0].ack(limit), None, pairs[1].ack(limit)]
    assert L.sgpu_decoders_ack_frames(*args()) == SUCCESS and q.value == 2
    assert list(res) == [SUCCESS, NEED_MORE, SUCCESS]
    assert rows.untouched(), "the call waited"
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    for k in (0, 2):
        fr = write_ack(L, flows[k], want[k][2])
        assert want[k][0] == SUCCESS and fr == ack_frame(flows[k], want[k][2])
        assert lens[k] == len(fr) and got[k] == fr + bytes(stride - len(fr)), "ack row %d" % k
    assert lens[1] == 0 and got[1] == bytes([FILL]) * stride
    assert L.sgpu_decoders_ack_frames(decs, 0, flows, limit, None, stride, None, res, C.byref(q)) == SUCCESS
    rows.free()
    for p in pairs:
        p.free()


def model_layout(frames, stride):
    """sgpu_encoder_pack_frames' cursor rule: [(row, off)], rows used."""
    out, row, off = [], 0, 0
    for f in frames:
        if off + len(f) > stride:
            row, off = row + 1, 0
        out.append((row, off))
        off = (off + len(f) + 15) & ~15
    return out, (row + 1 if frames else 0)


def rows_of(frames, stride, maxRows):
    lay, used = model_layout(frames, stride)
    rows = [bytearray(stride) for _ in range(used)]
    lens = [0] * maxRows
    for f, (r, o) in zip(frames, lay):
        rows[r][o:o + len(f)] = f
        lens[r] = o + len(f)
    return [bytes(r) for r in rows], lens


def retransmit_frames(L, enc, flow, maxPackets, rows, maxRows, stride=None):
    nums = (C.c_uint * max(1, maxPackets))()
    nrows, nframes = C.c_uint(77), C.c_uint(77)
    r = L.sgpu_encoder_retransmit_frames(enc, flow, maxPackets, rows.dst, stride or rows.stride, maxRows, rows.lens,
                                         nums, C.byref(nrows), C.byref(nframes))
    return r, list(nums)[:nframes.value], nrows.value


def check_retransmit_rows(path):
    """sgpu_encoder_retransmit_frames: the rows of the host-built layout of the
    same packet list, valid for sgpu_frames_parse and sgpu_frames_scan_packed;
    a maxRows that holds a part; a stride too small for the longest original."""
    L = load(path)
    lengths = [1199, 40, 700, 2, 1199, 333, 90, 121, 640, 17]
    data = [payload(900 + i, n) for i, n in enumerate(lengths)]
    p = Pair(L, data)
    for i in range(len(data)):
        assert p.add(i) == (SUCCESS, i)
    assert p.recv(0) == SUCCESS and p.recv(3) == SUCCESS
    assert L.sgpu_flush() == 0
    # (a measured round trip of 0.3 s makes the RTO 0.45 s: what this case sends again is not due
    # again before the case ends)
    time.sleep(0.3)
    r, used, msg = p.ack(64)
    assert r == SUCCESS and p.acknowledge(msg) == (SUCCESS, 1)
    time.sleep(RTO_SLEEP)
    flow, stride, maxRows = 0x010203, 1424, 8
    rows = Rows(L, maxRows, stride)
    # a stride below the longest original's frame: refused, nothing consumed
    small = Rows(L, 2, 1200)
    assert retransmit_frames(L, p.enc, flow, 99, small, 2) == (INVALID, [], 0)
    assert L.sgpu_flush() == 0 and small.untouched()
    small.free()
    for bad in (dict(flow=1 << 24), dict(stride=1432), dict(enc=None)):
        n1, n2 = C.c_uint(0), C.c_uint(0)
        assert L.sgpu_encoder_retransmit_frames(bad.get("enc", p.enc), bad.get("flow", flow), 9, rows.dst,
                                                bad.get("stride", stride), maxRows, rows.lens, None, C.byref(n1),
                                                C.byref(n2)) == INVALID
    assert L.sgpu_encoder_retransmit_frames(p.enc, flow, 9, rows.dst, stride, maxRows, rows.lens, None, None,
                                            C.byref(n2)) == INVALID
    r, q = p.retransmit()
    assert r == SUCCESS and q.PacketNum == 1, "the refused calls consumed a retransmission"
    # 2 rows hold a part: the call stops without consuming the rest
    r, nums1, used1 = retransmit_frames(L, p.enc, flow, 99, rows, 2)
    assert r == SUCCESS and 1 <= len(nums1) < 8 and used1 <= 2
    assert rows.untouched(), "the call waited"
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    fr = [header(L, ORIGINAL, flow, n, len(data[n])) + data[n] for n in nums1]
    wantRows, wantLens = rows_of(fr, stride, maxRows)
    assert len(wantRows) == used1 and lens[:2] == wantLens[:2] and got[:used1] == wantRows
    assert all(g == bytes([FILL]) * stride for g in got[used1:]) and lens[2:] == [0xA5A5A5A5] * 6
    rows.refill()
    r, nums2, used2 = retransmit_frames(L, p.enc, flow, 99, rows, maxRows)
    assert r == SUCCESS and sorted([1] + nums1 + nums2) == [1, 2, 4, 5, 6, 7, 8, 9], (nums1, nums2)
    assert L.sgpu_flush() == 0
    got, lens = rows.fetch()
    fr = [header(L, ORIGINAL, flow, n, len(data[n])) + data[n] for n in nums2]
    wantRows, wantLens = rows_of(fr, stride, maxRows)
    assert used2 == len(wantRows) and lens == wantLens and got[:used2] == wantRows
    assert all(g == bytes([FILL]) * stride for g in got[used2:])
    # valid input for the parser and the packed scan
    r, parsed = P.parse(L, b"".join(got[:used2]))
    assert r == SUCCESS and [f.PacketNum for f in parsed] == nums2
    recs, words, o = P.scan(L, rows.dst, stride, rows.lens, maxRows, 8)
    assert [x[6] for k in range(maxRows) for x in recs[k] if x[1] == ROW_OK] == nums2
    assert all(w & (PACKED_MALFORMED | PACKED_MORE) == 0 for w in words)
    o.free()
    # maxPackets bounds the call; nothing is due any more
    assert retransmit_frames(L, p.enc, flow, 0, rows, maxRows)[0:2] == (SUCCESS, [])
    r, nums3, used3 = retransmit_frames(L, p.enc, flow, 99, rows, maxRows)
    assert (r, nums3, used3) == (SUCCESS, [], 0)
    assert L.sgpu_flush() == 0
    assert rows.fetch()[1] == [0] * maxRows
    rows.free()
    p.free()


# 3 -------------------------------------------------------------------------
def read_prefix(b):
    """(prefix bytes, L) as read_length_prefix judges b, None when b is too short."""
    if not b:
        return None
    top = b[0] >> 6
    w = 1 if top <= 1 else 2 if top == 2 else 3 if b[0] & 0xE0 == 0xC0 else 4
    if len(b) < w:
        return None
    mask = [0xff, 0x3fff, 0x1fffff, 0x1fffffff][w - 1]
    return w, int.from_bytes(b[:w], "big") & mask


def model_row(row, stride, length, maxFrames, ackSlots, ackBytes):
    """frames.h ack_walk: (records, row word, slots) of one row."""
    slots = [bytes(ackBytes)] * ackSlots
    end = stride if length is None else length
    if end > stride:
        return [ZERO] * maxFrames, PACKED_MALFORMED, slots
    recs, flags, acks, at = [], 0, 0, 0
    while at < end:
        if row[at] == 0:
            at += 1
            continue
        if len(recs) == maxFrames:
            flags |= PACKED_MORE
            break
        pre = read_prefix(row[at:min(end, at + 4)])
        if pre is None or pre[1] < 1 or pre[0] + pre[1] > end - at:
            flags |= PACKED_MALFORMED
            break
        h, ln = pre
        kind = row[at + h]
        inner = 7 if kind == ORIGINAL else 4
        if kind > ACK or ln <= inner:
            flags |= PACKED_MALFORMED
            break
        flow = int.from_bytes(row[at + h + 1:at + h + 4], "little")
        d = ln - inner
        body = row[at + h + inner:at + h + ln]
        if kind == ACK:
            status = ROW_OK
            if acks < ackSlots:
                slots[acks] = body[:ackBytes] + bytes(ackBytes - len(body[:ackBytes]))
            if acks >= ackSlots or d > ackBytes:
                status = ROW_TRUNCATED
                flags |= PACKED_ACKS_DROPPED
            recs.append((at, status, ACK, h + 4, 0, flow, acks, d, bytes(4), bytes(8)))
            acks += 1
        elif kind == ORIGINAL:
            num = int.from_bytes(row[at + h + 4:at + h + 7], "little")
            if num > D.PACKET_NUM_MAX:
                flags |= PACKED_MALFORMED
                break
            recs.append((at, ROW_OK, ORIGINAL, h + 7, 0, flow, num, d, bytes(4), bytes(8)))
        else:
            t = min(8, d)
            recs.append((at, ROW_OK, RECOVERY, h + 4, t, flow, 0, d, body[:4] + bytes(4 - len(body[:4])),
                         bytes(8 - t) + body[len(body) - t:]))
        at += h + ln
    return recs + [ZERO] * (maxFrames - len(recs)), len(recs) | flags, slots


class Out:
    """A duplex scan's output in pinned memory between two guard records."""

    def __init__(self, L, count, maxFrames, ackSlots, ackBytes):
        self.L, self.count, self.m, self.slots, self.ab = L, count, maxFrames, ackSlots, ackBytes
        self.total = L.sgpu_frames_duplex_bytes(count, maxFrames, ackSlots, ackBytes)
        self.soff = L.sgpu_frames_duplex_slots(count, maxFrames)
        assert self.soff == (count * maxFrames * REC + 4 * count + 15) & ~15
        assert self.total == self.soff + count * ackSlots * ackBytes
        self.bytes = self.total + 2 * REC
        self.base = L.sgpu_host_alloc(self.bytes)
        assert self.base and self.base % 16 == 0
        self.out = self.base + REC
        C.memset(self.base, FILL, self.bytes)

    def fetch(self):
        """(records per row, row words, slots per row), guards checked."""
        raw = C.string_at(self.base, self.bytes)
        guard = bytes([FILL]) * REC
        assert raw[:REC] == guard, "guard record before the records was written"
        assert raw[-REC:] == guard, "guard record after the slots was written"
        self.raw = raw[REC:-REC]
        m = self.m
        recs = [[P.fields(PackedHead.from_buffer_copy(self.raw, REC * (k * m + j))) for j in range(m)]
                for k in range(self.count)]
        w0 = REC * self.count * m
        words = [int.from_bytes(self.raw[w0 + 4 * k:w0 + 4 * k + 4], "little") for k in range(self.count)]
        s0, ab = self.soff, self.ab
        slots = [[self.raw[s0 + (k * self.slots + a) * ab:s0 + (k * self.slots + a + 1) * ab]
                  for a in range(self.slots)] for k in range(self.count)]
        return recs, words, slots

    def free(self):
        self.L.sgpu_host_free(self.base)


def scan(L, dev, stride, lens, count, maxFrames, ackSlots, ackBytes):
    o = Out(L, count, maxFrames, ackSlots, ackBytes)
    t = L.sgpu_frames_scan_duplex(dev, stride, lens, count, maxFrames, ackSlots, ackBytes, o.out)
    assert t > 0, "sgpu_frames_scan_duplex returned %d" % t
    assert L.sgpu_gather_wait(t) == 0
    return o.fetch() + (o,)


def check_duplex(L, rows, stride, lens, maxFrames, ackSlots, ackBytes):
    """Scan host-built rows with and without their lengths against model_row;
    returns the expectation with lengths."""
    dr = DevRows(L, rows, stride, lens)
    first = None
    for lp in (dr.lens, None):
        want = [model_row(rows[k], stride, lens[k] if lp else None, maxFrames, ackSlots, ackBytes)
                for k in range(len(rows))]
        recs, words, slots, o = scan(L, dr.dev, stride, lp, len(rows), maxFrames, ackSlots, ackBytes)
        for k in range(len(rows)):
            how = "row %d (%s lengths)" % (k, "with" if lp else "without")
            assert words[k] == want[k][1], "%s: word %#x, expected %#x" % (how, words[k], want[k][1])
            assert recs[k] == want[k][0], "%s: %r, expected %r" % (how, recs[k], want[k][0])
            assert slots[k] == want[k][2], "%s: slots differ" % how
        o.free()
        first = first or want
    dr.free()
    return first


def check_walk_small(path):
    """stride 16: a 6-byte ack (a 1-byte message), an ack that ends on the
    row's last byte, L = 4 and L = 5, type 3, lengths 0, stride and stride + 16,
    maxFrames 1 with bytes left."""
    L = load(path)
    stride = 16
    one = ack_frame(0x0000AB, b"\x05")
    assert len(one) == 6
    full = ack_frame(9, payload(1, 11))            # 16 bytes: ends on the row's last byte
    l4 = bytes([4, ACK, 1, 0, 0])                  # L = 4: no message
    l5 = bytes([5, ACK, 1, 0, 0, 0x33])            # L = 5
    t3 = bytes([6, 3, 1, 0, 0, 1, 2])              # type 3
    two = one + ack_frame(2, b"\x01\x02")
    parts = [(one, 6), (full, 16), (l4, 5), (l5, 6), (t3, 7), (two, len(two)), (one, 0), (one, stride + 16),
             (bytes(3) + one, 9), (one + bytes(2) + l5, 14)]
    rows = [p + bytes(stride - len(p)) for p, _ in parts]
    lens = [n for _, n in parts]
    want = check_duplex(L, rows, stride, lens, 1, 1, 16)
    assert want[0][1] == 1 and want[0][0][0] == (0, ROW_OK, ACK, 5, 0, 0xAB, 0, 1, bytes(4), bytes(8))
    assert want[0][2] == [b"\x05" + bytes(15)]
    assert want[1][1] == 1 and want[1][2] == [payload(1, 11) + bytes(5)]
    assert want[2][1] == PACKED_MALFORMED and want[4][1] == PACKED_MALFORMED
    assert want[3][1] == 1 and want[3][0][0][7] == 1
    assert want[5][1] == 1 | PACKED_MORE
    assert want[6][1] == 0 and want[7][1] == PACKED_MALFORMED
    want = check_duplex(L, rows, stride, lens, 2, 2, 16)
    assert want[5][1] == 2 and want[5][2][1] == b"\x01\x02" + bytes(14)
    assert want[9][1] == 2
    check_duplex(L, rows, stride, lens, 2, 1, 16)


def check_walk_slots(path):
    """A message of exactly ackBytes and one of ackBytes + 1 (truncated, the
    data frame behind it still reported); ackSlots 1 with two acks; acks at odd
    offsets behind an original, at every byte of a word; ackBytes 16 and 1024."""
    L = load(path)
    for ackBytes, stride in ((16, 128), (1024, 2304)):
        orig = frame(ORIGINAL, 3, 77, payload(2, 20))
        rec = frame(RECOVERY, 3, 0, payload(3, 30))
        exact = ack_frame(5, payload(4, ackBytes), 2)
        over = ack_frame(6, payload(5, ackBytes + 1), 2)
        rows, lens = [], []
        for parts in ([exact, orig], [over, orig], [orig, exact, rec], [orig, 1, over, 3, rec],
                      [ack_frame(1, b"a"), ack_frame(2, b"bc"), orig], [rec, over, exact][:2 if ackBytes > 16 else 3]):
            r, n = row_of(parts, stride)
            rows.append(r)
            lens.append(n)
        for off in range(16):   # the message starts at every byte of a 16-byte word
            r, n = row_of([orig, off, ack_frame(off, payload(60 + off, min(ackBytes, 37 + off))), 2, rec], stride)
            rows.append(r)
            lens.append(n)
        want = check_duplex(L, rows, stride, lens, 4, 2, ackBytes)
        assert want[0][1] == 2 and want[0][2][0] == payload(4, ackBytes)
        assert want[1][1] == 2 | PACKED_ACKS_DROPPED and want[1][0][0][1] == ROW_TRUNCATED
        assert want[1][0][1][2] == ORIGINAL and want[1][2][0] == payload(5, ackBytes + 1)[:ackBytes]
        assert want[3][1] == 3 | PACKED_ACKS_DROPPED and want[3][0][2][2] == RECOVERY
        want = check_duplex(L, rows, stride, lens, 4, 1, ackBytes)
        assert want[4][1] == 3 | PACKED_ACKS_DROPPED
        assert [x[1] for x in want[4][0][:3]] == [ROW_OK, ROW_TRUNCATED, ROW_OK] and want[4][0][1][6] == 1
        assert want[4][2] == [b"a" + bytes(ackBytes - 1)]


def check_walk_counts(path):
    """count 1, 256 and 257 (the workgroup edge); rows without an ack give
    records and row words byte for byte sgpu_frames_scan_packed's."""
    L = load(path)
    stride, m = 96, 3
    for count in (1, 256, 257):
        rows, lens = [], []
        for k in range(count):
            parts = [frame(ORIGINAL, k, k, payload(k, 5 + k % 20))]
            if k % 3 != 1:
                parts += [k % 5, ack_frame(k, payload(7 * k, 1 + k % 16))]
            if k % 4 == 0:
                parts += [frame(RECOVERY, k, 0, payload(9 * k, 9))]
            r, n = row_of(parts, stride)
            rows.append(r)
            lens.append(n if k % 7 else 0)
        check_duplex(L, rows, stride, lens, m, 1, 16)
    # no acks at all: the packed scan's bytes
    plain = []
    lens = []
    for k in range(40):
        r, n = row_of([frame(ORIGINAL, k, k, payload(k, 3 + k)), k % 9, frame(RECOVERY, k, 0, payload(k + 1, 1 + k % 12)),
                       frame(ORIGINAL, 1, 2, b"xy")][:1 + k % 3 + 1], stride)
        plain.append(r)
        lens.append([n, 0, stride + 16, n - 1][k % 4] if k % 5 == 0 else n)
    dr = DevRows(L, plain, stride, lens)
    for lp in (dr.lens, None):
        for mf in (1, 2, 4):
            _, _, _, o = scan(L, dr.dev, stride, lp, 40, mf, 1, 16)
            _, _, po = P.scan(L, dr.dev, stride, lp, 40, mf)
            n = L.sgpu_frames_packed_bytes(40, mf)
            assert o.raw[:n] == C.string_at(po.out, n), "records or row words differ from the packed scan's"
            assert o.raw[o.soff:] == bytes(40 * 16)
            o.free()
            po.free()
    dr.free()


def check_duplex_arguments(path, gpu):
    L = load(path)
    stride = 64
    rows = [row_of([ack_frame(0, b"m")], stride)[0]] * 2
    dr = DevRows(L, rows, stride, [6, 6])
    o = Out(L, 2, 2, 1, 16)
    ok = dict(rows=dr.dev, stride=stride, lens=dr.lens, count=2, m=2, s=1, b=16, out=o.out)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sgpu_frames_scan_duplex(a["rows"], a["stride"], a["lens"], a["count"], a["m"], a["s"], a["b"],
                                         a["out"])
    for bad in (dict(rows=None), dict(rows=dr.dev + 8), dict(stride=0), dict(stride=72), dict(lens=dr.lens + 2),
                dict(out=None), dict(out=o.out + 8), dict(m=0), dict(m=257), dict(s=0), dict(s=3), dict(b=0),
                dict(b=8), dict(b=24), dict(b=1040)):
        assert call(**bad) == -1, bad
        if {"m", "s", "b"} & set(bad):
            assert L.sgpu_frames_duplex_bytes(2, bad.get("m", 2), bad.get("s", 1), bad.get("b", 16)) == 0
    assert C.string_at(o.base, o.bytes) == bytes([FILL]) * o.bytes
    t = call(count=0, rows=None, out=None)
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    before = stats(L)
    ms = (C.c_double * 13)()
    L.sgpu_timing(1, 1, None, None)
    t = call()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    L.sgpu_timing_kernels(ms, 13)
    L.sgpu_timing(0, 1, None, None)
    if gpu:
        assert ms[TIMING_ACKWALK] > 0 and ms[8] == 0, "k_ackwalk's device time is timing index 12"
    after = stats(L)
    assert after[STAT_DUPLEX] - before[STAT_DUPLEX] == 2 and after[P.STAT_WALKS] == before[P.STAT_WALKS]
    o.free()
    dr.free()


# recv_duplex ------------------------------------------------------------------
def recv(L, decs, encs, o, dev, stride, count, want=None):
    res = (C.c_int * (count * o.m))(*([-1] * (count * o.m)))
    nxt = (C.c_uint * (count * o.m))(*([0xEEEE] * (count * o.m)))
    acc = C.c_uint(99)
    r = L.sgpu_frames_recv_duplex(decs, len(decs) if decs else 0, encs, len(encs) if encs else 0, o.out, o.m, o.slots,
                                  o.ab, dev, stride, count, res, nxt, C.byref(acc))
    if want is not None:
        assert r == want, "sgpu_frames_recv_duplex returned %d, expected %d" % (r, want)
    return r, list(res), list(nxt), acc.value


def check_recv_duplex(path):
    """Routing: originals to decoders[Flow], acks to encoders[Flow]; a truncated
    ack, a flow without an encoder and forged records are InvalidInput and
    reach no encoder."""
    L = load(path)
    data = [payload(40 + i, 30 + i) for i in range(6)]
    a, b = Pair(L, data), Pair(L, data)   # flow 0 and flow 1
    for p in (a, b):
        for i in range(6):
            assert p.add(i) == (SUCCESS, i)
        for i in (0, 1, 3):
            assert p.recv(i) == SUCCESS
    r, _, msg = a.ack(32)
    assert r == SUCCESS
    stride, m = 160, 3
    extra = Pair(L, data)   # the receiver of the originals in the rows
    parts = [[ack_frame(0, msg), frame(ORIGINAL, 0, 4, data[4])],
             [frame(ORIGINAL, 0, 5, data[5]), ack_frame(1, msg), ack_frame(0, msg)],   # the second ack: no slot
             [ack_frame(2, msg)],                                                    # no encoder for flow 2
             [ack_frame(1, msg + bytes(20))]]                                        # longer than ackBytes 16
    built = [row_of(p, stride) for p in parts]
    dr = DevRows(L, [r for r, _ in built], stride, [n for _, n in built])
    assert len(msg) <= 16
    recs, words, slots, o = scan(L, dr.dev, stride, dr.lens, 4, m, 1, 16)
    decs = (C.c_void_p * 1)(extra.dec)
    encs = (C.c_void_p * 2)(a.enc, b.enc)
    before = (a.enc_stats()[6], b.enc_stats()[6])
    r, res, nxt, acc = recv(L, decs, encs, o, dr.dev, stride, 4, INVALID)
    assert res == [SUCCESS, SUCCESS, NEED_MORE, SUCCESS, SUCCESS, INVALID, INVALID, NEED_MORE, NEED_MORE,
                   INVALID, NEED_MORE, NEED_MORE], res
    assert acc == 4 and nxt[0] == 2 and nxt[4] == 2 and nxt[1] == 0xEEEE
    assert (a.enc_stats()[6], b.enc_stats()[6]) == (before[0] + 1, before[1] + 1)
    assert L.sgpu_decoder_has(extra.dec, 4) == SUCCESS and L.sgpu_decoder_has(extra.dec, 5) == SUCCESS
    # forged: records, words and slots are caller data
    good = bytes(o.raw)

    def forged(edit):
        raw = bytearray(good)
        edit(raw)
        C.memmove(o.out, bytes(raw), len(raw))
        return recv(L, decs, encs, o, dr.dev, stride, 4)

    def put(raw, k, j, **kw):
        h = PackedHead.from_buffer_copy(raw, REC * (k * m + j))
        for f, v in kw.items():
            setattr(h, f, v)
        raw[REC * (k * m + j):REC * (k * m + j + 1)] = bytes(h)
    for kw in (dict(PacketNum=1), dict(DataBytes=17), dict(DataBytes=0), dict(Status=ROW_TRUNCATED), dict(Status=4),
               dict(HeaderBytes=4), dict(HeaderBytes=9), dict(TailBytes=1), dict(Flow=1 << 24), dict(Offset=stride),
               dict(Head=(C.c_ubyte * 4)(1, 0, 0, 0))):
        r, res, _, acc = forged(lambda raw: put(raw, 0, 0, **kw))
        assert r == INVALID and res[0] == INVALID and res[1] == DUPLICATE, (kw, res)
    # a truncated record made to look whole: its slot holds a cut message
    r, res, _, _ = forged(lambda raw: put(raw, 3, 0, Status=ROW_OK))
    assert res[9] == INVALID
    r, res, _, _ = forged(lambda raw: put(raw, 1, 2, Status=ROW_OK))
    assert res[5] == INVALID
    acc = C.c_uint(0)
    for bad in (dict(m=0), dict(s=0), dict(s=4), dict(b=8), dict(heads=None), dict(stride=72), dict(acc=None)):
        g = dict(dict(m=m, s=1, b=16, heads=o.out, stride=stride, acc=C.byref(acc)), **bad)
        assert L.sgpu_frames_recv_duplex(decs, 1, encs, 2, g["heads"], g["m"], g["s"], g["b"], dr.dev, g["stride"], 4,
                                         None, None, g["acc"]) == INVALID, bad
    assert L.sgpu_frames_recv_duplex(decs, 1, None, 2, o.out, m, 1, 16, dr.dev, stride, 4, None, None,
                                     C.byref(acc)) == INVALID
    o.free()
    dr.free()
    for p in (a, b, extra):
        p.free()


DUPLICATE = 4


# 4 -------------------------------------------------------------------------
def check_loop(path):
    """8 flows on one device: the senders' k_frame rows, lost ones zeroed by
    their length, into the decoders; the decoders' ack rows through the duplex
    scan into the encoders; after the RTO the retransmission rows back into the
    decoders.  Every original arrives; no payload or ack byte crosses to the
    host but for the scan's records and slots."""
    L = load(path)
    flows, n, stride = 8, 12, 1232
    pairs = []
    for f in range(flows):
        data = [payload(7000 + 100 * f + i, variable_bytes(100 * f + i)) for i in range(n)]
        p = Pair(L, data)
        for i in range(n):
            assert p.add(i) == (SUCCESS, i)
        pairs.append(p)
    decs = (C.c_void_p * flows)(*[p.dec for p in pairs])
    encs = (C.c_void_p * flows)(*[p.enc for p in pairs])
    # forward: one original per row, all flows in one buffer
    fwd = Rows(L, flows * n, stride)
    lost = set()
    ch = Pcg(11, 5)
    for f, p in enumerate(pairs):
        res = (C.c_int * n)()
        q = C.c_uint(0)
        assert L.sgpu_encoder_deliver_range(p.enc, 0, n, f, fwd.dst + f * n * stride, stride, fwd.lens + 4 * f * n,
                                            res, C.byref(q)) == SUCCESS and q.value == n
        lost |= {f * n + i for i in range(1, n) if ch.next() % 100 < 30}
    assert L.sgpu_flush() == 0 and len(lost) >= flows
    for k in lost:   # the channel: a lost row's length word says so
        assert L.sgpu_h2d(fwd.lens + 4 * k, bytes(4), 4) == 0
    o = P.Out(L, flows * n, 1)
    t = L.sgpu_frames_scan_packed(fwd.dst, stride, fwd.lens, flows * n, 1, o.out)
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    acc = C.c_uint(0)
    assert L.sgpu_frames_recv_packed(decs, flows, o.out, 1, fwd.dst, stride, flows * n, None, C.byref(acc)) == SUCCESS
    assert acc.value == flows * n - len(lost)
    o.free()
    # back: one ack row per flow, through the duplex scan into the encoders
    back = Rows(L, flows, 64)
    fl = (C.c_uint * flows)(*range(flows))
    q = C.c_uint(0)
    assert L.sgpu_decoders_ack_frames(decs, flows, fl, 48, back.dst, 64, back.lens, None, C.byref(q)) == SUCCESS
    assert q.value == flows and L.sgpu_flush() == 0
    recs, words, slots, o = scan(L, back.dst, 64, back.lens, flows, 2, 1, 48)
    assert words == [1] * flows
    r, res, nxt, acc = recv(L, None, encs, o, back.dst, 64, flows, SUCCESS)
    assert acc == flows and res[0::2] == [SUCCESS] * flows
    for f in range(flows):
        firstLost = min(i for i in range(1, n + 1) if i == n or f * n + i in lost)
        assert nxt[2 * f] == firstLost
    o.free()
    time.sleep(RTO_SLEEP)
    # retransmissions: rows of several frames, back into the decoders
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
    assert L.sgpu_flush() == 0
    recs, words, slots, o = scan(L, re.dst, stride, re.lens, flows * maxRows, 8, 1, 16)
    r, res, nxt, acc = recv(L, decs, None, o, re.dst, stride, flows * maxRows)
    assert acc == sent and r in (SUCCESS, DUPLICATE)   # (a retransmission of a packet that did arrive)
    o.free()
    assert L.sgpu_flush() == 0
    # every original is there, byte for byte
    out = Rows(L, flows * n, stride)
    for f, p in enumerate(pairs):
        res = (C.c_int * n)()
        q = C.c_uint(0)
        assert L.sgpu_decoder_deliver_range(p.dec, 0, n, out.dst + f * n * stride, stride, out.lens + 4 * f * n, res,
                                            C.byref(q)) == SUCCESS
        assert q.value == n, "flow %d: %d of %d originals arrived" % (f, q.value, n)
    assert L.sgpu_flush() == 0
    got, lens = out.fetch()
    for f, p in enumerate(pairs):
        for i in range(n):
            k = f * n + i
            assert hashlib.sha256(got[k][:lens[k]]).digest() == hashlib.sha256(p.data[i]).digest(), (f, i)
    for r in (fwd, back, re, out):
        r.free()
    for p in pairs:
        p.free()
