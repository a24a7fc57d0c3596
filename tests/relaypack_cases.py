"""sgpu_decoder_pack_frames: the cases shared by test_relaypack_cpu.py (the CPU
test double, tests/hostsim) and test_relaypack_gpu.py (k_plan and k_pack on the
MI355X), driven through the C ABI with ctypes.

Expected bytes are built here from the originals each case feeds in,
sgpu_frame_write_header and layout(), a restatement of the packer's cursor
rule; where a sender holds the same packets they are the rows
sgpu_encoder_pack_frames wrote there.  Nothing expected comes from the call
under test.  Every case packs into rows with one guard row before and at least
one after, lengths and the info record with a guard on each side, everything
pre-filled with 0xA5 (deliver_cases.Rows, Info), and checks the guards.
"""
import ctypes as C
import random

import deliver_cases as D
import frame_cases as F
import pack_cases as P
import relay_cases as R
import scan_cases as SC
from deliver_cases import DISABLED, FILL, INVALID, NEED_MORE, PACKET_NUM_MAX, PENDING, SUCCESS, Rows, Stream
from frame_cases import FLOW, NONE, ORIGINAL
from relay_cases import framed
from siamese_amd.binding import bind_relay_pack_abi

STAT_RELAYS, STAT_PACKS = 25, 26
NSTATS = 27
TIMING_RELAY, TIMING_PLAN, TIMING_PACK = 9, 10, 11
WORD_FILL = 0xA5A5A5A5


def load(path):
    L = P.load(path)
    R.load(path)
    if getattr(L, "_relaypack_cases", False):
        return L
    # (the symbol under test: an AttributeError here is the parent's answer)
    bind_relay_pack_abi(L)
    L._relaypack_cases = True
    return L


def stats(L):
    v = (C.c_uint64 * NSTATS)()
    L.sgpu_engine_stats_ex(v, NSTATS)
    return list(v)


class Info:
    """The four info words between two 16-byte guards, all 0xA5."""

    def __init__(self, L):
        self.L = L
        self.base = L.sgpu_device_alloc(48)
        assert self.base and self.base % 16 == 0
        self.at = self.base + 16
        self.refill()

    def refill(self):
        assert self.L.sgpu_h2d(self.base, bytes([FILL]) * 48, 48) == 0

    def fetch(self):
        raw = D.read(self.L, self.base, 48)
        assert raw[:16] == bytes([FILL]) * 16 and raw[32:] == bytes([FILL]) * 16, "guards beside the info record"
        return [int.from_bytes(raw[16 + 4 * k:20 + 4 * k], "little") for k in range(4)]

    def untouched(self):
        return self.fetch() == [WORD_FILL] * 4

    def free(self):
        self.L.sgpu_device_free(self.base)


def pack(L, dec, flow, first, count, rows, maxRows, info, stride=None, dst=None, lens=None, infoAt=None, want=SUCCESS):
    res = (C.c_int * max(1, count))(*([-1] * max(1, count)))
    queued = C.c_uint(12345)
    r = L.sgpu_decoder_pack_frames(dec, flow, first, count, rows.dst if dst is None else dst,
                                   rows.stride if stride is None else stride, maxRows,
                                   rows.lens if lens is None else lens, info.at if infoAt is None else infoAt,
                                   res, C.byref(queued))
    assert r == want, "sgpu_decoder_pack_frames returned %d, expected %d" % (r, want)
    return list(res)[:count], queued.value


def layout(sizes, stride):
    """The packer's cursor rule: [(row, off)] of frames of `sizes` bytes, and the rows needed."""
    row = off = 0
    at = []
    for t in sizes:
        assert t <= stride
        if off + t > stride:
            row, off = row + 1, 0
        at.append((row, off))
        off = (off + t + 15) & ~15
    return at, (row + 1 if sizes else 0)


def expect(frames, stride, maxRows, unfit=0):
    """(rows [0, min(need, maxRows)), the maxRows length words, the info record)."""
    at, need = layout([len(f) for f in frames], stride)
    rows = [bytearray(stride) for _ in range(min(need, maxRows))]
    lens = [0] * maxRows
    written = 0
    for (r, o), f in zip(at, frames):
        if r < maxRows:
            rows[r][o:o + len(f)] = f
            lens[r] = o + len(f)
            written += 1
    return [bytes(r) for r in rows], lens, [need, written, unfit, len(frames) - written]


def check(rows, info, frames, maxRows, unfit=0, what="", beyond=None):
    """The buffer after a pack of `frames`: rows and lengths below
    min(need, maxRows) exact, the other length words below maxRows zero, every
    other row and word as `beyond` gives them (default: the 0xA5 fill)."""
    stride = rows.stride
    got, lens = rows.fetch()   # (the guard rows and words)
    wantRows, wantLens, wantInfo = expect(frames, stride, maxRows, unfit)
    assert info.fetch() == wantInfo, "%s: info %r, expected %r" % (what, info.fetch(), wantInfo)
    assert lens[:maxRows] == wantLens, "%s: length words" % what
    assert lens[maxRows:] == [WORD_FILL] * (rows.count - maxRows), "%s: a length word past maxRows was written" % what
    for r, w in enumerate(wantRows):
        assert got[r] == w, "%s: row %d differs from the layout rule's" % (what, r)
    for r in range(len(wantRows), rows.count):
        old = beyond[r] if beyond else bytes([FILL]) * stride
        assert got[r] == old, "%s: row %d past the rows written was touched" % (what, r)
    return got, lens, wantInfo


def frames_of(L, flow, first, data):
    return [framed(L, flow, first + k, d) for k, d in enumerate(data)]


# 1 -------------------------------------------------------------------------
EDGE_LENGTHS = R.EDGE_LENGTHS
EDGE_STRIDE = R.EDGE_STRIDE
# the same packets in ranges whose strides turn the row after nearly every frame
EDGE_RANGES = [(0, 10, 144), (10, 5, 16400), (15, 3, 32), (18, 3, 1040), (21, 3, 8208)]


def check_edge_lengths(path):
    L = load(path)
    st = Stream(L, EDGE_LENGTHS, seed=11)
    count = len(EDGE_LENGTHS)
    frames = frames_of(L, FLOW, 0, st.data)
    assert sorted(len(w) for w in frames[len(R.EDGE_N):]) == R.EDGE_T
    assert {len(w) - len(d) for w, d in zip(frames, st.data)} == {8, 9, 10}
    _, need = layout([len(f) for f in frames], EDGE_STRIDE)
    rows, info = Rows(L, need + 1, EDGE_STRIDE), Info(L)
    res, queued = pack(L, st.dec, FLOW, 0, count, rows, need + 1, info)
    assert res == [SUCCESS] * count and queued == count
    parts = []
    for first, n, stride in EDGE_RANGES:
        at, m = layout([len(f) for f in frames[first:first + n]], stride)
        pr, pi = Rows(L, m + 1, stride), Info(L)
        res, queued = pack(L, st.dec, FLOW, first, n, pr, m, pi)
        assert res == [SUCCESS] * n and queued == n
        parts.append((pr, pi, first, n, m))
    assert sum(n for _, n, _ in EDGE_RANGES) == count
    assert sum(p[4] for p in parts) >= count - 5, "the strides turn the row after nearly every frame"
    assert L.sgpu_flush() == 0
    check(rows, info, frames, need + 1, what="stride %d" % EDGE_STRIDE)
    for pr, pi, first, n, m in parts:
        check(pr, pi, frames[first:first + n], m, what="packets %d..%d, stride %d" % (first, first + n - 1, pr.stride))
        pr.free()
        pi.free()
    rows.free()
    info.free()
    st.free()


def check_exact_fits(path):
    """off + T == stride and one byte more, T == stride, and a frame longer
    than 8 KiB at a non-zero offset (a chunk edge inside its span)."""
    L = load(path)
    lengths = [100, 135, 100, 136, 247, 5]
    st = Stream(L, lengths, seed=12)
    frames = frames_of(L, 3, 0, st.data)
    at, need = layout([len(f) for f in frames], 256)
    assert at == [(0, 0), (0, 112), (1, 0), (2, 0), (3, 0), (4, 0)] and need == 5
    assert at[1][1] + len(frames[1]) == 256 and 112 + len(frames[3]) == 257 and len(frames[4]) == 256
    rows, info = Rows(L, need + 1, 256), Info(L)
    res, queued = pack(L, st.dec, 3, 0, len(lengths), rows, need, info)
    assert res == [SUCCESS] * len(lengths) and queued == len(lengths)
    big = Stream(L, [100, 9000, 5000, 40], seed=13)
    bframes = frames_of(L, 4, 0, big.data)
    bat, bneed = layout([len(f) for f in bframes], 16400)
    assert bat == [(0, 0), (0, 112), (0, 9136), (0, 14160)] and bneed == 1
    assert bat[2][1] - bat[1][1] > 8192, "the long frame's span crosses a chunk edge"
    brows, binfo = Rows(L, 2, 16400), Info(L)
    res, queued = pack(L, big.dec, 4, 0, 4, brows, 1, binfo)
    assert res == [SUCCESS] * 4 and queued == 4
    assert L.sgpu_flush() == 0
    check(rows, info, frames, need, what="exact fits, stride 256")
    check(brows, binfo, bframes, 1, what="a 9 KB frame at offset 112")
    for x in (rows, info, brows, binfo):
        x.free()
    st.free()
    big.free()


# 2 -------------------------------------------------------------------------
def small_lengths(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(1, 41) for _ in range(n)]


def check_plan_wave_edges(path):
    """63, 64, 65 and 129 packets of 1 to 40 bytes into rows of 256 bytes: the
    plan's 64-item batches end before, at and after the range's end."""
    L = load(path)
    for n in (63, 64, 65, 129):
        lengths = small_lengths(200 + n, n)
        st = Stream(L, lengths, seed=200 + n)
        frames = frames_of(L, n, 0, st.data)
        _, need = layout([len(f) for f in frames], 256)
        assert need >= 2
        rows, info = Rows(L, need + 2, 256), Info(L)
        s0 = stats(L)
        res, queued = pack(L, st.dec, n, 0, n, rows, need + 1, info)
        assert res == [SUCCESS] * n and queued == n
        assert L.sgpu_flush() == 0
        assert stats(L)[STAT_PACKS] - s0[STAT_PACKS] == n
        check(rows, info, frames, need + 1, what="%d packets" % n)
        rows.free()
        info.free()
        st.free()


JOB_STRIDES = [64, 256, 1408, 128, 512]


def check_jobs_one_submission(path, gpu):
    """3, 4 and 5 decoders packed by one submission (four jobs to a workgroup
    of k_plan), each into its own buffer at its own stride; and a submission
    that carries nothing but pack jobs."""
    L = load(path)
    streams = [Stream(L, small_lengths(300 + i, 30 + 7 * i), seed=300 + i) for i in range(5)]
    assert L.sgpu_flush() == 0
    for nd in (3, 4, 5):
        bufs = []
        L.sgpu_timing(1, 1, None, None)
        s0 = stats(L)
        t0 = L.sgpu_enqueue()
        for i in range(nd):
            st, stride = streams[i], JOB_STRIDES[i]
            frames = frames_of(L, i, 0, st.data)
            _, need = layout([len(f) for f in frames], stride)
            rows, info = Rows(L, need + 1, stride), Info(L)
            res, queued = pack(L, st.dec, i, 0, len(st.data), rows, need, info)
            assert res == [SUCCESS] * len(st.data) and queued == len(st.data)
            bufs.append((rows, info, frames, need))
        t1 = L.sgpu_enqueue()
        assert t1 > t0, "a submission of pack jobs alone must take a ticket"
        assert L.sgpu_wait(t1) == 0
        s1 = stats(L)
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 2), "one submission, the plan and the copy its only launches"
        assert s1[STAT_PACKS] - s0[STAT_PACKS] == sum(len(streams[i].data) for i in range(nd))
        assert s1[STAT_RELAYS] == s0[STAT_RELAYS]
        for i, (rows, info, frames, need) in enumerate(bufs):
            check(rows, info, frames, need, what="%d jobs, job %d" % (nd, i))
            rows.free()
            info.free()
        ms = (C.c_double * 12)()
        L.sgpu_timing_kernels(ms, 12)
        L.sgpu_timing(0, 1, None, None)
        if gpu:
            assert ms[TIMING_PLAN] > 0 and ms[TIMING_PACK] > 0, "k_plan and k_pack are timing indices 10 and 11"
            assert ms[TIMING_RELAY] == 0 and ms[5] == 0 and ms[6] == 0
    for st in streams:
        st.free()


# 3 -------------------------------------------------------------------------
def check_recovered(path, device):
    """Three of twelve originals recovered by a solve of the same submission
    as the pack (sgpu_decode), or through sgpu_decode_device."""
    L = load(path)
    st = Stream(L, R.REC_LENGTHS, lost=R.REC_LOST, recovery=4, seed=22)
    frames = frames_of(L, 7, 0, st.data)
    assert {(F.prefix_bytes(len(st.data[k])), len(frames[k]) - len(st.data[k])) for k in R.REC_LOST} == \
        {(1, 8), (1, 9), (2, 9)}
    _, need = layout([len(f) for f in frames], R.REC_STRIDE)
    assert 2 <= need < 12
    rows, info = Rows(L, need + 1, R.REC_STRIDE), Info(L)
    R.decode_lost(L, st, device, len(R.REC_LOST))
    res, queued = pack(L, st.dec, 7, 0, 12, rows, need, info)   # (before any flush of the solve)
    assert res == [SUCCESS] * 12 and queued == 12
    assert L.sgpu_flush() == 0
    check(rows, info, frames, need, what="three packets recovered in the submission")
    rows.free()
    info.free()
    st.free()


# 4, 5 ----------------------------------------------------------------------
HOP_STRIDE = 1408


def check_byte_identity(path):
    """The relay's rows, lengths and row count are the sender's."""
    L = load(path)
    hop = R.Hop(L, seed=31)
    frames = frames_of(L, FLOW, 0, hop.sn.data)
    _, need = layout([len(f) for f in frames], HOP_STRIDE)
    assert 2 <= need < hop.count
    sent, relayed, info = Rows(L, need + 1, HOP_STRIDE), Rows(L, need + 1, HOP_STRIDE), Info(L)
    res, nrows, nframes = P.pack(L, hop.sn.enc, FLOW, 0, hop.count, None, 0, sent, need + 1)
    assert res == [SUCCESS] * hop.count and (nrows, nframes) == (need, hop.count)
    res, queued = pack(L, hop.dec, FLOW, 0, hop.count, relayed, need + 1, info)   # (the solve rides in this submission)
    assert res == [SUCCESS] * hop.count and queued == hop.count
    assert L.sgpu_flush() == 0
    a, alens = sent.fetch()
    b, blens = relayed.fetch()
    assert info.fetch() == [nrows, nframes, 0, 0]
    assert alens == blens, "the relay's lengths differ from the sender's"
    for r in range(need + 1):
        assert a[r] == b[r], "row %d: the relay's differs from the sender's" % r
    check(relayed, info, frames, need + 1, what="the relay's rows")
    for x in (sent, relayed, info):
        x.free()
    hop.free()


def check_second_hop(path):
    """The relay's packed rows into the next hop's decoder without a host copy
    of a payload, and the same bytes through sgpu_frames_parse on the host."""
    L = load(path)
    hop = R.Hop(L, seed=41)
    count, stride, flow, maxFrames = hop.count, HOP_STRIDE, 0, 16
    frames = frames_of(L, flow, 0, hop.sn.data)
    at, need = layout([len(f) for f in frames], stride)
    rows, info = Rows(L, need + 1, stride), Info(L)
    res, queued = pack(L, hop.dec, flow, 0, count, rows, need + 1, info)
    assert res == [SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    got, lens, _ = check(rows, info, frames, need + 1, what="the relay's rows")
    # the next hop: scan, then receive from the records
    recs, words, o = P.scan(L, rows.dst, stride, rows.lens, need + 1, maxFrames)
    want = [P.expected_row(L, got[r], stride, lens[r], maxFrames) for r in range(need + 1)]
    assert (recs, words) == ([w[0] for w in want], [w[1] for w in want])
    assert sum(words) == count and words[need] == 0
    nxt = L.sgpu_decoder_create()
    m = C.c_uint(0)
    assert L.sgpu_frames_recv_packed((C.c_void_p * 1)(nxt), 1, o.out, maxFrames, rows.dst, stride, need + 1, None,
                                     C.byref(m)) == SUCCESS
    assert m.value == count
    back, tails = SC.delivered(L, nxt, count, stride)
    assert back == hop.sn.data, "the next hop's packets are the source's"
    assert all(t == bytes(len(t)) for t in tails)
    # the same rows on the host
    wire = b"".join(got[:need])
    r, fr = P.parse(L, wire)
    assert r == SUCCESS and len(fr) == count
    for k, f in enumerate(fr):
        assert (f.Type, f.Flow, f.PacketNum, f.Bytes) == (ORIGINAL, flow, k, len(hop.sn.data[k])), "frame %d" % k
        assert wire[f.Offset:f.Offset + f.Bytes] == hop.sn.data[k]
        assert f.Offset == at[k][0] * stride + at[k][1] + len(frames[k]) - f.Bytes
    L.sgpu_decoder_free(nxt)
    assert L.sgpu_flush() == 0
    o.free()
    rows.free()
    info.free()
    hop.free()


# 6 -------------------------------------------------------------------------
def check_absent(path):
    L = load(path)
    lengths = [60 + 7 * i for i in range(10)]
    lost = (3, 8)
    stride = 256
    st = Stream(L, lengths, lost=lost, seed=33)
    frames = frames_of(L, 5, 0, st.data)
    have = [f for k, f in enumerate(frames) if k not in lost]
    _, needAll = layout([len(f) for f in frames], stride)
    maxRows = needAll + 1
    rows, info = Rows(L, maxRows + 1, stride), Info(L)
    s0 = stats(L)
    res, queued = pack(L, st.dec, 5, 0, 10, rows, maxRows, info)
    assert res == [NEED_MORE if k in lost else SUCCESS for k in range(10)] and queued == 8
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_PACKS] - s0[STAT_PACKS] == 10, "absent packets' items are counted"
    check(rows, info, have, maxRows, what="two packets absent")
    # the stream fills in: the same buffer again, its rows rewritten whole
    for k in lost:
        assert L.sgpu_decoder_add_original(st.dec, k, st.at(k), lengths[k]) == SUCCESS
    res, queued = pack(L, st.dec, 5, 0, 10, rows, maxRows, info)
    assert res == [SUCCESS] * 10 and queued == 10
    assert L.sgpu_flush() == 0
    full, _, _ = check(rows, info, frames, maxRows, what="all ten packets")
    # a range that starts in the stream and runs past its end needs fewer rows:
    # the stale length words are zeroed, the stale rows left as they are
    res, queued = pack(L, st.dec, 5, 6, 8, rows, maxRows, info)
    assert res == [SUCCESS] * 4 + [NEED_MORE] * 4 and queued == 4
    assert L.sgpu_flush() == 0
    tail = frames_of(L, 5, 6, st.data[6:])
    _, needTail = layout([len(f) for f in tail], stride)
    assert needTail < needAll
    check(rows, info, tail, maxRows, what="packets 6..9", beyond=full)
    # nothing present: no row, every length word zero
    res, queued = pack(L, st.dec, 5, 10, 5, rows, maxRows, info)
    assert res == [NEED_MORE] * 5 and queued == 0
    assert L.sgpu_flush() == 0
    now, _ = rows.fetch()
    check(rows, info, [], maxRows, what="nothing present", beyond=now)
    assert info.fetch() == [0, 0, 0, 0]
    rows.free()
    info.free()
    st.free()


# 7 -------------------------------------------------------------------------
def check_does_not_fit(path):
    """A recovered 1000-byte packet into rows of 1008: its frame is 1009 bytes.
    Skipped on the device while the length is pending, the frames behind it
    closing up; refused by the call once the length is known."""
    L = load(path)
    st = Stream(L, [100, 1000, 50], lost=(1,), recovery=1, seed=44)
    frames = frames_of(L, FLOW, 0, st.data)
    assert len(frames[1]) == 1009
    rows, info = Rows(L, 3, 1008), Info(L)
    assert st.decode() == (SUCCESS, 1)
    res, queued = pack(L, st.dec, FLOW, 0, 3, rows, 2, info)
    assert res == [SUCCESS] * 3 and queued == 3
    assert L.sgpu_flush() == 0
    _, _, wantInfo = check(rows, info, [frames[0], frames[2]], 2, unfit=1, what="the 1000-byte packet skipped")
    assert wantInfo == [1, 2, 1, 0]
    # the length is known now
    rows.refill()
    info.refill()
    s0 = stats(L)
    _, queued = pack(L, st.dec, FLOW, 0, 3, rows, 2, info, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_PACKS] == s0[STAT_PACKS]
    assert rows.untouched() and info.untouched()
    wide = Rows(L, 3, 1024)
    res, queued = pack(L, st.dec, FLOW, 0, 3, wide, 2, info)
    assert res == [SUCCESS] * 3 and queued == 3
    assert L.sgpu_flush() == 0
    check(wide, info, frames, 2, what="rows of 1024")
    for x in (rows, wide, info):
        x.free()
    st.free()


# 8 -------------------------------------------------------------------------
def check_too_few_rows(path):
    L = load(path)
    lengths = [90 + 11 * i for i in range(12)]
    stride = 256
    st = Stream(L, lengths, seed=66)
    frames = frames_of(L, 9, 0, st.data)
    at, need = layout([len(f) for f in frames], stride)
    assert need >= 4
    dropped = sum(1 for r, _ in at if r >= need - 1)
    rows, info = Rows(L, need, stride), Info(L)   # (row need - 1 is a guard row here)
    res, queued = pack(L, st.dec, 9, 0, 12, rows, need - 1, info)
    assert res == [SUCCESS] * 12 and queued == 12
    assert L.sgpu_flush() == 0
    _, _, wantInfo = check(rows, info, frames, need - 1, what="one row short")
    assert wantInfo == [need, 12 - dropped, 0, dropped]
    # no rows at all: only the info record is written
    rows.refill()
    info.refill()
    for kw in (dict(), dict(dst=0, lens=0)):
        res, queued = pack(L, st.dec, 9, 0, 12, rows, 0, info, **kw)
        assert res == [SUCCESS] * 12 and queued == 12
        assert L.sgpu_flush() == 0
        assert info.fetch() == [need, 0, 0, 12]
        assert rows.untouched()
        info.refill()
    rows.free()
    info.free()
    st.free()


# 9 -------------------------------------------------------------------------
def check_arguments(path):
    L = load(path)
    st = Stream(L, [1400, 200, 300, 400], seed=55)
    rows, info = Rows(L, 4, 1408), Info(L)
    s0 = stats(L)
    bad = [
        ("null decoder", dict(dec=None)),
        ("null rows", dict(dst=0)),
        ("null lengths", dict(lens=0)),
        ("null info", dict(infoAt=0)),
        ("info not 16-byte aligned", dict(infoAt=info.at + 4)),
        ("rows not 16-byte aligned", dict(dst=rows.dst + 8)),
        ("stride zero", dict(stride=0)),
        ("stride no multiple of 16", dict(stride=1400)),
        ("stride above 4 GiB", dict(stride=(1 << 32) + 16)),
        ("lengths not 4-byte aligned", dict(lens=rows.lens + 2)),
        ("first packet number past the maximum", dict(first=PACKET_NUM_MAX + 1)),
        ("flow above 2^24 - 1", dict(flow=1 << 24)),
        ("SGPU_FRAME_NONE", dict(flow=NONE)),
        ("more than 65535 packets", dict(count=65536)),
    ]
    for what, kw in bad:
        dec = kw.pop("dec", st.dec)
        first = kw.pop("first", 1)
        flow = kw.pop("flow", FLOW)
        count = kw.pop("count", 3)
        _, queued = pack(L, dec, flow, first, count, rows, 3, info, want=INVALID, **kw)
        assert queued == 0, what
    # a row one byte too short for a packet of known length: 9 + 1400 = 1408 + 1
    assert len(framed(L, FLOW, 0, st.data[0])) == rows.stride + 1
    _, queued = pack(L, st.dec, FLOW, 0, 4, rows, 3, info, want=INVALID)
    assert queued == 0
    # a decoder with a device matrix job pending
    job = Stream(L, R.REC_LENGTHS, lost=R.REC_LOST, recovery=4, seed=56)
    jrows = Rows(L, 12, R.REC_STRIDE)
    r, _ = job.decode(device=True)
    assert r == PENDING
    _, queued = pack(L, job.dec, FLOW, 0, 12, jrows, 12, info, want=INVALID)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert job.decode(device=True) == (SUCCESS, len(R.REC_LOST))
    assert L.sgpu_flush() == 0
    # nothing was queued by any of them
    assert stats(L)[STAT_PACKS] == s0[STAT_PACKS]
    assert rows.untouched() and jrows.untouched() and info.untouched()
    # a dead decoder
    sn, dead = R.dead_decoder(L)
    _, queued = pack(L, dead, FLOW, 0, 2, rows, 3, info, want=DISABLED)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert rows.untouched() and info.untouched()
    L.sgpu_decoder_free(dead)
    sn.free()
    # count == 0: no row, the maxRows length words zeroed, a zero info record
    _, queued = pack(L, st.dec, FLOW, 0, 0, rows, 3, info)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_PACKS] == s0[STAT_PACKS]
    check(rows, info, [], 3, what="count == 0")
    info.refill()
    _, queued = pack(L, st.dec, FLOW, 0, 0, rows, 0, info, dst=0, lens=0)
    assert queued == 0
    assert L.sgpu_flush() == 0
    assert info.fetch() == [0, 0, 0, 0]
    # (the arguments were fine otherwise: the largest flow, 65535 packets of which three exist)
    rows.refill()
    res, queued = pack(L, st.dec, (1 << 24) - 1, 1, 65535, rows, 3, info)
    assert res == [SUCCESS] * 3 + [NEED_MORE] * 65532 and queued == 3
    assert L.sgpu_flush() == 0
    assert stats(L)[STAT_PACKS] - s0[STAT_PACKS] == 65535
    check(rows, info, frames_of(L, (1 << 24) - 1, 1, st.data[1:]), 3, what="the largest flow")
    for x in (rows, jrows, info):
        x.free()
    job.free()
    st.free()
