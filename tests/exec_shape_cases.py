"""k_exec's row-batch modes at window-shape edges: the cases shared by
test_exec_shapes_cpu.py (the CPU test double, tests/hostsim) and
test_exec_shapes_gpu.py (the HIP kernels on the MI355X), driven through the
siamese_gpu.h ABI with ctypes like size_cases.py.

size_cases.py moves the byte length of the symbols; this file moves the shape
of the OP_ROWS batches (ops.h) that the executor's modes are selected by.  A
case is a schedule, a list of steps on one encoder:

  ("add", k)            k sgpu_encoder_add calls
  ("encode", k)         k sgpu_encode calls, one packet each (not
                        sgpu_encode_range: rows are made between adds)
  ("remove_before", n)  sgpu_encoder_remove_before(n)

all queued without a flush, so the rows join batches as Program::rows_update
and Program::rows_row (engine.cpp) let them.  A packet is valid until the next
sgpu_encode only, so each is handed to the decoder (sgpu_decoder_add_recovery)
and copied bare into a guarded row of the test's own
(sgpu_frames_deliver_recovery: DeviceData read by the submission that wrote
it) as soon as it is made; the decoder takes the originals it receives as they
are added.  Then one flush, the decode (sgpu_decode, or sgpu_decode_device:
PENDING, flush, Success), and the delivery of every original the decoder
holds.  Checked, most independent first:

  1. every recovery packet (DataBytes, FooterBytes, sha256 of its bytes)
     against the reference's packets for the same schedule, recorded in
     tests/golden/exec_shapes.json by tests/golden/make_exec_shape_golden.py
     -- and against a live run of the reference where oracle/_ref is built;
  2. the decode returns Success with exactly the lost packets;
  3. every delivered row is the original this file generated, its length word
     right, its tail zero up to the stride, the guards intact;
  4. the engine counters (sgpu_engine_stats_ex [30..35], counted when the
     submission is laid out) show the batches the case is named for.

Symbol lengths cycle through LENGTHS: both sides of the 16-byte lane and of
the 256-byte executor tile, and 600 bytes, three tiles, so that sums grow
between rows, rows are shorter than their sums (the zero-tail rule of ops.h)
and the per-tile stage prefetch of k_exec (ti > 0) runs.  Payloads are
size_cases.payloads: SHAKE-256 of the seed and the packet's index.

What selects each mode (backend_hip.hip unless said otherwise), with
B = the batch's block words, kRowSums + (E - stageLo) + 2 U + 3 R for a
window snapshot of E entries read from element stageLo on, U sum updates and
R rows:

  versioned   an update joins a batch in which a row already read its sum
              (Program::rows_update): RowItem.cutoff, corrL; at most
              kVersionRows = 16 rows, kVersionMaxSpan = 32 elements per
              joining update, and only while the sum's buffer stays put and
              keeps the bytes the rows saw
  Fit         B <= kRowsTableLds = 1024 (ops.h): the whole block in the LDS
              table; else the words past it are read from the stream
  staged      E - stageLo <= the stage capacity (stats [35], from the
              device's LDS less k_exec's static LDS): else the elements past
              it are read from memory (kPlanGeneral rows, phase B1b)
  lane mode   decided on the device, no counter: for every window lane l the
              three sums 3l..3l+2 are updated over one staged element range,
              or none of them is.  An encoder folds into a sum only when a row
              selects it (EncoderCore::siamese_row_body), and a row selects
              about half of the 24 by its opcodes, so a batch of one or two
              rows over fresh sums updates part of some lane's three: the
              dword layout.  Sixteen rows or more over one window between
              them select every sum, each folded once over [base, base + E):
              lane mode.  The cases say which they are below.
  waves       R < kExecWaves = 16: a row's picks are split over 16 / R waves
              by PCG jump-ahead; R >= 16: whole rows per wave; rows past
              kPlanRows = 256 get no plan, terms past kPlanCap = 8192 none
  column      CX(column mod kColumnValuePeriod = 253) while the element index
              runs on
"""
import ctypes as C
import hashlib
import json
import os

import deliver_cases as D
import scenario_lib as S
import size_cases as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exec_shapes.json")

LENGTHS = [1, 15, 16, 17, 255, 256, 257, 600]
LONG = 600


def lengths(count, a=3, b=0):
    return Z.edge(count, a, b, LENGTHS)


def every(n, k, count):
    """The indices below count that are k mod n."""
    return tuple(range(k, count, n))


class Case:
    """enc / dec: the growth the encoder's schedule (up to its flush) and the
    decode (from there to the end) must show in the rows_* counters, keys
    without the rows_ prefix; a key left out is not asserted."""

    def __init__(self, seed, schedule, lost, lens=None, enc=None, dec=None):
        self.seed, self.schedule, self.lost = seed, tuple(tuple(s) for s in schedule), tuple(lost)
        count = sum(k for op, k in self.schedule if op == "add")
        self.lengths = tuple(lens) if lens is not None else lengths(count, 3, seed)
        self.recovery = sum(k for op, k in self.schedule if op == "encode")
        self.enc, self.dec = enc or {}, dec or {}
        assert len(self.lengths) == count
        assert all(op in ("add", "encode", "remove_before") for op, _ in self.schedule)
        assert len(set(self.lost)) == len(self.lost) <= self.recovery and max(self.lost) < count, \
            "lost packets: distinct indices of the stream, no more of them than recovery packets"
        assert max(self.lengths[i] for i in self.lost) + 3 > (max(self.lengths) + 2) // 256 * 256, \
            "a lost packet must end in the last 256-byte tile of the longest symbol: " \
            "otherwise the solve's last tile recovers only zeros and a solve that skips it passes"
        # every row is a Siamese row: more than kCauchyThreshold (codedef.h)
        # originals in flight at the first encode and at every later one
        added = first = 0
        for op, k in self.schedule:
            if op == "add":
                added += k
            elif op == "remove_before":
                first = max(first, k)
            else:
                assert added - first > 64, "a window of %d: Cauchy rows" % (added - first)
                assert added - first < 512, "a window of %d: its picks go to k_ldpc" % (added - first)

    def kept_from(self):
        """The first original the encoder still holds at the end."""
        return max([n for op, n in self.schedule if op == "remove_before"] or [0])

    def schedule_sha256(self):
        return hashlib.sha256(json.dumps([list(s) for s in self.schedule]).encode()).hexdigest()


def long_at(seed):
    """lengths(count, 3, seed)[i] is 600 for i = long_at(seed) mod 8."""
    return 3 * (7 - seed) % 8


def lose(seed, *idx):
    """idx, its second entry moved up to the next 600-byte original of
    lengths(count, 3, seed)."""
    i = idx[1] + (long_at(seed) - idx[1]) % 8
    assert i not in idx[:1] + idx[2:]
    return idx[:1] + (i,) + idx[2:]


def joins(rows, step=2, first=70):
    return [("add", first)] + [("add", step), ("encode", 1)] * rows


def window(w, rows=3):
    return [("add", w), ("encode", rows)]


def lost_long(case_lengths, want, lo=0, hi=None):
    """`want` indices of 600-byte originals in [lo, hi), spread evenly."""
    hi = len(case_lengths) if hi is None else hi
    at = [i for i in range(lo, hi) if case_lengths[i] == LONG]
    assert len(at) >= want
    return tuple(at[k * len(at) // want] for k in range(want))


def _window_case(seed, w):
    lens = lengths(w, 3, seed)
    # one batch of three rows (no update joins after a row read its sum: the
    # window does not move), block 24 + w + 2 U + 9 <= 24 + 511 + 48 + 9 < 1024
    return Case(seed, window(w), lost_long(lens, 2), lens=lens,
                enc=dict(batches=1, versioned=0, versioned_rows=0, unfit=0))


# The windows of the sweep: 167 / 168, the capacity edge of a 48 KiB stage
# (48 * 1024 / 256 - 25 = 167 elements: what be_init falls back to when the
# device refuses the larger one); 256, 384 and 448 between; 511, the last
# window before kLdpcSplitMin = 512 sends a row's picks to k_ldpc; and 356,
# 357, 358 around the stage capacity an MI355X reports, 357 (DESIGN.md
# section 4): test_exec_shapes_gpu.py picks the windows of its stage_edge test
# from the capacity the library reports, and these are the ones it finds.
SWEEP = (167, 168, 169, 256, 384, 448, 511)
STAGE_WINDOWS = (356, 357, 358)

# What each schedule makes of its batches, from the rules above.  E counts
# the window entries of the snapshot, which only grows while batches of one
# program follow each other (rows_open with keepWindow).
CASES = {
    # Row 0 is made over 72 originals: fresh sums, no row has read them, so
    # its updates do not make the batch versioned.  Every later row folds two
    # more originals into the sums it selects; from row 1 on some of those
    # were read by an earlier row: the update joins (2 <= kVersionMaxSpan,
    # fewer than kVersionRows rows so far) and the batch is versioned.  15 rows:
    # one versioned batch below the row limit.  The symbols come in lengths up
    # to 600 from the start, so no sum moves.  One or two rows' selections per
    # update round: not lane mode.  R = 15 < 16: picks split by jump-ahead.
    "join15": Case(11, joins(15), lose(11, 3, 40, 75, 99), enc=dict(batches=1, versioned=1, versioned_rows=15, unfit=0)),
    # exactly kVersionRows rows: still one batch, corrL full
    "join16": Case(12, joins(16), lose(12, 2, 41, 74, 101), enc=dict(batches=1, versioned=1, versioned_rows=16, unfit=0)),
    # the 17th row's joining updates find kVersionRows rows in the batch and
    # open the next one, which holds that row alone: nothing joins it
    "join17": Case(13, joins(17), lose(13, 1, 42, 73, 103), enc=dict(batches=2, versioned=1, versioned_rows=16, unfit=0)),
    # One joining update of exactly kVersionMaxSpan elements: an update takes
    # every 8th element of its lane, so an add of k originals gives each lane's
    # sums a range of k or k - 7 .. k elements end to end; rows_update measures
    # toElement - fromElement, the lane's range rounded up to whole strides of
    # 8 (EncoderCore::get_sum): 32 for an add of 25 to 32 originals, 40 for 33.
    # span32: row 0 over 72, then 32 more and row 1: joins, two versioned rows.
    "span32": Case(14, [("add", 72), ("encode", 1), ("add", 32), ("encode", 1)], lose(14, 5, 90),
                   enc=dict(batches=1, versioned=1, versioned_rows=2)),
    # span33: 33 more: the first update that would join spans 40 > 32 and opens
    # a new batch; two batches of one row, neither versioned.
    "span33": Case(15, [("add", 72), ("encode", 1), ("add", 33), ("encode", 1)], lose(15, 4, 95),
                   enc=dict(batches=2, versioned=0, versioned_rows=0)),
    # Steps of one original: each row's joining updates touch one lane only
    # (element e belongs to lane e mod 8) and only the sums of it the row
    # selects, seldom all three: the dword layout, not lane mode.
    "span1_lane": Case(16, joins(8, step=1), lose(16, 6, 33, 71), enc=dict(batches=1, versioned=1, versioned_rows=8)),
    # Steps of eight: every lane gets one new element per row, the ranges of
    # all updates equal in length.  Whether a round is in lane mode still
    # depends on the row selecting whole lanes; the batch as a whole carries
    # one update per sum over its joined range.
    "span8_lane": Case(17, joins(8, step=8), lose(17, 7, 44, 90, 130), enc=dict(batches=1, versioned=1, versioned_rows=8)),
    # 72 originals of at most 257 bytes, row 0; then two of 600 bytes and row
    # 1: the sums it selects grow past their buffers (EncoderCore::grow_sum
    # moves them), `seen.src != dst`, so the join is refused and a new batch
    # opens.  No versioned batch, although the span is 2.
    "grow": Case(18, [("add", 72), ("encode", 1), ("add", 2), ("encode", 1), ("add", 2), ("encode", 2)],
                 (10, 72, 73), lens=tuple(n for n in lengths(90, 3, 2) if n != LONG)[:72] + (LONG, LONG, 17, 255),
                 enc=dict(versioned_rows=0)),
    # Three rows after all 96 adds: one batch, the sums filling in as each row
    # selects more of them (an update of a sum no row has read joins without
    # versions).  R = 3: each row's picks split over 16 / 3 = 5 waves.
    "rows_few": Case(19, window(96, 3), lose(19, 8, 57), enc=dict(batches=1, versioned=0, unfit=0)),
    # R = 16 and R = 40: whole rows per wave; between them the rows select all
    # 24 sums, each folded once over [0, 96): lane mode.
    "rows_waves": Case(20, window(96, 16), lose(20, 0, 9, 58, 95), enc=dict(batches=1, versioned=0, unfit=0)),
    "rows_waves40": Case(21, window(96, 40), every(7, 0, 96), enc=dict(batches=1, versioned=0, unfit=0)),
    # 300 rows over a window of 100 in one batch: R > kPlanRows = 256, rows 256
    # to 299 unplanned; B = 24 + 100 + 2 * 24 + 3 * 300 = 1072 > 1024: not Fit.
    "rows300": Case(22, window(100, 300), tuple(i for i in range(100) if i % 8 != 4),
                    enc=dict(batches=1, versioned=0, unfit=1)),
    # B = 24 + 112 + 2 * 24 + 3 * 280 = 1024 exactly: Fit, the table full ...
    "fit_edge": Case(23, window(112, 280), every(7, 1, 112), enc=dict(batches=1, unfit=0)),
    # ... and 1025 with one more window entry: the last word read from the stream
    "fit_edge1": Case(24, window(113, 280), every(7, 2, 113), enc=dict(batches=1, unfit=1)),
    # remove_before(150) between the rows: the rows after it draw their picks
    # from element 150 on and fold only the new originals, so the batch reads
    # the tail of its snapshot: stageLo > 0, and the window's base is not 0.
    "trimmed": Case(25, [("add", 200), ("encode", 4), ("remove_before", 150), ("add", 30), ("encode", 4)],
                    lose(25, 151, 160, 199, 215, 229)),
    # the same with packet numbers 253 and 506 inside the live window
    # [240, 530): CX's column wraps twice, the element index does not
    # (two trims: the reference's decoder takes this stream, but not the one
    # that keeps its sums running from packet 0 through the trim at 240)
    "trimmed_wrap": Case(26, [("add", 100), ("encode", 2), ("remove_before", 100), ("add", 150), ("encode", 2),
                              ("remove_before", 240), ("add", 280), ("encode", 6)],
                         (252, 253, 505, 506, 512 + long_at(26))),
    # The decoder's side: the packets of join16's schedule each cover another
    # window, [0, 72 + 2 i), and the first and last originals are lost, so the
    # elimination of received data from each row (decoder.cpp's rows_update
    # callers) runs over ranges with absent elements at both ends, another
    # range per row.
    "dec_windows": Case(27, joins(16), (0, 1, 2, long_at(27) + 8, 97, 99, 101)),
}
for _k, _w in enumerate(SWEEP + STAGE_WINDOWS):
    CASES["window_%d" % _w] = _window_case(30 + _k, _w)


def describe(packets, case):
    """What exec_shapes.json records of a case: size_cases.describe, the
    payload of each packet as long as the longest symbol its encoder held
    when it was made, and the schedule's hash."""
    longest, added, first, k = [], 0, 0, 0
    for op, n in case.schedule:
        if op == "add":
            added += n
        elif op == "remove_before":
            first = max(first, n)
        else:
            longest += [max(Z.prefix_bytes(x) + x for x in case.lengths[first:added])] * n
    return {
        "originals": len(case.lengths),
        "lengths_sha256": hashlib.sha256(json.dumps(case.lengths).encode()).hexdigest(),
        "schedule_sha256": case.schedule_sha256(),
        "lost": list(case.lost),
        "recovery": [{"bytes": len(p), "footer_bytes": len(p) - longest[k], "sha256": hashlib.sha256(p).hexdigest()}
                     for k, p in enumerate(packets)],
    }


def reference_run(case, data):
    """The schedule through the reference's siamese.h API: its recovery
    packets, and what its decoder recovers from them (fed in the order the
    device's decoder is)."""
    lib = Z.binding().SiameseLib(S.REF_LIB).init()
    enc, dec = lib.Encoder(), lib.Decoder()
    packets, added = [], 0
    for op, n in case.schedule:
        if op == "add":
            for i in range(added, added + n):
                assert enc.add(data[i]) == i
                if i not in case.lost:
                    assert dec.add_original(i, data[i]) == 0
            added += n
        elif op == "remove_before":
            assert enc.remove_before(n) == 0
        else:
            for _ in range(n):
                p = enc.encode()
                assert p
                packets.append(p)
                assert dec.add_recovery(p) == 0
    # (a decode solves the earliest packets that suffice for the losses they
    # cover: a stream whose later losses only later packets cover takes
    # several)
    recovered = []
    for _ in range(len(case.lost)):
        more = dec.decode()
        if not more:
            break
        recovered += more
    enc.close()
    dec.close()
    return packets, recovered


_expected = {}


def expected(name):
    """The case's payloads and its recovery packets as recorded; where the
    reference is built, a live run of it must agree with the record first."""
    if name not in _expected:
        case = CASES[name]
        data = Z.payloads(case)
        with open(GOLDEN) as f:
            cases = json.load(f)["cases"]
        assert name in cases, "%s is not in exec_shapes.json: run tests/golden/make_exec_shape_golden.py" % name
        want = cases[name]
        mine = describe([], case)
        for key in ("originals", "lengths_sha256", "schedule_sha256", "lost"):
            assert want[key] == mine[key], "%s: exec_shapes.json was made for other %s: run " \
                "tests/golden/make_exec_shape_golden.py" % (name, key)
        assert len(want["recovery"]) == case.recovery
        if os.path.exists(S.REF_LIB):
            packets, _ = reference_run(case, data)
            assert describe(packets, case) == want, "exec_shapes.json is stale: run " \
                "tests/golden/make_exec_shape_golden.py"
        _expected[name] = (data, want)
    return _expected[name]


def bind(L):
    L.sgpu_encode.argtypes = [C.c_void_p, C.c_void_p]
    L.sgpu_encoder_remove_before.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_frames_deliver_recovery.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p]
    return L


def stage_cap(path):
    """The executor's stage capacity in window elements as the library
    reports it (0: the backend has no stage)."""
    return Z.engine(D.load(path))["stage_cap"]


class Run:
    """A case's schedule queued on one encoder and one decoder, unflushed.
    With `schedule`, only that much of it: play() queues more later
    (ge_cases.py: a decode between two parts of a stream)."""

    def __init__(self, L, case, data, schedule=None):
        self.L, self.case, self.data = L, case, data
        count = len(case.lengths)
        # (originals at odd device addresses, as deliver_cases.Stream lays them out)
        self.pitch = ((max(case.lengths) + 34) & ~15) + 2
        blob = bytearray(3 + self.pitch * count)
        for i, d in enumerate(data):
            blob[3 + i * self.pitch:3 + i * self.pitch + len(d)] = d
        self.src = L.sgpu_device_alloc(len(blob))
        assert self.src and L.sgpu_h2d(self.src, bytes(blob), len(blob)) == 0
        self.enc = L.sgpu_encoder_create()
        self.dec = L.sgpu_decoder_create()
        assert self.enc and self.dec
        # recovery packet k bare in row k: the longest symbol and its footer fit
        self.recRows = D.Rows(L, case.recovery, (max(case.lengths) + 3 + 8 + 15) & ~15)
        self.recs = (D.Rec * case.recovery)()
        self.added = self.made = 0
        self.play(case.schedule if schedule is None else schedule)

    def play(self, schedule):
        L, case, data = self.L, self.case, self.data
        for op, n in schedule:
            if op == "add":
                for i in range(self.added, self.added + n):
                    num = C.c_uint(0)
                    assert L.sgpu_encoder_add(self.enc, self.at(i), len(data[i]), C.byref(num)) == D.SUCCESS
                    assert num.value == i
                    if i not in case.lost:
                        assert L.sgpu_decoder_add_original(self.dec, i, self.at(i), len(data[i])) == D.SUCCESS
                self.added += n
            elif op == "remove_before":
                assert L.sgpu_encoder_remove_before(self.enc, n) == D.SUCCESS
            else:
                for _ in range(n):
                    made = self.made
                    r = self.recs[made]
                    assert L.sgpu_encode(self.enc, C.byref(r)) == D.SUCCESS
                    queued = C.c_uint(0)
                    assert L.sgpu_frames_deliver_recovery(
                        1, C.byref(r), None, self.recRows.dst + made * self.recRows.stride, self.recRows.stride,
                        self.recRows.lens + 4 * made, C.byref(queued)) == D.SUCCESS and queued.value == 1
                    assert L.sgpu_decoder_add_recovery(self.dec, C.byref(r)) == D.SUCCESS
                    self.made += 1

    def at(self, i):
        return self.src + 3 + i * self.pitch

    def decode(self, device=False):
        out, n = C.c_void_p(), C.c_uint(0)
        f = self.L.sgpu_decode_device if device else self.L.sgpu_decode
        return f(self.dec, C.byref(out), C.byref(n)), n.value

    def free(self):
        self.L.sgpu_encoder_free(self.enc)
        self.L.sgpu_decoder_free(self.dec)
        assert self.L.sgpu_flush() == 0   # (nothing queued still reads the sources)
        self.L.sgpu_device_free(self.src)
        self.recRows.free()


def check(name, path, device):
    L = bind(D.load(path))
    case = CASES[name]
    data, want = expected(name)
    count = len(case.lengths)
    e0 = Z.engine(L)      # (every earlier case ended with a flush: nothing of theirs is still queued)
    run = Run(L, case, data)
    assert L.sgpu_flush() == 0
    e1 = Z.engine(L)

    # 1. the recovery packets are the reference's
    got, lens = run.recRows.fetch()
    for k, w in enumerate(want["recovery"]):
        r = run.recs[k]
        assert (r.DataBytes, r.FooterBytes) == (w["bytes"], w["footer_bytes"]), \
            "recovery packet %d: %d bytes with a %d-byte footer, the reference's has %d with %d" % (
                k, r.DataBytes, r.FooterBytes, w["bytes"], w["footer_bytes"])
        assert lens[k] == r.DataBytes
        assert got[k][r.DataBytes - r.FooterBytes:r.DataBytes] == bytes(r.Footer[:r.FooterBytes]), \
            "recovery packet %d: the footer in device memory is not the host's copy" % k
        assert got[k][r.DataBytes:] == bytes(run.recRows.stride - r.DataBytes)
        assert hashlib.sha256(got[k][:r.DataBytes]).hexdigest() == w["sha256"], \
            "recovery packet %d (%d bytes) differs from the reference's" % (k, r.DataBytes)

    # 2. the decode
    # (a decode solves the earliest packets that suffice for the losses they
    # cover, as the reference's does: where later losses are covered by later
    # packets only, the next call goes on; every call must succeed, and
    # together they return exactly the lost packets)
    total = calls = jobs = 0
    while total < len(case.lost):
        if device:
            r, n = run.decode(device=True)
            if r == D.PENDING:
                jobs += 1
                assert L.sgpu_flush() == 0
                r, n = run.decode(device=True)
        else:
            r, n = run.decode()
        assert r == D.SUCCESS and n > 0, "the loss set must decode: call %d returned %d with %d packets after %d " \
            "of %d" % (calls, r, n, total, len(case.lost))
        total += n
        calls += 1
    assert total == len(case.lost), "%d packets recovered, %d lost" % (total, len(case.lost))
    assert not device or jobs >= 1, "sgpu_decode_device queued no matrix job"

    # 3. every original the decoder holds, received or recovered, into guarded
    # rows: all of them, but for the received ones its window has moved past
    # (the recovery packets of a trimmed encoder start at the first original
    # it kept, and the decoder drops what lies before the packets' start)
    stride = (max(case.lengths) + 16) & ~15
    rows = D.Rows(L, count, stride)
    res, queued = D.deliver(L, run.dec, 0, count, rows)
    kept = case.kept_from()
    assert res[kept:] == [D.SUCCESS] * (count - kept), "an original of the live window is missing: %r" % (res,)
    assert all(x in (D.SUCCESS, D.NEED_MORE) for x in res[:kept])
    if not kept:
        assert queued == count
    assert L.sgpu_flush() == 0
    e2 = Z.engine(L)
    got, lens = rows.fetch()
    for k, d in enumerate(data):
        if res[k] == D.SUCCESS:
            D.check_row(got[k], lens[k], d,
                        "packet %d (%d bytes%s)" % (k, len(d), ", recovered" if k in case.lost else ""))
    rows.free()
    run.free()

    # 4. the path
    def grew(key, a, b):
        return b[key] - a[key]
    assert grew("solves", e0, e2) == calls, "%d solves for %d decodes" % (grew("solves", e0, e2), calls)
    assert grew("ldpc_bytes", e0, e2) == 0, "a row's picks went to k_ldpc"
    assert grew("ge_jobs", e0, e2) == jobs
    shape = ("batches", "versioned", "versioned_rows", "unfit", "unstaged")
    enc = {k: grew("rows_" + k, e0, e1) for k in shape}
    dec = {k: grew("rows_" + k, e1, e2) for k in shape}
    print("%s: encoder batches %r, decode batches %r, stage capacity %d" % (name, enc, dec, e2["stage_cap"]))
    assert e2["stage_cap"] == e0["stage_cap"], "the stage capacity is a constant"
    for k, v in case.enc.items():
        assert enc[k] == v, "%s: the schedule's %s grew by %d, expected %d (%r)" % (name, k, enc[k], v, enc)
    for k, v in case.dec.items():
        assert dec[k] == v, "%s: the decode's %s grew by %d, expected %d (%r)" % (name, k, dec[k], v, dec)
    assert dec["batches"] >= 1, "the decode eliminated no received data through OP_ROWS"
    # the window against the stage: the same rule on every backend that has one
    cap = e2["stage_cap"]
    if name.startswith("window_"):
        w = len(case.lengths)
        assert enc["unstaged"] == (1 if cap and w > cap else 0), \
            "a window of %d against a stage of %d: %d batches past it" % (w, cap, enc["unstaged"])
    elif not cap:
        assert enc["unstaged"] == dec["unstaged"] == 0
    return enc, dec
