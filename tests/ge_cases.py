"""The device decode's coefficient side (k_ge, backend_hip.hip) at its
matrix-shape, pivot and singular edges: the cases shared by
test_ge_edges_cpu.py (the CPU test double, tests/hostsim) and
test_ge_edges_gpu.py (the HIP kernel on the MI355X), driven through the
siamese_gpu.h ABI with ctypes like size_cases.py and exec_shape_cases.py.

A case is a stream in block form, played by exec_shape_cases.Run: a list of
parts, each a schedule of ("add", n) and ("encode", k) steps followed by
decode calls, as many as the reference made for the same stream (it decodes
until it needs more data or everything lost so far is back).  Every case runs
twice in one process on fresh codecs: with sgpu_decode (the host's
elimination, the port every golden digest pins) and with sgpu_decode_device
(PENDING, flush, the result).  Checked, most independent first:

  1. every recovery packet (DataBytes, FooterBytes, sha256 of its bytes)
     against the reference's, recorded in tests/golden/ge_edges.json by
     tests/golden/make_ge_golden.py -- and against a live run of the
     reference where oracle/_ref is built;
  2. the result code and packet count of every decode call against the
     reference's (same file), for sgpu_decode_device after its PENDING round:
     a singular matrix is NeedMoreData at the call the reference says it at;
  3. every original, received or recovered, delivered into guarded rows byte
     for byte, and exactly the reference's set of them recovered;
  4. the device run's growth of ref_op_bytes and out_bytes equals the host
     run's: the reference's muladd bytes depend on which row became each
     pivot, on the column counts that grow in pivoted steps (cnt) and on the
     non-zero multipliers below the diagonal (nz), none of which changes the
     recovered bytes;
  5. the path by counters: ge_jobs, ge_chained, ge_retried, ge_pivoted ([37])
     and ge_singular ([38]) against the case's `dev`, and the host run's
     ge_pivoted against `host`.  The two eliminations are independent and must
     agree on whether pivoting happened; a singular device job is repeated by
     the host, which enters pivoted_ge again, so the device run counts one
     more per singular job: dev pivoted == host pivoted + dev singular.

Payloads are size_cases.payloads (SHAKE-256 of seed and index), 8 to 40 bytes;
the wide_ and pick-table cases use 8-byte packets.

What selects each branch of k_ge (backend_hip.hip; S4 = ge_stride_words(cols)
= ceil(cols / 4) | 1 dwords a row, 512 threads, four per row):

  job shape   check_recovery_possible (decoder.cpp) ends a region at the first
              recovery packet that brings the count up to the losses, so a
              first attempt's matrix is square whatever the stream offers: a
              decoder given r > c packets for c losses solves c of them: the
              NEWEST c, because list_insert puts a block's next packet in
              front of its run and the walk starts at the head.  Offering more
              packets therefore moves the matrix to other rows (r - c to r -
              1): max_255x256 (rows 1 to 255) pivots where square_255 with
              the same lost set (rows 0 to 254) does not, and rows_128 is made
              of rows 125 to 127.
              Only a resumed elimination (geResume_, after a singular attempt
              whose region survived) has more rows, and it stays on the host.
              rows > cols therefore never reaches
              k_ge through this ABI; the rowsNNN cases record that (a c x c
              chained job) and would fail if it changed.  Rows beyond 128 come
              from square jobs of more than 128 columns.
  second row  `k = pivot + 1 + (tid >> 2); k < rows; k += 128`: a second pass
  pass        at pivot p when rows - p - 1 > 128: square jobs of 130 columns
              and more (129 has exactly 128 rows below pivot 0: one pass);
              the stride-512 loops over rows * S4 dwords take a second pass
              from rows * S4 > 512, 23 x 23 (S4 = 7: 161) no, 65 x 65 (S4 =
              17: 1105) yes; those over `rows` never (rows <= 256).
  quarters    per = ceil((w1 - w0) / 4) dwords a thread, w0 = (pivot + 1) / 4,
              w1 = ceil(end / 4); byte_mask clips at pivot + 1 and at end.
              1 column: no step at all; 2: the last column's step is the
              swap-only branch or nothing; 3, 4, 5: one dword, two at 5; 16,
              17: per = 1 up to 16 columns right of the pivot, 2 from 17; 64,
              65, 68, 69: per = 4 up to 64 right of the pivot (65 columns at
              pivot 0, w1 - w0 = 17: per = 5), so the inner `w += 4` loop runs
              twice from 65 columns at pivot 0 and the 68/69 pair moves w1 by
              one more dword; 127, 128, 129 the row-pass edge; 253, 254, 255:
              S4 = 65 at 255, 16640 dwords = 66560 bytes of dynamic LDS.
              (No counter shows per or the inner loop's trips: derived.)
  refusals    submit_device_ge / submit_chained: cols > kGeMaxCols = 255 is
              refused, and the decoder's own limit (kMaxLossRecovery = 255,
              the reference's) refuses 256 losses before any matrix.
  pick table  pickLen = pickHi - pickLo over the Siamese rows (submit_device_ge):
              pickLo = the rows' elementStart (0 in block form), pickHi =
              elementStart + ldpcCount = the window, so pickLen = the window's
              originals; staged in LDS up to kGePickLds = 4096 bytes (window
              4096), read from global memory above (4097).  The pick pass of a
              row draws P = 2 * ceil(N / 16) picks, 64 a pass: P = 64 at N =
              512 (one pass), 66 at N = 520 (two).  Windows from kLdpcSplitMin
              = 512 are wide rows: the chained decode carries gated k_ldpc
              items (stats [20]).  (No counter shows pickStaged or the second
              PCG pass: derived.)
  row kinds   a window of at most kCauchyThreshold = 64 originals makes parity
              (row 0) and Cauchy rows; 65 and more Siamese rows.  GeCol.ccol
              and GeRow.rbase reach their ends with columns 0 and 63 lost.
              Rows made over an older, shorter window have jEnd < cols.
  pivoting    the first zero pivot ends the no-pivot loop; from there every
              step searches (foundL[pivot % 3]), swaps (pivB[pivot & 1]) and,
              but for the last column (`pivot >= cols - 1`: swap only), grows
              cnt[rk] to the pivot row's end.  A Siamese pivot is zero about
              once in 256, so these cases are found by tools/find_ge_cases.py;
              their counters are asserted, so a case that stops hitting its
              branch fails.
  singular    no non-zero left in a column: stop < cols, outcome word 0.  A
              chained job then ran nothing gated and the host restores the 24
              sums (chain_sums_restore), repeats the elimination and goes on
              as sgpu_decode does.
"""
import ctypes as C
import hashlib
import json
import os

import deliver_cases as D
import exec_shape_cases as X
import scenario_lib as S
import size_cases as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge_edges.json")

COUNTERS = ("jobs", "chained", "retried", "pivoted", "singular")
MAX_DECODES = 8   # per part
SHARED_WINDOW = 300


def lengths(count, seed):
    """8 to 40 bytes, neighbours differing, every value coming up."""
    return tuple(8 + (7 * i + seed) % 33 for i in range(count))


def spread(n, count, seed=0):
    """n distinct indices below count, drawn by SHAKE-256 of the seed and the
    index: another set for every seed, the same one on every machine."""
    assert n <= count
    order = sorted(range(count), key=lambda i: hashlib.shake_256(b"ge:%d:%d" % (seed, i)).digest(8))
    return tuple(sorted(order[:n]))


class Case:
    """parts: schedules, each followed by decode calls.  lost: the stream's
    lost originals.  dev: the growth the sgpu_decode_device run must show in
    ge_jobs, ge_chained, ge_retried, ge_pivoted, ge_singular (keys without the
    ge_ prefix; all five stated).  host: the sgpu_decode run's ge_pivoted."""

    def __init__(self, seed, parts, lost, dev, host=0, lens=None, short=False):
        self.parts = tuple(tuple(tuple(s) for s in part) for part in parts)
        self.schedule = tuple(s for part in self.parts for s in part)
        self.lost = tuple(lost)
        count = sum(k for op, k in self.schedule if op == "add")
        # The matrix depends on the lost set and the rows, not on the bytes,
        # and a recovery packet on the originals its encoder holds alone: the
        # cases whose stream starts with SHARED_WINDOW originals all carry the
        # same payloads and lengths, so their packets are one run of the
        # reference's (stored once in ge_edges.json), and `seed` is left to
        # draw each case's lost set.
        shared = self.schedule[0] == ("add", SHARED_WINDOW) and lens is None and not short
        self.seed = seed = SHARED_WINDOW if shared else seed
        self.lengths = tuple(lens) if lens is not None else ((8,) * count if short else lengths(count, seed))
        self.recovery = sum(k for op, k in self.schedule if op == "encode")
        self.dev, self.host = dict(dev), host
        assert len(self.lengths) == count and all(8 <= n <= 40 for n in self.lengths)
        assert all(op in ("add", "encode") for op, _ in self.schedule)
        assert len(set(self.lost)) == len(self.lost) and max(self.lost) < count
        assert sorted(self.dev) == sorted(COUNTERS)
        assert self.dev["pivoted"] == self.host + self.dev["singular"], \
            "the host repeats a singular device job: one more pivoted elimination each"

    def parts_sha256(self):
        return hashlib.sha256(json.dumps([[list(s) for s in p] for p in self.parts]).encode()).hexdigest()


def block(w, recovery):
    return [[("add", w), ("encode", recovery)]]


def dev(jobs=1, chained=1, retried=0, pivoted=0, singular=0):
    return dict(jobs=jobs, chained=chained, retried=retried, pivoted=pivoted, singular=singular)


def square(seed, n, w=300, pivoted=0, **kw):
    """n lost of a window of w, n recovery packets: one n x n chained job."""
    return Case(seed, block(w, n), spread(n, w, seed), dev(pivoted=pivoted), host=pivoted, **kw)


def mixed(seed, dev, host=0, then=(), first=60, ra=3, more=40, rb=5, la=4):
    """Two windows: ra packets over the first `first` originals, rb over all
    first + more, la > ra of the losses in the first window so that one
    region takes every packet.  The first window's symbols are at most 30
    bytes and original `first` has 40, so the rows have two lengths: the job
    is square but not chained, and the host installs the device's matrix,
    used rows and column counts (finish_device_ge).  first = 60 <=
    kCauchyThreshold: a parity row, Cauchy rows and Siamese rows in one
    matrix, the early ones with jEnd = la < cols."""
    lost = spread(la, first, seed) + tuple(first + i for i in spread(ra + rb - la, more, seed + 1))
    lens = tuple(min(n, 30) for n in lengths(first, seed)) + (40,) + lengths(more - 1, seed)
    return Case(seed, [[("add", first), ("encode", ra), ("add", more), ("encode", rb)]] + list(then), lost, dev, host,
                lens=lens)


CASES = {}

# Square Siamese matrices of a window of 300 (see `quarters` and `second row
# pass` above for what each count is an edge of), each with the first seed
# from its own count on whose matrix eliminates without pivoting
# (find_ge_cases.py square N --want plain --seeds N 4000): 1 - (255/256)^N of
# all seeds pivot, two in three at 255, so which it is belongs to the case.
SQUARE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 16: 16, 17: 17, 64: 64, 65: 65, 68: 68, 69: 69, 127: 127, 128: 128,
          129: 130, 130: 132, 253: 253, 254: 254, 255: 257}
for _n, _seed in SQUARE.items():
    CASES["square_%d" % _n] = square(_seed, _n)

CASES.update({
    # 255 lost and 256 packets offered: the region takes the newest 255, rows
    # 1 to 255 (see `job shape`): the kernel's largest matrix, chained, and
    # another one than square_255's, whose lost set it shares: this one pivots
    "max_255x256": Case(257, block(300, 256), spread(255, 300, 257), dev(pivoted=1), host=1),
    # 257 offered: rows 2 to 256, which eliminate without pivoting; kGeMaxRows
    # is never reached
    "over_255x257": Case(257, block(300, 257), spread(255, 300, 257), dev()),
    # 256 lost: past kMaxLossRecovery, the decoder (as the reference) asks for
    # more data without making a matrix on either placement
    "over_256x256": Case(256, block(300, 256), spread(256, 300, 256), dev(jobs=0, chained=0)),
    # 3 lost and 128 to 256 packets offered: 3 x 3 chained jobs of the newest
    # three rows, 125 to 127 up to 253 to 255 (`job shape`)
    "rows_128": Case(3, block(300, 128), spread(3, 300, 3), dev()),
    "rows_129": Case(3, block(300, 129), spread(3, 300, 3), dev()),
    "rows_130": Case(3, block(300, 130), spread(3, 300, 3), dev()),
    "rows_131": Case(3, block(300, 131), spread(3, 300, 3), dev()),
    "rows_256": Case(3, block(300, 256), spread(3, 300, 3), dev()),
    # window 64 = kCauchyThreshold: row 0 parity, rows 1 to 5 Cauchy; columns 0
    # and 63 lost: GeCol.ccol at both ends, rbase = row - 1 + 64 ... 68
    "cauchy_64": Case(40, block(64, 6), (0, 9, 22, 41, 50, 63), dev()),
    # seven packets offered: the region takes the newest six, rows 1 to 6, all
    # Cauchy and no parity row (the double's trace: kinds 0 6 0), rbase up to 69
    "cauchy_64_no_parity": Case(40, block(64, 7), (0, 9, 22, 41, 50, 63), dev()),
    # window 65: Siamese rows over the same ends
    "siamese_65": Case(41, block(65, 6), (0, 9, 22, 41, 63, 64), dev()),
    # parity, Cauchy and Siamese rows in one matrix, jEnd < cols, not chained
    "mixed_kinds": mixed(42, dev(chained=0)),
    # three windows (60, 100, 130 originals), rows of three lengths
    "mixed_three": Case(43, [[("add", 60), ("encode", 3), ("add", 40), ("encode", 4), ("add", 30), ("encode", 5)]],
                        spread(5, 60, 43) + tuple(60 + i for i in spread(4, 40, 44)) +
                        tuple(100 + i for i in spread(3, 30, 45)), dev(chained=0),
                        lens=tuple(min(n, 20) for n in lengths(60, 43)) + (30,) +
                        tuple(min(n, 30) for n in lengths(39, 43)) + (40,) + lengths(29, 43)),
    # pick tables: P = 64 and 66 picks a row (one PCG pass, two); pickLen 4096
    # (staged in LDS) and 4097 (read from global memory); wide rows, 8 bytes
    "wide_512": Case(50, block(512, 4), spread(4, 512, 50), dev(), short=True),
    "wide_520": Case(51, block(520, 4), spread(4, 520, 51), dev(), short=True),
    "wide_4096": Case(52, block(4096, 4), spread(4, 4096, 52), dev(), short=True),
    "wide_4097": Case(53, block(4097, 4), spread(4, 4097, 53), dev(), short=True),
    # The pivoted cases (find_ge_cases.py square N --want pivoted --at ...).
    # First zero pivot at column 0 of 8: every step is pivoted, the foundL
    # slots rotate through 0, 1, 2 twice, the last column swaps only.
    "pivot_first": square(30, 8, pivoted=1),
    # at column 34 of 100: 34 steps without pivoting, 66 with
    "pivot_middle": square(4, 100, pivoted=1),
    # not chained, first zero pivot at column 6 of 8 (find_ge_cases.py mixed 8
    # --want pivoted): the used rows and the grown column counts reach the
    # host, which eliminates the received data by them
    "pivot_unchained": mixed(13, dev(chained=0, pivoted=1), host=1),
    # (No case makes a pivoted step raise a column count, cnt[rk] = end: the
    # rows come shortest first and the pivot search takes the first non-zero,
    # so a longer row eliminates a shorter one only where the shorter ones
    # before it all hold a zero.  A walk of 278,000 two-window streams,
    # mixed(seed, first=65..264) with one and two short rows, read through the
    # trace's `grown`, found none; dropping the growth in the test double
    # fails no case.  Unproven.)
    # (a first zero pivot at the LAST column of a square matrix has no row left
    # to swap in: that is singular_last below; an eliminated one needs rows >
    # cols, which `job shape` rules out)
})


def _singular(seed, n, lost, w=300, more=(), jobs=1, **kw):
    """A chained n x n job that comes back singular: the decode asks for more
    data as the reference does, one more packet is added, and the next decode
    succeeds.  A block's next packet goes in front of the list (list_insert),
    which resets the region: the second attempt is a fresh n x n matrix of the
    newest n packets, on the host (geHost_: the singular region's retries stay
    there).  pivoted_ge is entered by the failed attempt on the host; in the
    device run also by the host's repeat of the device's attempt
    (finish_chained), whose restored sums the second attempt and everything
    after it build on."""
    return Case(seed, [[("add", w), ("encode", n)], [("encode", 1)]] + list(more), lost,
                dev(jobs=jobs, retried=1, chained=jobs, pivoted=2, singular=1), host=1, **kw)


CASES.update({
    # 1 x 1, the single coefficient zero.  No lost index of a window of 300
    # has a zero in row 0; window 304, original 0 has (find_ge_cases.py single
    # 1 --want singular --windows 296 321).
    "singular_1x1": _singular(60, 1, (0,), w=304),
    # not chained (find_ge_cases.py mixed 8 --want singular): stopped at column
    # 7 of 8; ge_retried counts chained jobs only
    "singular_unchained": mixed(68, dev(chained=0, pivoted=2, singular=1), host=1, then=[[("encode", 1)]]),
    # 24 x 24, stopped at the last column, 23 (find_ge_cases.py square 24
    # --want singular): a random matrix runs out of non-zeros at column s with
    # probability 256^-(n - s), so by chance only the last column is within
    # reach.  The stream then goes on: 100 more originals, 3 of them lost, 3
    # packets over all 400: a second loss region on the same decoder, whose
    # sums are the restored ones carried forward, and whose first attempt is a
    # device job again: ge_jobs 2.  (geHost_, set by the singular job, is
    # cleared once its region is solved; left set, the decoder would never use
    # the device again and ge_jobs would stay 1.)
    "singular_last": _singular(468, 24, spread(24, 300, 468) + (310, 355, 399), jobs=2,
                               more=[[("add", 100), ("encode", 3)]]),
})


def describe(packets, decodes, recovered, case):
    """What ge_edges.json records of a case: size_cases.describe with the
    payload of each packet as long as the longest symbol its encoder held,
    the parts' hash, every decode call's [result, packets] per part and the
    recovered packet numbers."""
    longest, added = [], 0
    for op, n in case.schedule:
        if op == "add":
            added += n
        else:
            longest += [max(Z.prefix_bytes(x) + x for x in case.lengths[:added])] * n
    return {
        "originals": len(case.lengths),
        "lengths_sha256": hashlib.sha256(json.dumps(case.lengths).encode()).hexdigest(),
        "parts_sha256": case.parts_sha256(),
        "lost": list(case.lost),
        "recovery": [{"bytes": len(p), "footer_bytes": len(p) - longest[k], "sha256": hashlib.sha256(p).hexdigest()}
                     for k, p in enumerate(packets)],
        "decodes": decodes,
        "recovered": sorted(recovered),
    }


def pack(cases):
    """ge_edges.json's form of {name: describe(...)}: every distinct packet
    record once, in a table, and each case's packets as runs [first, count]
    of it (cases over the same originals share their packets); the recovered
    packet numbers only where they are not the lost ones."""
    table, index, out = [], {}, {}
    for name, c in cases.items():
        runs = []
        for r in c["recovery"]:
            key = (r["bytes"], r["footer_bytes"], r["sha256"])
            if key not in index:
                index[key] = len(table)
                table.append(list(key))
            k = index[key]
            if runs and runs[-1][0] + runs[-1][1] == k:
                runs[-1][1] += 1
            else:
                runs.append([k, 1])
        out[name] = dict(c, recovery=runs)
        if c["recovered"] == sorted(c["lost"]):
            out[name]["recovered"] = "lost"
    return {"packets": table, "cases": out}


def unpack(packed):
    table = [{"bytes": b, "footer_bytes": f, "sha256": h} for b, f, h in packed["packets"]]
    cases = {}
    for name, c in packed["cases"].items():
        cases[name] = dict(c, recovery=[table[k] for first, n in c["recovery"] for k in range(first, first + n)])
        if c["recovered"] == "lost":
            cases[name]["recovered"] = sorted(c["lost"])
    return cases


def lost_so_far(case, part):
    added = sum(k for p in case.parts[:part + 1] for op, k in p if op == "add")
    return set(i for i in case.lost if i < added)


def reference_run(case, data):
    """The stream through the reference's siamese.h API: its recovery
    packets, its decode results per part and what it recovered."""
    lib = Z.binding().SiameseLib(S.REF_LIB).init()
    enc, dec = lib.Encoder(), lib.Decoder()
    packets, decodes, recovered, added = [], [], {}, 0
    for k, part in enumerate(case.parts):
        for op, n in part:
            if op == "add":
                for i in range(added, added + n):
                    assert enc.add(data[i]) == i
                    if i not in case.lost:
                        assert dec.add_original(i, data[i]) == 0
                added += n
            else:
                for _ in range(n):
                    p = enc.encode()
                    assert p
                    packets.append(p)
                    assert dec.add_recovery(p) == 0
        calls = []
        while len(calls) < MAX_DECODES and set(recovered) != lost_so_far(case, k):
            rc, out = dec.decode_raw()
            calls.append([rc, len(out) if out else 0])
            if rc != D.SUCCESS:
                break
            recovered.update(out)
        decodes.append(calls)
    enc.close()
    dec.close()
    return packets, decodes, recovered


_expected = {}


def expected(name):
    """The case's payloads and what the reference made of them as recorded;
    where the reference is built, a live run of it must agree first."""
    if name not in _expected:
        case = CASES[name]
        data = Z.payloads(case)
        with open(GOLDEN) as f:
            cases = unpack(json.load(f))
        assert name in cases, "%s is not in ge_edges.json: run tests/golden/make_ge_golden.py" % name
        want = cases[name]
        mine = describe([], [], [], case)
        for key in ("originals", "lengths_sha256", "parts_sha256", "lost"):
            assert want[key] == mine[key], "%s: ge_edges.json was made for other %s: run " \
                "tests/golden/make_ge_golden.py" % (name, key)
        assert len(want["recovery"]) == case.recovery and len(want["decodes"]) == len(case.parts)
        if os.path.exists(S.REF_LIB):
            packets, decodes, recovered = reference_run(case, data)
            assert all(recovered[i] == data[i] for i in recovered)
            assert describe(packets, decodes, recovered, case) == want, \
                "ge_edges.json is stale: run tests/golden/make_ge_golden.py"
        _expected[name] = (data, want)
    return _expected[name]


def run_once(L, case, data, want, device, what):
    """One placement of the case on fresh codecs: checks 1 to 3, and the
    counters' growth for 4 and 5."""
    count = len(case.lengths)
    e0 = Z.engine(L)      # (every earlier run ended with a flush: nothing of theirs is still queued)
    run = X.Run(L, case, data, schedule=())
    recovered, pending = set(), 0
    for k, part in enumerate(case.parts):
        run.play(part)
        assert L.sgpu_flush() == 0
        # 2. the decode calls the reference made, with its results
        for call, (rc, n) in enumerate(want["decodes"][k]):
            out, got = C.POINTER(D.Orig)(), C.c_uint(0)
            f = L.sgpu_decode_device if device else L.sgpu_decode
            r = f(run.dec, C.byref(out), C.byref(got))
            if device and r == D.PENDING:
                pending += 1
                assert L.sgpu_flush() == 0
                r = f(run.dec, C.byref(out), C.byref(got))
            assert (r, got.value) == (rc, n), "%s: decode %d of part %d returned %d with %d packets, the " \
                "reference's %d with %d" % (what, call, k, r, got.value, rc, n)
            if r == D.SUCCESS:
                recovered.update(out[i].PacketNum for i in range(got.value))
    assert sorted(recovered) == want["recovered"], "%s: recovered %r, the reference %r" % (
        what, sorted(recovered), want["recovered"])
    assert L.sgpu_flush() == 0

    # 1. the recovery packets are the reference's
    got, lens = run.recRows.fetch()
    for k, w in enumerate(want["recovery"]):
        r = run.recs[k]
        assert (r.DataBytes, r.FooterBytes) == (w["bytes"], w["footer_bytes"]), \
            "%s: recovery packet %d: %d bytes with a %d-byte footer, the reference's has %d with %d" % (
                what, k, r.DataBytes, r.FooterBytes, w["bytes"], w["footer_bytes"])
        assert lens[k] == r.DataBytes
        assert got[k][r.DataBytes:] == bytes(run.recRows.stride - r.DataBytes)
        assert hashlib.sha256(got[k][:r.DataBytes]).hexdigest() == w["sha256"], \
            "%s: recovery packet %d (%d bytes) differs from the reference's" % (what, k, r.DataBytes)

    # 3. every original the decoder holds into guarded rows
    rows = D.Rows(L, count, 48)
    res, queued = D.deliver(L, run.dec, 0, count, rows)
    have = [i not in case.lost or i in recovered for i in range(count)]
    assert res == [D.SUCCESS if h else D.NEED_MORE for h in have], "%s: delivery results %r" % (what, res)
    assert queued == sum(have)
    assert L.sgpu_flush() == 0
    e1 = Z.engine(L)
    got, lens = rows.fetch()
    for k, d in enumerate(data):
        if have[k]:
            D.check_row(got[k], lens[k], d, "%s: packet %d (%d bytes%s)" % (
                what, k, len(d), ", recovered" if k in case.lost else ""))
    rows.free()
    run.free()
    grew = {k: e1[k] - e0[k] for k in ("ref_op_bytes", "out_bytes", "solves", "ldpc_bytes", "ge_jobs", "ge_chained",
                                         "ge_retried", "ge_pivoted", "ge_singular")}
    assert grew["ge_jobs"] == pending, "%s: %d PENDING rounds, %d jobs" % (what, pending, grew["ge_jobs"])
    return grew


def check(name, path):
    L = X.bind(D.load(path))
    case = CASES[name]
    data, want = expected(name)
    host = run_once(L, case, data, want, False, name + " (sgpu_decode)")
    got = run_once(L, case, data, want, True, name + " (sgpu_decode_device)")
    print("%s: host %r\n%s: device %r" % (name, host, name, got))
    # 4. the accounted bytes do not depend on the placement
    # (not `solves`: a chained job's solve is queued, and counted, before its
    # outcome gates it off)
    for key in ("ref_op_bytes", "out_bytes", "ldpc_bytes"):
        assert got[key] == host[key], "%s: %s grew by %d with sgpu_decode_device, by %d with sgpu_decode" % (
            name, key, got[key], host[key])
    # 5. the path
    assert (host["ge_jobs"], host["ge_chained"], host["ge_retried"], host["ge_singular"]) == (0, 0, 0, 0)
    assert host["ge_pivoted"] == case.host, "%s: sgpu_decode entered pivoted_ge %d times, expected %d" % (
        name, host["ge_pivoted"], case.host)
    for key in COUNTERS:
        assert got["ge_" + key] == case.dev[key], "%s: ge_%s grew by %d with sgpu_decode_device, expected %d (%r)" % (
            name, key, got["ge_" + key], case.dev[key], got)
    assert got["ge_pivoted"] == host["ge_pivoted"] + got["ge_singular"], \
        "%s: the two eliminations disagree on pivoting" % name
    return host, got
