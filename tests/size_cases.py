"""The GF(256) arithmetic at tile-boundary packet sizes: the cases shared by
test_sizes_cpu.py (the CPU test double, tests/hostsim) and test_sizes_gpu.py
(the HIP kernels on the MI355X), driven through the siamese_gpu.h ABI with
ctypes like deliver_cases.py.

A case adds all its originals to an encoder, asks sgpu_encode_range for its
recovery packets, gives a decoder every original but the lost ones and every
recovery packet, decodes, and delivers the whole stream into guarded rows.
Checked, most independent first:

  1. every recovery packet (DataBytes, FooterBytes, sha256 of its bytes read
     from DeviceData) against the reference's packets for the same originals,
     recorded in tests/golden/size_edges.json by tests/golden/make_size_golden.py
     -- and against a live run of the reference where oracle/_ref is built;
  2. the decode returns Success with exactly the lost packets;
  3. every delivered row is the original this file generated, its length word
     right, its tail zero up to the stride, the guards intact;
  4. the engine counters show the path the case is named for.

Lengths are payload bytes.  A symbol is the payload behind a 1-3 byte length
prefix (1 byte below 128, 2 below 16384), so EDGE walks up to every tile edge
of ops.h from 4 bytes below to 1 above: 16 (a lane), 256 (kExecTileBytes,
kSolveNarrowTileBytes), 1024 (kTileBytes), 8192 (kIngestChunkBytes), 16384
(ldpc_pairs_per_item's switch, and the prefix growing to 3 bytes), 65280 (kExecRunMax tiles of 256) and 65536.
Mixed in one window, they put terms with len < op.n on both sides of each edge
(the zero-tail rule of ops.h).

Payloads are SHAKE-256 of the case's seed and the packet's index: the
committed hashes do not depend on a random generator's implementation.
"""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import deliver_cases as D
import scenario_lib as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "size_edges.json")

EDGE = [1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025,
        8187, 8188, 8189, 8190, 8191, 8192, 8193,
        16381, 16382, 16383, 16384, 16385,
        65276, 65277, 65278, 65279, 65280, 65281, 65536]
SMALL = [n for n in EDGE if n <= 8193]        # 18 values


def edge(count, a, b, table=EDGE):
    """table[(a*i + b) % len(table)], a coprime to the length: neighbours
    differ, every value comes up."""
    return tuple(table[(a * i + b) % len(table)] for i in range(count))


class Case:
    def __init__(self, seed, lengths, lost, recovery, ranges=False, align=False):
        self.seed, self.lengths, self.lost, self.recovery = seed, tuple(lengths), tuple(lost), recovery
        self.ranges, self.align = ranges, align
        assert len(set(self.lost)) == len(self.lost) <= recovery and max(self.lost) < len(self.lengths), \
            "lost packets: distinct indices of the window, no more of them than recovery packets"
        assert max(self.lengths[i] for i in self.lost) + 3 > (max(self.lengths) + 2) // 256 * 256, \
            "a lost packet must end in the last 256-byte tile of the window's longest symbol: " \
            "otherwise the solve's last tile recovers only zeros and a solve that skips it passes"


# What selects each path (ops.h unless said otherwise).  Every case loses a
# packet that ends in the longest symbol's last tile, so every tile of the
# solve has bytes to get wrong, the last one included.
CASES = {
    # window <= kCauchyThreshold (codedef.h): Cauchy rows, one OP_LINCOMBS per
    # packet; m = 6 < kSolveSplitMinRows and one solve in the launch, so
    # solve_split is false: the fused sweeps of k_solve_main on 1 KiB tiles.
    # The 1-byte and the 65536-byte packet are both lost.
    "cauchy30": Case(1, EDGE, (0, 4, 15, 16, 27, 29), 7),
    # window > kCauchyThreshold: Siamese rows (OP_ROWS over the lane sums, the
    # LDPC picks in the executor since ldpcN < kLdpcSplitMin); first and last
    # packet lost.
    "siamese96": Case(2, edge(96, 7, 3), (0, 17, 31, 68, 77, 95), 8),
    # m = kSolveSplitMinRows, square, rows of one length: sgpu_decode_device
    # chains k_ge -> gated rows -> solve in one submission; solve_split true.
    "split16": Case(3, edge(48, 11, 5), (1, 4, 7, 10, 13, 16, 19, 22, 24, 28, 31, 34, 37, 40, 43, 46), 16),
    # window exactly kCauchyThreshold; 16 <= m <= kProductMaxRows: the product
    # solve (k_solve_pre + k_solve_tr), or with SGPU_TR_SOLVE=0 the two sweeps
    # (k_solve_prefix + k_solve_main); 21 rows x 20 columns on the device.
    "product20": Case(4, edge(64, 13, 1),
                      (0, 3, 6, 9, 12, 16, 18, 21, 24, 27, 30, 33, 36, 39, 42, 45, 48, 51, 54, 63), 21),
    # m > kSolveWideMaxRows: solve_tile_bytes = 256, sweeps only (m >
    # kProductMaxRows), rows up to 65539 bytes.  13 of every 20 packets lost.
    "narrow130": Case(5, edge(200, 17, 2),
                      tuple(i for i in range(200) if i % 20 in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 14, 15, 16)), 133),
    # ldpcN >= kLdpcSplitMin: the rows' picks go to k_ldpc.  The symbols, 16354
    # to 16418 bytes, take 2- and 3-byte prefixes, but ldpc_pairs_per_item goes
    # by the ROW's bytes, and every row (encoder's and decoder's) is as long as
    # the window's longest symbol: 16418 >= 16 x 1024, so 64 pairs per item.
    # ceil(540 / 16) = 34 pairs are one item per tile: no two items meet.
    "wide540": Case(6, tuple(16384 + (i * 37) % 64 - 32 for i in range(540)), (3, 200, 539), 4),
    # The other side of that switch: the longest symbol is 16383 bytes, rows
    # below 16 x 1024 take 32 pairs per item, so the 34 pairs of each tile are
    # two items that meet by atomic XOR, on the last, partial tile too.
    "wide540low": Case(9, tuple(16350 + (i * 37) % 32 for i in range(540)), (3, 200, 539), 4),
    # The meeting on the 64-pair side: rows of 16418 bytes and ceil(1040 / 16)
    # = 65 pairs, two items per tile (64 pairs and 1).
    "wide1040": Case(10, tuple(16384 + (i * 37) % 64 - 32 for i in range(1040)), (5, 512, 1039), 4),
    # sgpu_encoder_add_range / sgpu_decoder_add_original_range with bytes[]:
    # 70 equal packets make ingest runs past kIngestRunMax (one descriptor for
    # up to 64 symbols: the block table); 8190 bytes behind their 2-byte
    # prefix end exactly on the 8 KiB chunk.  Then 60 lengths that break every
    # run.  The decoder's ingest of an original its encoder took in during the
    # same submission rides on the encoder's descriptor as a second
    # destination (dst2, dst2Mask with holes at the lost packets).
    "runs": Case(7, (8190,) * 70 + edge(60, 19, 4), (2, 40, 69, 95, 129), 6, ranges=True),
    # original i at a device address = i (mod 16): every source alignment of
    # k_ingest's two-load recombination, feeding the arithmetic.
    "align16": Case(8, edge(16, 5, 2, SMALL), (3, 8, 15), 4, align=True),
}


def payloads(case):
    return [hashlib.shake_256(b"size:%d:%d" % (case.seed, i)).digest(n) for i, n in enumerate(case.lengths)]


def prefix_bytes(n):
    return 1 if n < 128 else 2 if n < 16384 else 3


def describe(packets, case):
    """What size_edges.json records of a case's recovery packets.  Every
    packet covers the whole window, so its payload is as long as the longest
    symbol and the rest of it is the metadata footer."""
    longest = max(prefix_bytes(n) + n for n in case.lengths)
    return {
        "originals": len(case.lengths),
        "lengths_sha256": hashlib.sha256(json.dumps(case.lengths).encode()).hexdigest(),
        "lost": list(case.lost),
        "recovery": [{"bytes": len(p), "footer_bytes": len(p) - longest, "sha256": hashlib.sha256(p).hexdigest()}
                     for p in packets],
    }


_binding = None


def binding():
    """siamese_amd/binding.py by path: the package itself refuses to import
    without the HIP library."""
    global _binding
    if _binding is None:
        spec = importlib.util.spec_from_file_location("_siamese_binding",
                                                      os.path.join(S.ROOT, "siamese_amd", "binding.py"))
        _binding = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_binding)
    return _binding


def reference_run(case, data):
    """The case through the reference's siamese.h API: its recovery packets,
    and what its decoder recovers from them."""
    lib = binding().SiameseLib(S.REF_LIB).init()
    enc, dec = lib.Encoder(), lib.Decoder()
    for i, d in enumerate(data):
        assert enc.add(d) == i
    packets = [enc.encode() for _ in range(case.recovery)]
    assert all(packets)
    for i, d in enumerate(data):
        if i not in case.lost:
            assert dec.add_original(i, d) == 0
    for p in packets:
        assert dec.add_recovery(p) == 0
    recovered = dec.decode()
    enc.close()
    dec.close()
    return packets, recovered


_expected = {}


def expected(name):
    """The case's payloads and its recovery packets as recorded; where the
    reference is built, a live run of it must agree with the record first."""
    if name not in _expected:
        case = CASES[name]
        data = payloads(case)
        with open(GOLDEN) as f:
            want = json.load(f)["cases"][name]
        mine = describe([], case)
        for key in ("originals", "lengths_sha256", "lost"):
            assert want[key] == mine[key], "%s: size_edges.json was made for other %s: run " \
                "tests/golden/make_size_golden.py" % (name, key)
        assert len(want["recovery"]) == case.recovery
        if os.path.exists(S.REF_LIB):
            packets, _ = reference_run(case, data)
            assert describe(packets, case) == want, "size_edges.json is stale: run tests/golden/make_size_golden.py"
        _expected[name] = (data, want)
    return _expected[name]


def engine(L):
    v = (C.c_uint64 * len(S.ENGINE_KEYS))()
    L.sgpu_engine_stats_ex(v, len(S.ENGINE_KEYS))
    return dict(zip(S.ENGINE_KEYS, v))


def check(name, path, device):
    L = D.load(path)
    case = CASES[name]
    data, want = expected(name)
    count = len(case.lengths)
    longest = max(case.lengths)
    e0 = engine(L)      # (every earlier case ended with a flush: nothing of theirs is still queued)
    if case.align:
        pitch = (longest + 47) & ~15
        st = D.Stream(L, case.lengths, lost=case.lost, recovery=case.recovery, data=data, pitch=pitch,
                      offsets=list(range(count)))
        assert [st.at(i) & 15 for i in range(count)] == list(range(count))
    else:
        st = D.Stream(L, case.lengths, lost=case.lost, recovery=case.recovery, data=data, ranges=case.ranges)
    assert L.sgpu_flush() == 0
    e1 = engine(L)

    # 1. the recovery packets are the reference's
    for k, w in enumerate(want["recovery"]):
        r = st.recs[k]
        assert (r.DataBytes, r.FooterBytes) == (w["bytes"], w["footer_bytes"]), \
            "recovery packet %d: %d bytes with a %d-byte footer, the reference's has %d with %d" % (
                k, r.DataBytes, r.FooterBytes, w["bytes"], w["footer_bytes"])
        got = D.read(L, r.DeviceData, r.DataBytes)
        assert got[r.DataBytes - r.FooterBytes:] == bytes(r.Footer[:r.FooterBytes]), \
            "recovery packet %d: the footer in device memory is not the host's copy" % k
        assert hashlib.sha256(got).hexdigest() == w["sha256"], \
            "recovery packet %d (%d bytes) differs from the reference's" % (k, r.DataBytes)

    # 2. the decode
    if device:
        r, _ = st.decode(device=True)
        assert r == D.PENDING, "sgpu_decode_device queued no matrix job: %d" % r
        assert L.sgpu_flush() == 0
        r, n = st.decode(device=True)
    else:
        r, n = st.decode()
    assert (r, n) == (D.SUCCESS, len(case.lost)), "the loss set must decode: result %d, %d packets" % (r, n)

    # 3. every original, received or recovered, into guarded rows
    stride = (longest + 16) & ~15
    rows = D.Rows(L, count, stride)
    res, queued = D.deliver(L, st.dec, 0, count, rows)
    assert res == [D.SUCCESS] * count and queued == count
    assert L.sgpu_flush() == 0
    e2 = engine(L)
    got, lens = rows.fetch()
    assert lens == list(case.lengths)
    for k, d in enumerate(data):
        D.check_row(got[k], lens[k], d, "packet %d (%d bytes%s)" % (k, len(d), ", recovered" if k in case.lost else ""))
    rows.free()
    st.free()

    # 4. the path
    def grew(key, a=e0, b=e2):
        return b[key] - a[key]
    assert grew("solves") == 1, "one solve, not %d" % grew("solves")
    if name.startswith("wide"):
        assert grew("ldpc_bytes") > 0, "no row's picks went to k_ldpc"
    else:
        assert grew("ldpc_bytes") == 0
    if device:
        assert grew("ge_jobs") == 1
        if name == "split16":
            assert grew("ge_chained") == 1, "the square job was not chained into its decode's submission"
    else:
        assert grew("ge_jobs") == 0
    if name == "runs":
        # One descriptor per kIngestRunMax (64) packets of each stretch of equal
        # lengths: 2 for the 70 equal ones, 60 for the rest.  The decoder's
        # ingests add none, they are second destinations of the encoder's.
        # (Without runs it would be one per original, 130.)
        runs, i = 0, 0
        while i < count:
            j = i
            while j < count and case.lengths[j] == case.lengths[i]:
                j += 1
            runs += (j - i + 63) // 64
            i = j
        assert runs == 62 < count
        assert grew("ingests", e0, e1) == runs, "%d ingest descriptors for %d originals, expected %d" % (
            grew("ingests", e0, e1), count, runs)


def check_in_child(name, path, device, env):
    """check() in a fresh process with `env` added to the environment (knobs
    the library reads once per process)."""
    code = "import sys; sys.path.insert(0, %r); import size_cases; size_cases.check(%r, %r, %r); print('ok')" % (
        os.path.dirname(os.path.abspath(__file__)), name, path, device)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=120, cwd=S.ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
