"""k_ackstreamwalk against the two walks it is formed from, on identical rows,
timed with sgpu_timing_kernels in interleaved A/B runs (three rounds of warm-up,
nine measured):

    python tools/duplex_streams_probe.py [--rows 4096] [--reps 9]

Comparison 1: k_ackstreamwalk [20] against k_ackwalkd [12] on the duplex-dense
probe's mixed-fill shape (rows of 1424 bytes that hold 1 to 8 originals by a
fixed-seed rule, an 8-byte ack frame behind the last frame of one row in 16;
maxFrames 9, ackSlots 1, ackBytes 64), start 0 and no partial frame: the same
walk plus a start and one branch per row, so parity is the expectation.  Asserts
that the first sgpu_frames_duplex_dense_bytes bytes of the two outputs are equal.

Comparison 2: k_ackstreamwalk [20] against k_streamwalk [19] on ack-free rows in
streams_probe.py's two shapes (256 frames of about 100 bytes; one 1200-byte
frame).  Asserts that the records are equal.  Reported only: no call is switched
to another kernel on its strength.

Prints every sample, the medians, the ranges and the ratios."""
import argparse
import ctypes as C
import os
import random
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import duplex_streams_cases as K  # noqa: E402
import scenario_lib as S  # noqa: E402
import streams_probe as SP  # noqa: E402

TIMING_ACKWALK, TIMING_STREAMWALK, TIMING_ACKSTREAMWALK, NTIMING = 12, 19, 20, 21
WARMUP = 3


def mixed_fill_row(stride, k, rnd):
    """(row bytes, end): 1 to 8 originals of 176 bytes, an ack in one row of 16."""
    r = K.Row(stride)
    for i in range(rnd.randrange(1, 9)):
        r.add(K.original(8 * k + i, 176, flow=k & 0xff))
    if k % 16 == 0:
        r.ack(k & 0xff, b"ack")
    return r.bytes(), r.at


def timed(L, call, slot):
    L.sgpu_timing(1, 1, None, None)
    t = call()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    return ms[slot]


def ab(name, L, a, b, nameA, slotA, nameB, reps, same):
    """Interleaved A/B of two scans; b is the duplex stream scan."""
    for _ in range(WARMUP):
        timed(L, a, slotA), timed(L, b, TIMING_ACKSTREAMWALK)
    same()
    A, B = [], []
    for rep in range(reps):
        A.append(timed(L, a, slotA))
        B.append(timed(L, b, TIMING_ACKSTREAMWALK))
        print("%s rep %2d  %s %.4f ms  k_ackstreamwalk %.4f ms" % (name, rep, nameA, A[-1], B[-1]), flush=True)
    ma, mb = statistics.median(A), statistics.median(B)
    print("%s: median %s %.4f ms (min %.4f max %.4f), %s %.4f ms (min %.4f max %.4f), %s / %s = %.2f"
          % (name, nameA, ma, min(A), max(A), nameB, mb, min(B), max(B), nameA, nameB, ma / mb), flush=True)


def against_ackwalkd(L, count, reps):
    stride, m, s, abytes = 1424, 9, 1, 64
    rnd = random.Random(5)
    built = [mixed_fill_row(stride, k, rnd) for k in range(count)]
    blob = b"".join(r for r, _ in built)
    ends = struct.pack("<%dI" % count, *[e for _, e in built])
    dev, devEnds = L.sgpu_device_alloc(len(blob)), L.sgpu_device_alloc(4 * count)
    assert dev and devEnds and L.sgpu_h2d(dev, blob, len(blob)) == 0 and L.sgpu_h2d(devEnds, ends, 4 * count) == 0
    maxRecords, maxAcks = count * m, count * s
    dense = L.sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, abytes)
    nbytes = L.sgpu_frames_duplex_streams_bytes(count, maxRecords, maxAcks, abytes)
    outA, outB = L.sgpu_host_alloc(nbytes), L.sgpu_host_alloc(nbytes)

    def a():
        return L.sgpu_frames_scan_duplex_dense(dev, stride, devEnds, count, m, s, abytes, maxRecords, maxAcks, outA)

    def b():
        return L.sgpu_frames_scan_duplex_streams(dev, stride, None, devEnds, count, m, s, abytes, maxRecords, maxAcks,
                                                 outB)

    def same():
        assert C.string_at(outA, dense) == C.string_at(outB, dense), "the two scans disagree"

    ab("mixed-fill, %d rows" % count, L, a, b, "k_ackwalkd", TIMING_ACKWALK, "k_ackstreamwalk", reps, same)
    L.sgpu_host_free(outA)
    L.sgpu_host_free(outB)
    L.sgpu_device_free(dev)
    L.sgpu_device_free(devEnds)


def against_streamwalk(L, shape, count, reps):
    stride, m = ((256 * 108 + 15) & ~15, 256) if shape == "many" else (1216, 4)
    distinct = [SP.rows_of(shape, stride, 1000 * k) for k in range(16)]
    blob = b"".join(distinct[k % 16] for k in range(count))
    dev = L.sgpu_device_alloc(len(blob))
    assert dev and L.sgpu_h2d(dev, blob, len(blob)) == 0
    frames = 256 if shape == "many" else 1
    maxRecords, s, abytes = max(m, count * frames), 1, 16
    maxAcks = s
    plain = L.sgpu_frames_dense_bytes(count, maxRecords)   # (up to the end of the records the layouts agree)
    outA = L.sgpu_host_alloc(L.sgpu_frames_streams_bytes(count, maxRecords))
    outB = L.sgpu_host_alloc(L.sgpu_frames_duplex_streams_bytes(count, maxRecords, maxAcks, abytes))

    def a():
        return L.sgpu_frames_scan_streams(dev, stride, None, None, count, m, maxRecords, outA)

    def b():
        return L.sgpu_frames_scan_duplex_streams(dev, stride, None, None, count, m, s, abytes, maxRecords, maxAcks, outB)

    def same():
        assert C.string_at(outA, plain) == C.string_at(outB, plain), "the two scans' records disagree"

    ab("%s, %d rows x %d frames, stride %d" % (shape, count, frames, stride), L, a, b, "k_streamwalk",
       TIMING_STREAMWALK, "k_ackstreamwalk", reps, same)
    L.sgpu_host_free(outA)
    L.sgpu_host_free(outB)
    L.sgpu_device_free(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import siamese_amd
    siamese_amd.require_gpu()
    L = K.load(S.AMD_LIB)
    against_ackwalkd(L, args.rows, args.reps)
    for shape in ("many", "one"):
        against_streamwalk(L, shape, args.rows, args.reps)


if __name__ == "__main__":
    main()
