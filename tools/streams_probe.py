"""k_streamwalk against k_walkd on identical rows (start 0, no partial frame, so
both walks do the same work and write the same dense output), timed with
sgpu_timing_kernels in interleaved A/B runs:

    python tools/streams_probe.py [--rows 4096] [--reps 15]

Two shapes: rows of 256 frames of about 100 bytes (the latency-bound case the
wave-per-row walk exists for) and rows of one 1200-byte frame (where the
lane-per-row walk should win or tie).  Prints every sample, the medians and the
ratio k_walkd / k_streamwalk per shape."""
import argparse
import ctypes as C
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scenario_lib as S  # noqa: E402
import streams_cases as K  # noqa: E402

TIMING_WALK, TIMING_STREAMWALK, NTIMING = 8, 19, 20


def rows_of(shape, stride, seed):
    rnd = random.Random(seed)
    r = K.Row(stride)
    if shape == "many":
        for i in range(256):
            size = rnd.randrange(92, 108)
            r.add(K.recovery(seed + i, size) if i % 4 == 3 else K.original(seed + i, size))
    else:
        r.add(K.original(seed, 1200))
    return r.bytes()


def timed(L, call, slot):
    L.sgpu_timing(1, 1, None, None)
    t = call()
    assert t > 0 and L.sgpu_gather_wait(t) == 0
    ms = (C.c_double * NTIMING)()
    L.sgpu_timing_kernels(ms, NTIMING)
    L.sgpu_timing(0, 1, None, None)
    return ms[slot]


def probe(L, shape, count, reps):
    stride, m = (256 * 108 + 15) & ~15 if shape == "many" else 1216, 256 if shape == "many" else 4
    distinct = [rows_of(shape, stride, 1000 * k) for k in range(16)]
    blob = b"".join(distinct[k % 16] for k in range(count))
    dev = L.sgpu_device_alloc(len(blob))
    assert dev and L.sgpu_h2d(dev, blob, len(blob)) == 0
    frames = 256 if shape == "many" else 1
    maxRecords = max(m, count * frames)
    nbytes = L.sgpu_frames_streams_bytes(count, maxRecords)
    dense = L.sgpu_frames_dense_bytes(count, maxRecords)
    outA, outB = L.sgpu_host_alloc(nbytes), L.sgpu_host_alloc(nbytes)

    def a():
        return L.sgpu_frames_scan_dense(dev, stride, None, count, m, maxRecords, outA)

    def b():
        return L.sgpu_frames_scan_streams(dev, stride, None, None, count, m, maxRecords, outB)

    for _ in range(2):
        timed(L, a, TIMING_WALK), timed(L, b, TIMING_STREAMWALK)
    assert C.string_at(outA, dense) == C.string_at(outB, dense), "the two scans disagree"
    A, B = [], []
    for rep in range(reps):
        A.append(timed(L, a, TIMING_WALK))
        B.append(timed(L, b, TIMING_STREAMWALK))
        print("%s rep %2d  k_walkd %.4f ms  k_streamwalk %.4f ms" % (shape, rep, A[-1], B[-1]), flush=True)
    ma, mb = statistics.median(A), statistics.median(B)
    print("%s: %d rows x %d frames, stride %d: median k_walkd %.4f ms (min %.4f max %.4f), k_streamwalk %.4f ms "
          "(min %.4f max %.4f), k_walkd / k_streamwalk = %.2f" % (shape, count, frames, stride, ma, min(A), max(A), mb,
                                                                   min(B), max(B), ma / mb), flush=True)
    L.sgpu_host_free(outA)
    L.sgpu_host_free(outB)
    L.sgpu_device_free(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    import siamese_amd
    siamese_amd.require_gpu()
    L = K.load(S.AMD_LIB)
    for shape in ("many", "one"):
        probe(L, shape, args.rows, args.reps)


if __name__ == "__main__":
    main()
