#!/usr/bin/env python3
"""k_frame's rate on the headline shard's sender output, against a plain copy.

1024 encoders x 256 originals of 1400 B and their recovery packets (64 per
encoder) are framed in one submission into rows of 1424 B
(sgpu_encoder_deliver_range for the originals, sgpu_frames_deliver_recovery
for the recovery packets, each encoder's flow its index); the kernel's device
time is sgpu_timing_kernels[6].  The yardstick is a plain device-to-device
copy of the same number of rows x 1424 bytes in the same process
(hipMemcpyAsync of the HIP runtime the library itself loaded, timed with
device events).  Warm-up first, then --reps repetitions of each, interleaved;
the medians are reported.  The packets are encoded once, before the
repetitions: each repetition is a submission that carries nothing but the
frames.

Bytes of k_frame per repetition, from the shapes: per packet the aligned
16-byte source words holding a packet byte (an original's payload starts 2
bytes into its symbol: 88 words = 1408 B; a recovery packet starts its
buffer), the 1424-byte row and the 4-byte length, against the copy's
2 x 1424 B per row.  Rates are those bytes over the device time; HBM peak is
the 8 TB/s specification.

    python tools/frame_probe.py [--encoders 1024] [--packets 256] [--recovery 64] [--reps 9] [--out FILE]

Needs an MI355X: without one the library refuses to initialise and the probe
fails (no CPU fallback; --library with the CPU test double rehearses the call
sequence only and prints no rate).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
HIP_D2D = 3   # hipMemcpyDeviceToDevice


class Rec(C.Structure):
    _fields_ = [("DeviceData", C.c_void_p), ("DataBytes", C.c_uint), ("FooterBytes", C.c_uint),
                ("Footer", C.c_ubyte * 8), ("Head", C.c_ubyte * 4), ("Producer", C.c_void_p)]


def hip_runtime():
    """The HIP runtime already in the process (the library's own)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    sys.exit("frame_probe: no HIP runtime in the process")


def prefix_bytes(n):
    return 1 if n < 0x80 else 2 if n < 0x4000 else 3 if n < 0x200000 else 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--encoders", type=int, default=1024)
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--recovery", type=int, default=64)
    ap.add_argument("--bytes", type=int, default=1400)
    ap.add_argument("--stride", type=int, default=1424)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    L = C.CDLL(a.library)
    L.sgpu_encoder_create.restype = C.c_void_p
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_encoder_add_range.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint,
                                         C.c_void_p, C.c_void_p]
    L.sgpu_encode_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    L.sgpu_encoder_deliver_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_frames_deliver_recovery.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("frame_probe: the library did not initialise (no MI355X?)")

    n, per, nrec, size, stride = a.encoders, a.packets, a.recovery, a.bytes, a.stride
    each = per + nrec
    # one set of originals feeds every encoder (each ingests its own symbols)
    pitch = (size + 15) & ~15
    src_bytes = per * pitch
    src = L.sgpu_device_alloc(src_bytes)
    blob = bytes((i * 131 + 7) % 251 for i in range(src_bytes))
    assert src and L.sgpu_h2d(src, blob, src_bytes) == 0
    encs, recs = [], []
    for _ in range(n):
        e = L.sgpu_encoder_create()
        first, added, made = C.c_uint(0), C.c_uint(0), C.c_uint(0)
        assert L.sgpu_encoder_add_range(e, src, pitch, None, size, per, C.byref(first), C.byref(added)) == 0
        assert added.value == per and first.value == 0
        r = (Rec * nrec)()
        assert L.sgpu_encode_range(e, r, nrec, C.byref(made)) == 0 and made.value == nrec
        encs.append(e)
        recs.append(r)
    assert L.sgpu_flush() == 0
    rows = n * each
    total = rows * stride
    dst = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * rows)
    assert dst and lens

    if not rehearsal:
        hip = hip_runtime()
        ca, cb = L.sgpu_device_alloc(total), L.sgpu_device_alloc(total)
        assert ca and cb
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    flows = [(C.c_uint * nrec)(*([i] * nrec)) for i in range(n)]

    def frame_ms():
        L.sgpu_timing(1, 1, None, None)
        queued = C.c_uint(0)
        for i, e in enumerate(encs):
            at = i * each
            assert L.sgpu_encoder_deliver_range(e, 0, per, i, dst + at * stride, stride, lens + 4 * at, None,
                                                C.byref(queued)) == 0 and queued.value == per
            at += per
            assert L.sgpu_frames_deliver_recovery(nrec, recs[i], flows[i], dst + at * stride, stride, lens + 4 * at,
                                                  C.byref(queued)) == 0 and queued.value == nrec
        assert L.sgpu_flush() == 0
        ms = (C.c_double * 7)()
        L.sgpu_timing_kernels(ms, 7)
        return ms[6]

    def copy_ms():
        ms = C.c_float(0)
        ok = (hip.hipEventRecord(e0, None) == 0 and
              hip.hipMemcpyAsync(C.c_void_p(cb), C.c_void_p(ca), C.c_size_t(total), HIP_D2D, None) == 0 and
              hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0 and
              hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0)
        assert ok, "the device-to-device copy failed"
        return ms.value

    fr, cp = [], []
    for r in range(a.warmup + a.reps):
        f = frame_ms()
        c = copy_ms() if not rehearsal else 0.0
        if r >= a.warmup:
            fr.append(f)
            cp.append(c)
    L.sgpu_timing(0, 1, None, None)

    def fetch(dev, nbytes):
        buf = (C.c_ubyte * nbytes)()
        srcs = (C.c_void_p * 1)(dev)
        ln = (C.c_uint * 1)(nbytes)
        assert L.sgpu_gather(1, srcs, ln, buf) == 0
        return bytes(buf)

    def header(kind, flow, num, nbytes):
        out = (C.c_ubyte * 16)()
        return bytes(out[:L.sgpu_frame_write_header(kind, flow, num, nbytes, out)])

    # spot check: the first original, the last encoder's last original and its
    # last recovery packet hold their frames
    last = n - 1
    for row, want in ((0, header(0, 0, 0, size) + blob[:size]),
                      (last * each + per - 1, header(0, last, per - 1, size) + blob[(per - 1) * pitch:(per - 1) * pitch + size]),
                      (rows - 1, header(1, last, 0, recs[last][nrec - 1].DataBytes) +
                       fetch(recs[last][nrec - 1].DeviceData, recs[last][nrec - 1].DataBytes))):
        got = fetch(dst + row * stride, stride)
        assert got == want + bytes(stride - len(want)), "row %d differs from its frame" % row

    def words(offset, nbytes):
        return (offset + nbytes + 15) // 16 - offset // 16

    rec_words = sum(words(0, r[k].DataBytes) for r in recs for k in range(nrec))
    frame_bytes = 16 * (n * per * words(prefix_bytes(size), size) + rec_words) + rows * (stride + 4)
    copy_bytes = 2 * total
    out = {"probe": "frame", "encoders": n, "packets": per, "recovery": nrec, "bytes": size, "stride": stride,
           "reps": a.reps, "rows": rows, "frame_bytes": frame_bytes, "copy_bytes": copy_bytes}
    if not rehearsal:
        fm, cm = statistics.median(fr), statistics.median(cp)
        frate, crate = frame_bytes / (fm * 1e-3), copy_bytes / (cm * 1e-3)
        out.update({"k_frame_ms_median": round(fm, 4), "k_frame_ms": [round(v, 4) for v in fr],
                    "copy_ms_median": round(cm, 4), "copy_ms": [round(v, 4) for v in cp],
                    "k_frame_TBps": round(frate / 1e12, 3), "copy_TBps": round(crate / 1e12, 3),
                    "k_frame_frac_hbm_peak": round(frate / HBM_PEAK, 3), "copy_frac_hbm_peak": round(crate / HBM_PEAK, 3),
                    "k_frame_over_copy": round(frate / crate, 3)})
    else:
        out["rehearsal"] = "CPU test double: call sequence only, no rate"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
