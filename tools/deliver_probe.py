#!/usr/bin/env python3
"""k_deliver's rate on the headline shard's output, against a plain copy.

1024 decoders x 256 received packets of 1400 B are delivered in one
submission into rows of 1408 B (sgpu_decoder_deliver_range); the kernel's
device time is sgpu_timing_kernels[5].  The yardstick is a plain
device-to-device copy of the same 1024 x 256 x 1408 bytes in the same process
(hipMemcpyAsync of the HIP runtime the library itself loaded, timed with
device events).  Warm-up first, then --reps repetitions of
each, interleaved; the medians are reported.

Bytes of k_deliver per repetition, from the shapes: per packet one 16-byte
word per lane with a payload byte (the aligned source words holding the 1402-
byte symbol: 88 words = 1408 B), the 1408-byte row and the 4-byte length:
2820 B, against the copy's 2 x 1408 B.  Rates are those bytes over the device
time; HBM peak is the 8 TB/s specification.

    python tools/deliver_probe.py [--decoders 1024] [--packets 256] [--reps 9] [--out FILE]

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


def hip_runtime():
    """The HIP runtime already in the process (the library's own)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    sys.exit("deliver_probe: no HIP runtime in the process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--decoders", type=int, default=1024)
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=1400)
    ap.add_argument("--stride", type=int, default=1408)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    L = C.CDLL(a.library)
    L.sgpu_decoder_create.restype = C.c_void_p
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_decoder_add_original_range.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                                  C.c_uint, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_deliver_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("deliver_probe: the library did not initialise (no MI355X?)")

    n, per, size, stride = a.decoders, a.packets, a.bytes, a.stride
    # one set of originals feeds every decoder (each ingests its own symbols)
    src_bytes = per * stride
    src = L.sgpu_device_alloc(src_bytes)
    blob = bytes((i * 131 + 7) % 251 for i in range(src_bytes))
    assert src and L.sgpu_h2d(src, blob, src_bytes) == 0
    decs = []
    for _ in range(n):
        d = L.sgpu_decoder_create()
        calls = C.c_uint(0)
        assert L.sgpu_decoder_add_original_range(d, 0, src, stride, None, size, per, None, C.byref(calls)) == 0
        assert calls.value == per
        decs.append(d)
    assert L.sgpu_flush() == 0
    total = n * per * stride
    dst = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * n * per)
    assert dst and lens

    if not rehearsal:
        hip = hip_runtime()
        ca, cb = L.sgpu_device_alloc(total), L.sgpu_device_alloc(total)
        assert ca and cb
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def deliver_ms():
        L.sgpu_timing(1, 1, None, None)
        queued = C.c_uint(0)
        for i, d in enumerate(decs):
            assert L.sgpu_decoder_deliver_range(d, 0, per, dst + i * per * stride, stride, lens + 4 * i * per, None,
                                                C.byref(queued)) == 0 and queued.value == per
        assert L.sgpu_flush() == 0
        ms = (C.c_double * 6)()
        L.sgpu_timing_kernels(ms, 6)
        return ms[5]

    def copy_ms():
        ms = C.c_float(0)
        ok = (hip.hipEventRecord(e0, None) == 0 and
              hip.hipMemcpyAsync(C.c_void_p(cb), C.c_void_p(ca), C.c_size_t(total), HIP_D2D, None) == 0 and
              hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0 and
              hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0)
        assert ok, "the device-to-device copy failed"
        return ms.value

    dl, cp = [], []
    for r in range(a.warmup + a.reps):
        d = deliver_ms()
        c = copy_ms() if not rehearsal else 0.0
        if r >= a.warmup:
            dl.append(d)
            cp.append(c)
    L.sgpu_timing(0, 1, None, None)

    # spot check: the first and the last row hold their packet
    for row, k in ((0, 0), (n * per - 1, per - 1)):
        buf = (C.c_ubyte * stride)()
        srcs = (C.c_void_p * 1)(dst + row * stride)
        ln = (C.c_uint * 1)(stride)
        assert L.sgpu_gather(1, srcs, ln, buf) == 0
        want = blob[k * stride:k * stride + size] + bytes(stride - size)
        assert bytes(buf) == want, "row %d differs from its packet" % row

    words = (size + (1 if size <= 0x7f else 2 if size <= 0x3fff else 3) + 15) // 16
    deliver_bytes = n * per * (16 * words + stride + 4)
    copy_bytes = 2 * total
    out = {"probe": "deliver", "decoders": n, "packets": per, "bytes": size, "stride": stride,
           "reps": a.reps, "deliver_bytes": deliver_bytes, "copy_bytes": copy_bytes}
    if not rehearsal:
        dm, cm = statistics.median(dl), statistics.median(cp)
        dr, cr = deliver_bytes / (dm * 1e-3), copy_bytes / (cm * 1e-3)
        out.update({"k_deliver_ms_median": round(dm, 4), "k_deliver_ms": [round(v, 4) for v in dl],
                    "copy_ms_median": round(cm, 4), "copy_ms": [round(v, 4) for v in cp],
                    "k_deliver_TBps": round(dr / 1e12, 3), "copy_TBps": round(cr / 1e12, 3),
                    "k_deliver_frac_hbm_peak": round(dr / HBM_PEAK, 3), "copy_frac_hbm_peak": round(cr / HBM_PEAK, 3),
                    "k_deliver_over_copy": round(dr / cr, 3)})
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
