#!/usr/bin/env python3
"""k_relay's device time against k_deliver's over the same packets.

1024 decoders x 256 received originals of 1400 B (the frame probe's packet
set, tools/frame_probe.py, on the receiving side) are handed out in one
submission into rows of 1424 B, once as wire frames
(sgpu_decoder_deliver_frames, each decoder's flow its index: k_relay,
sgpu_timing_kernels[9]) and once bare (sgpu_decoder_deliver_range: k_deliver,
sgpu_timing_kernels[5]).  One build, one process: warm-up first, then --reps
repetitions of each, interleaved, the one that goes first alternating; medians
and ranges are reported.  The packets are received once, before the
repetitions: each repetition is a submission that carries nothing but its
items.

Both kernels read the same aligned source words of each symbol (88 words =
1408 B for a 1400-byte payload behind its 2-byte prefix), write the same
1424-byte row and 4-byte length; k_relay's row holds 9 header bytes more
content in place of zero fill, so the bytes moved are equal and the header's
share of a row is 9 / 1424.

    python tools/relay_probe.py [--decoders 1024] [--packets 256] [--reps 10] [--out FILE]

Needs an MI355X: without one the library refuses to initialise and the probe
fails (no CPU fallback; --library with the CPU test double rehearses the call
sequence only and prints no time).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--decoders", type=int, default=1024)
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=1400)
    ap.add_argument("--stride", type=int, default=1424)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
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
    L.sgpu_decoder_deliver_frames.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("relay_probe: the library did not initialise (no MI355X?)")

    n, per, size, stride = a.decoders, a.packets, a.bytes, a.stride
    # one set of originals feeds every decoder (each ingests its own symbols)
    pitch = (size + 15) & ~15
    src_bytes = per * pitch
    src = L.sgpu_device_alloc(src_bytes)
    blob = bytes((i * 131 + 7) % 251 for i in range(src_bytes))
    assert src and L.sgpu_h2d(src, blob, src_bytes) == 0
    decs = []
    for _ in range(n):
        d = L.sgpu_decoder_create()
        calls = C.c_uint(0)
        assert L.sgpu_decoder_add_original_range(d, 0, src, pitch, None, size, per, None, C.byref(calls)) == 0
        assert calls.value == per
        decs.append(d)
    assert L.sgpu_flush() == 0
    rows = n * per
    total = rows * stride
    dst = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * rows)
    assert dst and lens

    def kernel_ms(framed):
        L.sgpu_timing(1, 1, None, None)
        queued = C.c_uint(0)
        for i, d in enumerate(decs):
            at = i * per
            if framed:
                r = L.sgpu_decoder_deliver_frames(d, i, 0, per, dst + at * stride, stride, lens + 4 * at, None,
                                                  C.byref(queued))
            else:
                r = L.sgpu_decoder_deliver_range(d, 0, per, dst + at * stride, stride, lens + 4 * at, None,
                                                 C.byref(queued))
            assert r == 0 and queued.value == per
        assert L.sgpu_flush() == 0
        ms = (C.c_double * 10)()
        L.sgpu_timing_kernels(ms, 10)
        assert (ms[5] == 0) if framed else (ms[9] == 0)
        return ms[9] if framed else ms[5]

    def fetch(dev, nbytes):
        buf = (C.c_ubyte * nbytes)()
        srcs = (C.c_void_p * 1)(dev)
        ln = (C.c_uint * 1)(nbytes)
        assert L.sgpu_gather(1, srcs, ln, buf) == 0
        return bytes(buf)

    def header(flow, num):
        out = (C.c_ubyte * 16)()
        return bytes(out[:L.sgpu_frame_write_header(0, flow, num, size, out)])

    def spot_check(framed):
        # the first packet and the last decoder's last packet hold what was asked for
        for row, flow, num in ((0, 0, 0), (rows - 1, n - 1, per - 1)):
            want = (header(flow, num) if framed else b"") + blob[num * pitch:num * pitch + size]
            got = fetch(dst + row * stride, stride)
            assert got == want + bytes(stride - len(want)), "row %d differs (%s)" % (row, "framed" if framed else "bare")
            assert int.from_bytes(fetch(lens + 4 * row, 4), "little") == len(want)

    rl, dl = [], []
    for r in range(a.warmup + a.reps):
        # (which of the two goes first alternates, so neither always follows the other)
        if r % 2 == 0:
            f = kernel_ms(True)
            if r == 0:
                spot_check(True)
            d = kernel_ms(False)
            if r == 0:
                spot_check(False)
        else:
            d = kernel_ms(False)
            f = kernel_ms(True)
        if r >= a.warmup:
            rl.append(f)
            dl.append(d)
    L.sgpu_timing(0, 1, None, None)

    prefix = 1 if size < 0x80 else 2 if size < 0x4000 else 3
    words = (prefix + size + 15) // 16
    moved = rows * (16 * words + stride + 4)
    hf = len(header(0, 0))
    out = {"probe": "relay", "decoders": n, "packets": per, "bytes": size, "stride": stride, "reps": a.reps,
           "rows": rows, "bytes_moved": moved, "header_bytes": hf, "header_share_of_row": round(hf / stride, 4)}
    if not rehearsal:
        rm, dm = statistics.median(rl), statistics.median(dl)
        out.update({"k_relay_ms_median": round(rm, 4), "k_relay_ms_min": round(min(rl), 4),
                    "k_relay_ms_max": round(max(rl), 4), "k_relay_ms": [round(v, 4) for v in rl],
                    "k_deliver_ms_median": round(dm, 4), "k_deliver_ms_min": round(min(dl), 4),
                    "k_deliver_ms_max": round(max(dl), 4), "k_deliver_ms": [round(v, 4) for v in dl],
                    "k_relay_TBps": round(moved / (rm * 1e-3) / 1e12, 3),
                    "k_deliver_TBps": round(moved / (dm * 1e-3) / 1e12, 3),
                    "k_relay_frac_hbm_peak": round(moved / (rm * 1e-3) / HBM_PEAK, 3),
                    "k_deliver_frac_hbm_peak": round(moved / (dm * 1e-3) / HBM_PEAK, 3),
                    "k_relay_over_k_deliver_time": round(rm / dm, 4)})
    else:
        out["rehearsal"] = "CPU test double: call sequence only, no time"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
