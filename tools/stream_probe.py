#!/usr/bin/env python3
"""k_offsets' and k_concat's device time against k_deliver's over the same packets.

Two legs, each a set of decoders whose received originals are handed out in one
submission, once as byte streams (sgpu_decoder_deliver_stream: k_offsets and
k_concat, sgpu_timing_kernels[13] and [14]) and once as rows
(sgpu_decoder_deliver_range: k_deliver, sgpu_timing_kernels[5]):

  mtu    1400-byte originals, 1024 decoders x 256: rows of 1408 B against a
         stream whose packets start at every residue of 1400 k + 5 mod 16.
  large  64 KiB originals, 64 decoders x 64: rows of 65536 B against a stream
         at an odd address, where the body stores dominate.

Both forms move the same payload bytes; k_deliver also zeroes each row's tail
(8 B of 1408, none of 65536) and writes a length word per row where k_offsets
writes an offset word and a 16-byte record.  Every decoder's stream starts at
an odd address (base + 5 + i * packets * bytes), so no destination word of the
stream is aligned with its source.

One build, one process: warm-up first, then --reps repetitions of each form,
interleaved, the one that goes first alternating; medians and ranges are
reported.  The packets are received once, before the repetitions: each
repetition is a submission that carries nothing but its items.

    python tools/stream_probe.py [--reps 10] [--out FILE]

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
NTIMING = 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divide the decoder counts (rehearsals)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    L = C.CDLL(a.library)
    L.sgpu_decoder_create.restype = C.c_void_p
    L.sgpu_decoder_free.argtypes = [C.c_void_p]
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_device_free.argtypes = [C.c_void_p]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_decoder_add_original_range.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                                  C.c_uint, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_deliver_range.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    L.sgpu_decoder_deliver_stream.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("stream_probe: the library did not initialise (no MI355X?)")

    def fetch(dev, nbytes):
        buf = (C.c_ubyte * nbytes)()
        srcs = (C.c_void_p * 1)(dev)
        ln = (C.c_uint * 1)(nbytes)
        assert L.sgpu_gather(1, srcs, ln, buf) == 0
        return bytes(buf)

    def leg(size, n, per):
        n = max(1, n // a.scale)
        stride = (size + 15) & ~15
        pitch = stride
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
        cap = per * size                               # one decoder's stream
        rows = L.sgpu_device_alloc(n * per * stride)
        lens = L.sgpu_device_alloc(4 * n * per)
        strm = L.sgpu_device_alloc(n * cap + 16)
        offs = L.sgpu_device_alloc(4 * n * (per + 1))
        info = L.sgpu_device_alloc(16 * n)
        assert rows and lens and strm and offs and info

        def kernel_ms(stream):
            L.sgpu_timing(1, 1, None, None)
            queued = C.c_uint(0)
            for i, d in enumerate(decs):
                if stream:
                    r = L.sgpu_decoder_deliver_stream(d, 0, per, strm + 5 + i * cap, cap, offs + 4 * i * (per + 1),
                                                      info + 16 * i, None, C.byref(queued))
                else:
                    r = L.sgpu_decoder_deliver_range(d, 0, per, rows + i * per * stride, stride, lens + 4 * i * per,
                                                     None, C.byref(queued))
                assert r == 0 and queued.value == per
            assert L.sgpu_flush() == 0
            ms = (C.c_double * NTIMING)()
            L.sgpu_timing_kernels(ms, NTIMING)
            assert (ms[5] == 0) if stream else (ms[13] == 0 and ms[14] == 0)
            return (ms[13], ms[14]) if stream else ms[5]

        def spot_check(stream):
            # the last decoder's last two packets hold what was asked for, where the sums put them
            i, k = n - 1, per - 2
            want = blob[k * pitch:k * pitch + size] + blob[(k + 1) * pitch:(k + 1) * pitch + size]
            if stream:
                got = fetch(strm + 5 + i * cap + k * size, 2 * size)
                assert [int.from_bytes(fetch(info + 16 * i + 4 * j, 4), "little") for j in range(4)] == [per, cap, 0, per]
            else:
                got = fetch(rows + (i * per + k) * stride, size) + fetch(rows + (i * per + k + 1) * stride, size)
            assert got == want, "the last packets differ (%s)" % ("stream" if stream else "rows")

        ko, kc, kd = [], [], []
        for r in range(a.warmup + a.reps):
            # (which of the two goes first alternates, so neither always follows the other)
            for stream in ((True, False) if r % 2 == 0 else (False, True)):
                v = kernel_ms(stream)
                if r == 0:
                    spot_check(stream)
                if r >= a.warmup:
                    if stream:
                        ko.append(v[0])
                        kc.append(v[1])
                    else:
                        kd.append(v)
        L.sgpu_timing(0, 1, None, None)
        for d in decs:
            L.sgpu_decoder_free(d)
        assert L.sgpu_flush() == 0
        for x in (src, rows, lens, strm, offs, info):
            L.sgpu_device_free(x)

        prefix = 1 if size < 0x80 else 2 if size < 0x4000 else 3
        words = (prefix + size + 15) // 16
        items = n * per
        deliver_moved = items * (32 + 16 * words + stride + 4)
        concat_moved = items * (16 + 16 + 16 * words + size)
        offsets_moved = items * (16 + 4 + 16 + 4) + n * (40 + 4 + 16)
        res = {"bytes": size, "decoders": n, "packets": per, "items": items, "payload_bytes": items * size,
               "k_deliver_bytes_moved": deliver_moved, "k_concat_bytes_moved": concat_moved,
               "k_offsets_bytes_moved": offsets_moved}
        if not rehearsal:
            def summary(name, v):
                return {name + "_ms_median": round(statistics.median(v), 4), name + "_ms_min": round(min(v), 4),
                        name + "_ms_max": round(max(v), 4), name + "_ms": [round(x, 4) for x in v]}
            res.update(summary("k_offsets", ko))
            res.update(summary("k_concat", kc))
            res.update(summary("k_offsets_plus_k_concat", [x + y for x, y in zip(ko, kc)]))
            res.update(summary("k_deliver", kd))
            om, cm, dm = statistics.median(ko), statistics.median(kc), statistics.median(kd)
            res.update({"k_concat_TBps": round(concat_moved / (cm * 1e-3) / 1e12, 3),
                        "k_deliver_TBps": round(deliver_moved / (dm * 1e-3) / 1e12, 3),
                        "k_concat_frac_hbm_peak": round(concat_moved / (cm * 1e-3) / HBM_PEAK, 3),
                        "k_deliver_frac_hbm_peak": round(deliver_moved / (dm * 1e-3) / HBM_PEAK, 3),
                        "k_concat_over_k_deliver_time": round(cm / dm, 4),
                        "k_offsets_plus_k_concat_over_k_deliver_time": round((om + cm) / dm, 4)})
        return res

    out = {"probe": "stream", "reps": a.reps, "mtu": leg(1400, 1024, 256), "large": leg(65536, 64, 64)}
    if rehearsal:
        out["rehearsal"] = "CPU test double: call sequence only, no time"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
