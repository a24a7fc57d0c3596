#!/usr/bin/env python3
"""k_plan's and k_pack's device time against k_relay's over the same packets.

Two legs, each 1024 decoders x 256 received originals handed out in one
submission, once packed (sgpu_decoder_pack_frames: k_plan and k_pack,
sgpu_timing_kernels[10] and [11]) and once one frame per row
(sgpu_decoder_deliver_frames: k_relay, sgpu_timing_kernels[9]):

  large  1400-byte originals into rows of 1424 B, the packets and byte volume
         of tools/relay_probe.py (profiles/relay_probe.json).  A row holds one
         frame either way, so both forms write the same rows: the leg compares
         the two copies byte for byte moved and prices the plan.
  small  100-byte originals into rows of 1408 B: the packed form writes a
         thirteenth of the rows.

One build, one process: warm-up first, then --reps repetitions of each form,
interleaved, the one that goes first alternating; medians and ranges are
reported.  The packets are received once, before the repetitions: each
repetition is a submission that carries nothing but its items.  Bytes moved are
counted from the shapes: each symbol's aligned source words once, every row
written (k_relay: one per packet; k_pack: the rows the layout needs), the
length words; for k_plan the items (24 B), a 4-byte read per symbol, the
records (16 B) and the length words.

    python tools/relaypack_probe.py [--decoders 1024] [--packets 256] [--reps 10] [--out FILE]

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
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
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
    L.sgpu_decoder_deliver_frames.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_decoder_pack_frames.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_uint,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    L.sgpu_gather.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("relaypack_probe: the library did not initialise (no MI355X?)")

    def fetch(dev, nbytes):
        buf = (C.c_ubyte * nbytes)()
        srcs = (C.c_void_p * 1)(dev)
        ln = (C.c_uint * 1)(nbytes)
        assert L.sgpu_gather(1, srcs, ln, buf) == 0
        return bytes(buf)

    def leg(size, stride):
        n, per = a.decoders, a.packets
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
        out = (C.c_ubyte * 16)()
        hf = L.sgpu_frame_write_header(0, 0, 0, size, out)
        T = hf + size
        slot = (T + 15) & ~15
        fit = 1 + (stride - T) // slot            # frames of one size a row holds (the cursor rule)
        need = (per + fit - 1) // fit              # rows one decoder's range needs
        dst = L.sgpu_device_alloc(n * per * stride)   # (k_relay's rows; the packed form uses the first n * need)
        lens = L.sgpu_device_alloc(4 * n * per)
        info = L.sgpu_device_alloc(16 * n)
        assert dst and lens and info

        def kernel_ms(packed):
            L.sgpu_timing(1, 1, None, None)
            queued = C.c_uint(0)
            for i, d in enumerate(decs):
                if packed:
                    r = L.sgpu_decoder_pack_frames(d, i, 0, per, dst + i * need * stride, stride, need,
                                                   lens + 4 * i * need, info + 16 * i, None, C.byref(queued))
                else:
                    r = L.sgpu_decoder_deliver_frames(d, i, 0, per, dst + i * per * stride, stride, lens + 4 * i * per,
                                                      None, C.byref(queued))
                assert r == 0 and queued.value == per
            assert L.sgpu_flush() == 0
            ms = (C.c_double * 12)()
            L.sgpu_timing_kernels(ms, 12)
            assert (ms[9] == 0) if packed else (ms[10] == 0 and ms[11] == 0)
            return (ms[10], ms[11]) if packed else ms[9]

        def spot_check(packed):
            # the last decoder's last packet holds what was asked for, where the rule puts it
            i, k = n - 1, per - 1
            hdr = bytes(out[:L.sgpu_frame_write_header(0, i, k, size, out)])
            want = hdr + blob[k * pitch:k * pitch + size]
            if packed:
                row, off = i * need + k // fit, (k % fit) * slot
                assert [int.from_bytes(fetch(info + 16 * i + 4 * j, 4), "little") for j in range(4)] == [need, per, 0, 0]
            else:
                row, off = i * per + k, 0
            got = fetch(dst + row * stride + off, len(want))
            assert got == want, "the last frame differs (%s)" % ("packed" if packed else "one frame per row")

        pl, pk, rl = [], [], []
        for r in range(a.warmup + a.reps):
            # (which of the two goes first alternates, so neither always follows the other)
            for packed in ((True, False) if r % 2 == 0 else (False, True)):
                v = kernel_ms(packed)
                if r == 0:
                    spot_check(packed)
                if r >= a.warmup:
                    if packed:
                        pl.append(v[0])
                        pk.append(v[1])
                    else:
                        rl.append(v)
        L.sgpu_timing(0, 1, None, None)
        for d in decs:
            L.sgpu_decoder_free(d)
        assert L.sgpu_flush() == 0
        for x in (src, dst, lens, info):
            L.sgpu_device_free(x)

        prefix = 1 if size < 0x80 else 2 if size < 0x4000 else 3
        words = (prefix + size + 15) // 16
        items = n * per
        relay_rows, pack_rows = items, n * need
        relay_moved = items * 16 * words + relay_rows * (stride + 4)
        pack_moved = items * (16 * words + 16 + 24) + pack_rows * stride
        plan_moved = items * (24 + 4 + 16) + pack_rows * 4 + n * (40 + 16)
        res = {"bytes": size, "stride": stride, "frame_bytes": T, "frames_per_row": fit, "items": items,
               "k_relay_rows": relay_rows, "k_pack_rows": pack_rows,
               "k_relay_row_bytes": relay_rows * stride, "k_pack_row_bytes": pack_rows * stride,
               "row_bytes_ratio_pack_over_relay": round(pack_rows / relay_rows, 4),
               "k_relay_bytes_moved": relay_moved, "k_pack_bytes_moved": pack_moved, "k_plan_bytes_moved": plan_moved}
        if not rehearsal:
            def summary(name, v):
                return {name + "_ms_median": round(statistics.median(v), 4), name + "_ms_min": round(min(v), 4),
                        name + "_ms_max": round(max(v), 4), name + "_ms": [round(x, 4) for x in v]}
            res.update(summary("k_plan", pl))
            res.update(summary("k_pack", pk))
            res.update(summary("k_relay", rl))
            pm, km, rm = statistics.median(pl), statistics.median(pk), statistics.median(rl)
            res.update({"k_pack_TBps": round(pack_moved / (km * 1e-3) / 1e12, 3),
                        "k_relay_TBps": round(relay_moved / (rm * 1e-3) / 1e12, 3),
                        "k_pack_frac_hbm_peak": round(pack_moved / (km * 1e-3) / HBM_PEAK, 3),
                        "k_relay_frac_hbm_peak": round(relay_moved / (rm * 1e-3) / HBM_PEAK, 3),
                        "k_plan_us_per_job_step": round(pm * 1e3 / per, 4),
                        "k_pack_over_k_relay_time": round(km / rm, 4),
                        "k_plan_plus_k_pack_over_k_relay_time": round((pm + km) / rm, 4)})
        return res

    out = {"probe": "relaypack", "decoders": a.decoders, "packets": a.packets, "reps": a.reps,
           "large": leg(1400, 1424), "small": leg(100, 1408)}
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
