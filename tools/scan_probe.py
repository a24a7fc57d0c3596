#!/usr/bin/env python3
"""sgpu_frames_scan_rows against the copy it replaces.

The frame probe's shape (tools/frame_probe.py): 1024 flows x (256 originals of
1400 B + 64 recovery packets) = 327,680 frame rows of 1424 B in device memory.
Two ways to give the host what it needs to route them to decoders, timed in
the same process, interleaved, after a warm-up:

  (a) sgpu_frames_scan_rows + sgpu_gather_wait: k_scan writes a 32-byte record
      per row, one DMA brings the records to pinned memory (host wall clock
      around both calls; the kernel's own device time is
      sgpu_timing_kernels[7]);
  (b) what sgpu_frames_recv needs: a device-to-host copy of every row into
      pinned memory (hipMemcpyAsync of the HIP runtime the library itself
      loaded, host wall clock until the copy's event has passed).

The claim the numbers support is only that (a) moves 32 bytes per row to the
host instead of the stride.  The medians are reported, with every repetition.

    python tools/scan_probe.py [--flows 1024] [--packets 256] [--recovery 64] [--reps 9] [--out FILE]

Needs an MI355X: without one the library refuses to initialise and the probe
fails (no CPU fallback; --library with the CPU test double rehearses the call
sequence only and prints no time).
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIP_D2H = 2   # hipMemcpyDeviceToHost


def hip_runtime():
    """The HIP runtime already in the process (the library's own)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    sys.exit("scan_probe: no HIP runtime in the process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--flows", type=int, default=1024)
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--recovery", type=int, default=64)
    ap.add_argument("--bytes", type=int, default=1400)
    ap.add_argument("--stride", type=int, default=1424)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    from siamese_amd.binding import ROW_OK, RowHead, bind_rows_abi
    L = bind_rows_abi(C.CDLL(a.library))
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_host_alloc.restype = C.c_void_p
    L.sgpu_host_alloc.argtypes = [C.c_size_t]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("scan_probe: the library did not initialise (no MI355X?)")

    n, per, nrec, size, stride = a.flows, a.packets, a.recovery, a.bytes, a.stride
    each = per + nrec
    rows = n * each
    total = rows * stride

    def header(kind, flow, num, nbytes):
        out = (C.c_ubyte * 16)()
        return bytes(out[:L.sgpu_frame_write_header(kind, flow, num, nbytes, out)])

    # one flow's rows at a time: its originals, then its recovery packets
    # (stand-ins of the same size: the scan reads their ends, not their sense)
    rng = random.Random(7)
    data = [rng.randbytes(size) for _ in range(each)]
    rsize = stride - 16
    dev = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * rows)
    assert dev and lens
    for i in range(n):
        block, lw = [], []
        for k in range(each):
            fr = (header(0, i, k, size) + data[k]) if k < per else (header(1, i, 0, rsize) + data[k][:rsize].ljust(rsize, b"\x5a"))
            assert len(fr) <= stride
            block.append(fr + bytes(stride - len(fr)))
            lw.append(len(fr).to_bytes(4, "little"))
        blob, lraw = b"".join(block), b"".join(lw)
        assert L.sgpu_h2d(dev + i * each * stride, blob, len(blob)) == 0
        assert L.sgpu_h2d(lens + 4 * i * each, lraw, len(lraw)) == 0

    heads = L.sgpu_host_alloc(rows * C.sizeof(RowHead))
    assert heads
    if not rehearsal:
        hip = hip_runtime()
        host = L.sgpu_host_alloc(total)
        assert host
        ev = C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev)) == 0

    def scan_ms():
        L.sgpu_timing(1, 1, None, None)
        t0 = time.perf_counter()
        t = L.sgpu_frames_scan_rows(dev, stride, lens, rows, heads)
        assert t > 0 and L.sgpu_gather_wait(t) == 0
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 8)()
        L.sgpu_timing_kernels(ms, 8)
        return wall, ms[7]

    def copy_ms():
        t0 = time.perf_counter()
        ok = (hip.hipMemcpyAsync(C.c_void_p(host), C.c_void_p(dev), C.c_size_t(total), HIP_D2H, None) == 0 and
              hip.hipEventRecord(ev, None) == 0 and hip.hipEventSynchronize(ev) == 0)
        wall = (time.perf_counter() - t0) * 1e3
        assert ok, "the device-to-host copy failed"
        return wall

    sc, kn, cp = [], [], []
    for r in range(a.warmup + a.reps):
        s, k = scan_ms()
        c = copy_ms() if not rehearsal else 0.0
        if r >= a.warmup:
            sc.append(s)
            kn.append(k)
            cp.append(c)
    L.sgpu_timing(0, 1, None, None)

    # spot check: first and last flow, an original and a recovery packet each
    recs = (RowHead * rows).from_address(heads)
    for i in (0, n - 1):
        for k in (0, per - 1, per, each - 1):
            h = recs[i * each + k]
            want = (size, 0, k) if k < per else (rsize, 1, 0)
            assert (h.Status, h.Flow, h.DataBytes, h.Type, h.PacketNum) == (ROW_OK, i) + want, "row %d" % (i * each + k)
            if k >= per:
                tail = data[k][:rsize].ljust(rsize, b"\x5a")
                assert bytes(h.Tail) == tail[-8:] and bytes(h.Head) == tail[:4]

    out = {"probe": "scan", "flows": n, "packets": per, "recovery": nrec, "bytes": size, "stride": stride,
           "reps": a.reps, "rows": rows, "record_bytes": rows * C.sizeof(RowHead), "row_bytes": total}
    if not rehearsal:
        sm, km, cm = statistics.median(sc), statistics.median(kn), statistics.median(cp)
        out.update({"scan_wait_ms_median": round(sm, 4), "scan_wait_ms": [round(v, 4) for v in sc],
                    "k_scan_ms_median": round(km, 4), "k_scan_ms": [round(v, 4) for v in kn],
                    "copy_rows_ms_median": round(cm, 4), "copy_rows_ms": [round(v, 4) for v in cp],
                    "copy_over_scan": round(cm / sm, 2), "k_scan_rows_per_us": round(rows / (km * 1e3), 1) if km else None})
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
