#!/usr/bin/env python3
"""sgpu_frames_scan_duplex against what the library offered before it for rows
that carry acknowledgements: a copy of every row to the host and a parse there.

2048 rows of 1424 B in device memory (one datagram each, as a NIC would leave
them): three originals of 400 B and, last, one ack frame with a 24-byte
message, each frame at a 16-byte boundary.  Two ways to learn what is in them,
timed in the same process, interleaved, after a warm-up:

  (a) sgpu_frames_scan_duplex (maxFrames 4, one slot of 32 bytes) +
      sgpu_gather_wait: k_ackwalk writes four records, a word and a slot per
      row, one DMA brings them to pinned memory (host wall clock around both
      calls; the kernel's own device time is sgpu_timing_kernels[12]);
  (b) a device-to-host copy of every row into pinned memory (hipMemcpyAsync of
      the HIP runtime the library itself loaded, host wall clock until the
      copy's event has passed), then one sgpu_frames_parse call over the host
      copy.  sgpu_frames_parse calls an ack frame malformed and stops there, so
      the parsed copy holds a recovery frame of the same size where the ack is:
      the parser walks the same number of frames and bytes.  Copy and parse are
      reported apart and summed.

The medians are reported, with every repetition.

    python tools/duplex_probe.py [--rows 2048] [--reps 15] [--out FILE]

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


class Frame(C.Structure):
    _fields_ = [("Type", C.c_uint), ("Flow", C.c_uint), ("PacketNum", C.c_uint), ("Offset", C.c_uint),
                ("Bytes", C.c_uint)]


def hip_runtime():
    """The HIP runtime already in the process (the library's own)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    sys.exit("duplex_probe: no HIP runtime in the process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--originals", type=int, default=3, help="originals per row, before the ack")
    ap.add_argument("--bytes", type=int, default=400)
    ap.add_argument("--ack", type=int, default=24, help="ack message bytes")
    ap.add_argument("--stride", type=int, default=1424)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    from siamese_amd.binding import FRAME_ACK, ROW_OK, PackedHead, bind_duplex_abi
    L = bind_duplex_abi(C.CDLL(a.library))
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_host_alloc.restype = C.c_void_p
    L.sgpu_host_alloc.argtypes = [C.c_size_t]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_frames_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("duplex_probe: the library did not initialise (no MI355X?)")

    rows, no, size, stride = a.rows, a.originals, a.bytes, a.stride
    nf = no + 1
    slot = (a.ack + 15) & ~15
    total = rows * stride

    def header(kind, flow, num, nbytes):
        out = (C.c_ubyte * 16)()
        return bytes(out[:L.sgpu_frame_write_header(kind, flow, num, nbytes, out)])

    rng = random.Random(7)
    data = [rng.randbytes(size) for _ in range(no)]
    msgs = [rng.randbytes(a.ack) for _ in range(rows)]
    block, twin, lw = [], [], []
    for k in range(rows):
        row = bytearray()
        for j in range(no):
            row += bytes(-len(row) % 16)
            row += header(0, k % 4096, k * no + j, size) + data[j]
        row += bytes(-len(row) % 16)
        at = len(row)
        ack = (C.c_ubyte * (a.ack + 8))()
        n = L.sgpu_frame_write_ack(k % 4096, msgs[k], a.ack, ack, a.ack + 8)
        assert n == a.ack + 5
        row += bytes(ack[:n])
        assert len(row) <= stride
        lw.append(len(row).to_bytes(4, "little"))
        block.append(bytes(row) + bytes(stride - len(row)))
        # the parsed copy: a recovery frame of the same bytes in the ack's place
        t = bytearray(block[-1])
        t[at:at + 5] = header(1, k % 4096, 0, a.ack)
        twin.append(bytes(t))
    blob, lraw, tblob = b"".join(block), b"".join(lw), b"".join(twin)
    dev = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * rows)
    assert dev and lens
    assert L.sgpu_h2d(dev, blob, total) == 0 and L.sgpu_h2d(lens, lraw, len(lraw)) == 0

    outBytes = L.sgpu_frames_duplex_bytes(rows, nf, 1, slot)
    out = L.sgpu_host_alloc(outBytes)
    host = L.sgpu_host_alloc(total)
    parsed = (Frame * (rows * nf + 1))()
    assert out and host
    C.memmove(host, tblob, total)   # (the rehearsal parses this; a run copies the rows over it and puts it back)
    if not rehearsal:
        hip = hip_runtime()
        ev = C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev)) == 0

    def duplex_ms():
        L.sgpu_timing(1, 1, None, None)
        t0 = time.perf_counter()
        t = L.sgpu_frames_scan_duplex(dev, stride, lens, rows, nf, 1, slot, out)
        assert t > 0 and L.sgpu_gather_wait(t) == 0
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 13)()
        L.sgpu_timing_kernels(ms, 13)
        return wall, ms[12]

    def copy_ms():
        t0 = time.perf_counter()
        ok = (hip.hipMemcpyAsync(C.c_void_p(host), C.c_void_p(dev), C.c_size_t(total), HIP_D2H, None) == 0 and
              hip.hipEventRecord(ev, None) == 0 and hip.hipEventSynchronize(ev) == 0)
        wall = (time.perf_counter() - t0) * 1e3
        assert ok, "the device-to-host copy failed"
        return wall

    def parse_ms():
        C.memmove(host, tblob, total)   # (not timed: the copy left the ack frames there)
        n = C.c_uint(0)
        t0 = time.perf_counter()
        r = L.sgpu_frames_parse(host, total, parsed, rows * nf + 1, C.byref(n))
        wall = (time.perf_counter() - t0) * 1e3
        assert r == 0 and n.value == rows * nf, "the host parse found %d frames (%d)" % (n.value, r)
        return wall

    dx, kn, cp, ps = [], [], [], []
    for r in range(a.warmup + a.reps):
        d, k = duplex_ms()
        c = copy_ms() if not rehearsal else 0.0
        p = parse_ms()
        if r >= a.warmup:
            dx.append(d)
            kn.append(k)
            cp.append(c)
            ps.append(p)
    L.sgpu_timing(0, 1, None, None)

    # spot check: every row's word, its ack record and its slot
    recs = (PackedHead * (rows * nf)).from_address(out)
    words = (C.c_uint * rows).from_address(out + rows * nf * C.sizeof(PackedHead))
    slots = C.string_at(out + L.sgpu_frames_duplex_slots(rows, nf), rows * slot)
    for k in range(rows):
        h = recs[k * nf + no]
        assert words[k] == nf, "row %d: word %#x" % (k, words[k])
        assert (h.Status, h.Type, h.Flow, h.PacketNum, h.DataBytes) == (ROW_OK, FRAME_ACK, k % 4096, 0, a.ack), k
        assert slots[k * slot:(k + 1) * slot] == msgs[k] + bytes(slot - a.ack), "row %d: slot" % k

    res = {"probe": "duplex", "rows": rows, "stride": stride, "frames_per_row": nf, "original_bytes": size,
           "ack_bytes": a.ack, "slot_bytes": slot, "warmup": a.warmup, "reps": a.reps, "output_bytes": outBytes,
           "row_bytes": total}
    if not rehearsal:
        med = statistics.median
        both = [c + p for c, p in zip(cp, ps)]
        res.update({"duplex_wait_ms_median": round(med(dx), 4), "duplex_wait_ms": [round(v, 4) for v in dx],
                    "k_ackwalk_ms_median": round(med(kn), 4), "k_ackwalk_ms": [round(v, 4) for v in kn],
                    "copy_rows_ms_median": round(med(cp), 4), "copy_rows_ms": [round(v, 4) for v in cp],
                    "host_parse_ms_median": round(med(ps), 4), "host_parse_ms": [round(v, 4) for v in ps],
                    "copy_plus_parse_ms_median": round(med(both), 4),
                    "copy_plus_parse_over_duplex": round(med(both) / med(dx), 2)})
    else:
        res["rehearsal"] = "CPU test double: call sequence only, no time"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
