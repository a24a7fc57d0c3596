#!/usr/bin/env python3
"""sgpu_frames_scan_packed against the copy it replaces and the one-frame scan.

The scan probe's row count (tools/scan_probe.py): 1024 flows x 320 rows =
327,680 rows of 1424 B in device memory, but every row holds eight frames
(seven originals of 160 B and a recovery packet of 170 B, each frame at a
16-byte boundary, as sgpu_encoder_pack_frames lays them out).  Three ways to
look at them, timed in the same process, interleaved, after a warm-up:

  (a) sgpu_frames_scan_packed (maxFrames 8) + sgpu_gather_wait: k_walk writes
      eight 32-byte records and a word per row, one DMA brings them to pinned
      memory (host wall clock around both calls; the kernel's own device time
      is sgpu_timing_kernels[8]);
  (b) what sgpu_frames_recv needs: a device-to-host copy of every row into
      pinned memory (hipMemcpyAsync of the HIP runtime the library itself
      loaded, host wall clock until the copy's event has passed);
  (c) sgpu_frames_scan_rows + sgpu_gather_wait on the same buffer: the
      one-frame scan, which sees the first frame of each row only, as the
      floor (its kernel time is sgpu_timing_kernels[7]).

The medians are reported, with every repetition.

--dense adds two legs that compare sgpu_frames_scan_packed with
sgpu_frames_scan_dense (k_walk's walk, k_rowsum, k_compact) on the same rows,
both with maxFrames = --frames, interleaved in the same process:

  all-full    the rows as above, every row full: maxRecords = rows x frames, so
              the dense form brings more bytes than the packed one (the starts
              and the info words) and shows what its two extra launches and the
              scratch round trip cost;
  mixed-fill  the same rows with length words that end row k behind its
              f_k-th frame, f_k drawn uniformly from 1..frames with a fixed
              seed (mean (frames + 1) / 2, the mean drawn is reported):
              maxRecords = the known total rounded up to a multiple of 1024.

For each: the bytes to the host, the median and range of scan plus wait, and
the device time of each kernel (sgpu_timing_kernels [8], [15], [16]).

--duplex-dense adds two legs that compare sgpu_frames_scan_duplex with
sgpu_frames_scan_duplex_dense (k_ackwalk's walk, k_rowsum2, k_compact, k_slots)
on the same rows, both with maxFrames = --frames + 1, ackSlots 1 and ackBytes
64, interleaved in the same process.  Every row is built with an 8-byte
acknowledgement frame behind its last frame, which the length words of the legs
above hide:

  all-full    every row full and its ack in every row: maxRecords = rows x
              (frames + 1) and maxAcks = rows, where the dense form cannot win;
  mixed-fill  the mixed-fill rows above, and in one row of 16 an ack written
              behind the row's last frame: maxRecords and maxAcks = the known
              totals rounded up to a multiple of 1024.

For each: the bytes to the host, the median and range of scan plus wait, and
the device time of each kernel (sgpu_timing_kernels [12], [17], [16], [18]).

    python tools/pack_probe.py [--flows 1024] [--rows 320] [--frames 8] [--reps 9] [--dense] [--duplex-dense]
                               [--out FILE]

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
    sys.exit("pack_probe: no HIP runtime in the process")


def dense_legs(L, a, dev, lens, rows, nf, stride, ends, rehearsal):
    """The all-full and the mixed-fill leg: packed against dense on the same rows."""
    med = statistics.median
    legs = {}
    rng = random.Random(11)
    fills = [rng.randrange(1, nf + 1) for _ in range(rows)]
    for leg in ("all_full", "mixed_fill"):
        if leg == "mixed_fill":
            # (every frame's header has the same width here, so the first row's frame ends hold for all rows)
            lraw = b"".join(ends[f - 1].to_bytes(4, "little") for f in fills)
            assert L.sgpu_h2d(lens, lraw, len(lraw)) == 0
            total = sum(fills)
            maxRecords = min(rows * nf, (total + 1023) & ~1023)
        else:
            total = maxRecords = rows * nf
        pBytes = L.sgpu_frames_packed_bytes(rows, nf)
        dBytes = L.sgpu_frames_dense_bytes(rows, maxRecords)
        pOut, dOut = L.sgpu_host_alloc(pBytes), L.sgpu_host_alloc(dBytes)
        assert pOut and dOut

        def timed(call):
            L.sgpu_timing(1, 1, None, None)
            t0 = time.perf_counter()
            t = call()
            assert t > 0 and L.sgpu_gather_wait(t) == 0
            wall = (time.perf_counter() - t0) * 1e3
            ms = (C.c_double * 17)()
            L.sgpu_timing_kernels(ms, 17)
            return wall, list(ms)

        pw, pk, dw, dk = [], [], [], []
        for r in range(a.warmup + a.reps):
            w1, m1 = timed(lambda: L.sgpu_frames_scan_packed(dev, stride, lens, rows, nf, pOut))
            w2, m2 = timed(lambda: L.sgpu_frames_scan_dense(dev, stride, lens, rows, nf, maxRecords, dOut))
            if r >= a.warmup:
                pw.append(w1)
                pk.append(m1[8])
                dw.append(w2)
                dk.append((m2[8], m2[15], m2[16]))
        info = (C.c_uint * 4).from_address(dOut)
        assert list(info) == [total, total, rows, 0], "dense info %r, expected T = W = %d" % (list(info), total)
        words = (C.c_uint * rows).from_address(pOut + rows * nf * 32)   # (behind the 32-byte records)
        assert sum(words) == total
        res = {"frames": total, "mean_frames_per_row": round(total / rows, 4), "max_records": maxRecords,
               "packed_bytes": pBytes, "dense_bytes": dBytes}
        if not rehearsal:
            res.update({"packed_wait_ms_median": round(med(pw), 4), "packed_wait_ms_range": [round(min(pw), 4), round(max(pw), 4)],
                        "dense_wait_ms_median": round(med(dw), 4), "dense_wait_ms_range": [round(min(dw), 4), round(max(dw), 4)],
                        "packed_k_walk_ms_median": round(med(pk), 4),
                        "dense_k_walk_ms_median": round(med([k[0] for k in dk]), 4),
                        "k_rowsum_ms_median": round(med([k[1] for k in dk]), 4),
                        "k_compact_ms_median": round(med([k[2] for k in dk]), 4),
                        "packed_wait_ms": [round(v, 4) for v in pw], "dense_wait_ms": [round(v, 4) for v in dw],
                        "dense_over_packed": round(med(dw) / med(pw), 3)})
        legs[leg] = res
        L.sgpu_host_free(pOut)
        L.sgpu_host_free(dOut)
    return legs


ACK_MSG = bytes(range(0xA0, 0xA8))   # the probe's 8-byte acknowledgement message
ACK_EVERY = 16                        # the mixed-fill leg: an ack in one row of this many


def duplex_dense_legs(L, a, dev, lens, rows, per, nf, stride, ends, rehearsal):
    """The all-full and the mixed-fill leg: the duplex scan against its dense form on the same rows."""
    med = statistics.median
    legs = {}
    m, slots, ab = nf + 1, 1, 64
    ackLen = 5 + len(ACK_MSG)
    rng = random.Random(11)
    fills = [rng.randrange(1, nf + 1) for _ in range(rows)]
    for leg in ("all_full", "mixed_fill"):
        if leg == "mixed_fill":
            # (every frame's header has the same width here, so the first row's frame ends hold for all rows)
            words = []
            for k, f in enumerate(fills):
                if k % ACK_EVERY == 0:
                    fr = bytes([ackLen - 1, 2]) + (k // per).to_bytes(3, "little") + ACK_MSG
                    assert L.sgpu_h2d(dev + k * stride + ends[f - 1], fr, len(fr)) == 0
                    words.append(ends[f - 1] + ackLen)
                else:
                    words.append(ends[f - 1])
            lraw = b"".join(w.to_bytes(4, "little") for w in words)
            acks = (rows + ACK_EVERY - 1) // ACK_EVERY
            total = sum(fills) + acks
            maxRecords = min(rows * m, (total + 1023) & ~1023)
            maxAcks = min(rows * slots, (acks + 1023) & ~1023)
        else:
            lraw = (ends[nf - 1] + ackLen).to_bytes(4, "little") * rows
            acks = rows
            total = maxRecords = rows * m
            maxAcks = rows * slots
        assert L.sgpu_h2d(lens, lraw, len(lraw)) == 0
        pBytes = L.sgpu_frames_duplex_bytes(rows, m, slots, ab)
        dBytes = L.sgpu_frames_duplex_dense_bytes(rows, maxRecords, maxAcks, ab)
        pOut, dOut = L.sgpu_host_alloc(pBytes), L.sgpu_host_alloc(dBytes)
        assert pBytes and dBytes and pOut and dOut

        def timed(call):
            L.sgpu_timing(1, 1, None, None)
            t0 = time.perf_counter()
            t = call()
            assert t > 0 and L.sgpu_gather_wait(t) == 0
            wall = (time.perf_counter() - t0) * 1e3
            ms = (C.c_double * 19)()
            L.sgpu_timing_kernels(ms, 19)
            return wall, list(ms)

        pw, pk, dw, dk = [], [], [], []
        for r in range(a.warmup + a.reps):
            w1, m1 = timed(lambda: L.sgpu_frames_scan_duplex(dev, stride, lens, rows, m, slots, ab, pOut))
            w2, m2 = timed(lambda: L.sgpu_frames_scan_duplex_dense(dev, stride, lens, rows, m, slots, ab, maxRecords,
                                                                   maxAcks, dOut))
            if r >= a.warmup:
                pw.append(w1)
                pk.append(m1[12])
                dw.append(w2)
                dk.append((m2[12], m2[17], m2[16], m2[18]))
        info = (C.c_uint * 4).from_address(dOut)
        assert list(info) == [total, total, rows, acks], "info %r, expected T = W = %d, WA = %d" % (list(info), total, acks)
        pwords = (C.c_uint * rows).from_address(pOut + rows * m * 32)   # (behind the 32-byte records)
        assert sum(pwords) == total
        # the first and the last ack's slot in both outputs
        first = C.string_at(dOut + L.sgpu_frames_duplex_dense_slots(rows, maxRecords), ab)
        last = C.string_at(dOut + L.sgpu_frames_duplex_dense_slots(rows, maxRecords) + (acks - 1) * ab, ab)
        assert first == last == ACK_MSG + bytes(ab - len(ACK_MSG))
        assert C.string_at(pOut + L.sgpu_frames_duplex_slots(rows, m), ab) == first
        res = {"frames": total, "acks": acks, "mean_frames_per_row": round(total / rows, 4), "max_frames": m,
               "ack_slots": slots, "ack_bytes": ab, "max_records": maxRecords, "max_acks": maxAcks,
               "duplex_bytes": pBytes, "dense_bytes": dBytes}
        if not rehearsal:
            res.update({"duplex_wait_ms_median": round(med(pw), 4), "duplex_wait_ms_range": [round(min(pw), 4), round(max(pw), 4)],
                        "dense_wait_ms_median": round(med(dw), 4), "dense_wait_ms_range": [round(min(dw), 4), round(max(dw), 4)],
                        "duplex_k_ackwalk_ms_median": round(med(pk), 4),
                        "dense_k_ackwalkd_ms_median": round(med([k[0] for k in dk]), 4),
                        "k_rowsum2_ms_median": round(med([k[1] for k in dk]), 4),
                        "k_compact_ms_median": round(med([k[2] for k in dk]), 4),
                        "k_slots_ms_median": round(med([k[3] for k in dk]), 4),
                        "duplex_wait_ms": [round(v, 4) for v in pw], "dense_wait_ms": [round(v, 4) for v in dw],
                        "dense_over_duplex": round(med(dw) / med(pw), 3)})
        legs[leg] = res
        L.sgpu_host_free(pOut)
        L.sgpu_host_free(dOut)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "siamese_amd", "libsiamese_amd.so"))
    ap.add_argument("--flows", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=320, help="rows per flow")
    ap.add_argument("--frames", type=int, default=8, help="frames per row: the last is a recovery packet")
    ap.add_argument("--bytes", type=int, default=160)
    ap.add_argument("--stride", type=int, default=1424)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dense", action="store_true", help="add the all-full and mixed-fill legs of the dense scan")
    ap.add_argument("--duplex-dense", action="store_true",
                    help="add the all-full and mixed-fill legs of the dense duplex scan (run last: they rewrite rows)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    rehearsal = "hostsim" in os.path.basename(a.library)

    from siamese_amd.binding import ROW_OK, PackedHead, RowHead, bind_dense_abi, bind_duplex_dense_abi
    L = bind_dense_abi(C.CDLL(a.library))
    if a.duplex_dense:
        bind_duplex_dense_abi(L)
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_device_alloc.argtypes = [C.c_size_t]
    L.sgpu_host_alloc.restype = C.c_void_p
    L.sgpu_host_alloc.argtypes = [C.c_size_t]
    L.sgpu_host_free.argtypes = [C.c_void_p]
    L.sgpu_h2d.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.sgpu_frame_write_header.restype = C.c_uint
    L.sgpu_frame_write_header.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.sgpu_timing.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sgpu_timing_kernels.argtypes = [C.c_void_p, C.c_uint]
    if L.sgpu_init(-1 if rehearsal else 0) != 0:
        sys.exit("pack_probe: the library did not initialise (no MI355X?)")

    n, per, nf, size, stride = a.flows, a.rows, a.frames, a.bytes, a.stride
    rows = n * per
    total = rows * stride
    rsize = size + 10

    def header(kind, flow, num, nbytes):
        out = (C.c_ubyte * 16)()
        return bytes(out[:L.sgpu_frame_write_header(kind, flow, num, nbytes, out)])

    # one flow's rows at a time: row r holds originals r*(nf-1) .. and a
    # recovery packet (a stand-in of the right size: the scan reads its ends,
    # not its sense), every frame at a 16-byte boundary
    rng = random.Random(7)
    data = [rng.randbytes(rsize) for _ in range(nf)]
    dev = L.sgpu_device_alloc(total)
    lens = L.sgpu_device_alloc(4 * rows)
    assert dev and lens
    ends = []   # where each frame of a row ends (the same in every row but for the header's width)
    for i in range(n):
        block, lw = [], []
        for r in range(per):
            row = bytearray()
            for j in range(nf):
                row += bytes(-len(row) % 16)
                row += (header(0, i, r * (nf - 1) + j, size) + data[j][:size]) if j < nf - 1 else \
                    (header(1, i, 0, rsize) + data[j])
                if i == 0 and r == 0:
                    ends.append(len(row))
            assert len(row) <= stride
            lw.append(len(row).to_bytes(4, "little"))
            if a.duplex_dense:   # (behind the row's length: only the duplex legs, which set their own lengths, see it)
                row += bytes([4 + len(ACK_MSG), 2]) + i.to_bytes(3, "little") + ACK_MSG
                assert len(row) <= stride
            block.append(bytes(row) + bytes(stride - len(row)))
        blob, lraw = b"".join(block), b"".join(lw)
        assert L.sgpu_h2d(dev + i * per * stride, blob, len(blob)) == 0
        assert L.sgpu_h2d(lens + 4 * i * per, lraw, len(lraw)) == 0

    outBytes = L.sgpu_frames_packed_bytes(rows, nf)
    packed = L.sgpu_host_alloc(outBytes)
    heads = L.sgpu_host_alloc(rows * C.sizeof(RowHead))
    assert packed and heads
    if not rehearsal:
        hip = hip_runtime()
        host = L.sgpu_host_alloc(total)
        assert host
        ev = C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev)) == 0

    def timed(call, index):
        L.sgpu_timing(1, 1, None, None)
        t0 = time.perf_counter()
        t = call()
        assert t > 0 and L.sgpu_gather_wait(t) == 0
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 9)()
        L.sgpu_timing_kernels(ms, 9)
        return wall, ms[index]

    def walk_ms():
        return timed(lambda: L.sgpu_frames_scan_packed(dev, stride, lens, rows, nf, packed), 8)

    def scan_ms():
        return timed(lambda: L.sgpu_frames_scan_rows(dev, stride, None, rows, heads), 7)

    def copy_ms():
        t0 = time.perf_counter()
        ok = (hip.hipMemcpyAsync(C.c_void_p(host), C.c_void_p(dev), C.c_size_t(total), HIP_D2H, None) == 0 and
              hip.hipEventRecord(ev, None) == 0 and hip.hipEventSynchronize(ev) == 0)
        wall = (time.perf_counter() - t0) * 1e3
        assert ok, "the device-to-host copy failed"
        return wall

    wk, wn, sc, kn, cp = [], [], [], [], []
    for r in range(a.warmup + a.reps):
        w, wkn = walk_ms()
        c = copy_ms() if not rehearsal else 0.0
        s, k = scan_ms()
        if r >= a.warmup:
            wk.append(w)
            wn.append(wkn)
            sc.append(s)
            kn.append(k)
            cp.append(c)
    dense = dense_legs(L, a, dev, lens, rows, nf, stride, ends, rehearsal) if a.dense else None
    duplexDense = (duplex_dense_legs(L, a, dev, lens, rows, per, nf, stride, ends, rehearsal)
                   if a.duplex_dense else None)
    L.sgpu_timing(0, 1, None, None)

    # spot check: first and last flow, first and last row, every frame
    recs = (PackedHead * (rows * nf)).from_address(packed)
    words = (C.c_uint * rows).from_address(packed + rows * nf * C.sizeof(PackedHead))
    for i in (0, n - 1):
        for r in (0, per - 1):
            k = i * per + r
            assert words[k] == nf, "row %d: word %#x" % (k, words[k])
            for j in range(nf):
                h = recs[k * nf + j]
                want = (size, 0, r * (nf - 1) + j) if j < nf - 1 else (rsize, 1, 0)
                assert (h.Status, h.Flow, h.DataBytes, h.Type, h.PacketNum) == (ROW_OK, i) + want, "row %d frame %d" % (k, j)
                assert h.Offset % 16 == 0
                if j == nf - 1:
                    assert bytes(h.Tail) == data[j][-8:] and bytes(h.Head) == data[j][:4]

    out = {"probe": "pack", "flows": n, "rows_per_flow": per, "frames_per_row": nf, "bytes": size, "stride": stride,
           "reps": a.reps, "rows": rows, "frames": rows * nf, "output_bytes": outBytes, "row_bytes": total}
    if not rehearsal:
        med = statistics.median
        out.update({"walk_wait_ms_median": round(med(wk), 4), "walk_wait_ms": [round(v, 4) for v in wk],
                    "k_walk_ms_median": round(med(wn), 4), "k_walk_ms": [round(v, 4) for v in wn],
                    "copy_rows_ms_median": round(med(cp), 4), "copy_rows_ms": [round(v, 4) for v in cp],
                    "scan_rows_wait_ms_median": round(med(sc), 4), "scan_rows_wait_ms": [round(v, 4) for v in sc],
                    "k_scan_ms_median": round(med(kn), 4), "k_scan_ms": [round(v, 4) for v in kn],
                    "copy_over_walk": round(med(cp) / med(wk), 2), "walk_over_scan_rows": round(med(wk) / med(sc), 2),
                    "k_walk_frames_per_us": round(rows * nf / (med(wn) * 1e3), 1) if med(wn) else None})
    else:
        out["rehearsal"] = "CPU test double: call sequence only, no time"
    if dense:
        out["dense"] = dense
    if duplexDense:
        out["duplex_dense"] = duplexDense
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
