"""Workloads around the uniform subwindows of both codecs (test_uniform_slots_cpu.py,
test_uniform_slots_gpu.py): a subwindow filled by range adds of one length
keeps one descriptor instead of 64 slot records (encoder.h EncUniform,
decoder.h DecUniform).

Harness configs, with reference digests under tests/golden/<name>.json written
by tests/golden/make_uniform_golden.py from oracle/_ref/libsiamese_ref.so, and
scripted call sequences on the batch ABI that run the same originals through
range calls and through single calls of one library.  The scripted sequences
are NOT compared with the reference library: they have no fixture; the single
calls they are compared with are the per-element path, which this change
leaves as it was and which the harness fixtures compare with the reference.

The slot counters are printed when the process exits, so the CPU test runs
each case in a process of its own:  python uniform_cases.py LIBRARY CASE
"""
import ctypes as C
import json
import os
import sys

import scenario_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Block mode, 100 B, 30 % loss.  56: the growth rule's first spare subwindow
# (element + 8 >= 64); 57, 63, 64, 65: around a subwindow's edge and the
# Cauchy/Siamese threshold; 128 and 130: whole subwindows, the ingest-run cap
# (64) met twice, and a tail of two.
BLOCK_SIZES = (56, 57, 63, 64, 65, 128, 130)
CONFIGS = {}
for _n in BLOCK_SIZES:
    for _r in (0, 1):
        CONFIGS["uni_block%d%s" % (_n, "r" if _r else "")] = S.make_config(
            block_mode=1, streams=4, originals=_n, payload_bytes=100, loss_pct=30, recovery_loss_pct=30,
            add_ranges=_r)
# the GPU run: 8 streams x 130 x 100 B, 20 % loss, every byte hashed
CONFIGS["uni_block130x8r"] = S.make_config(block_mode=1, streams=8, originals=130, payload_bytes=100, loss_pct=20,
                                           recovery_loss_pct=20, add_ranges=1)
# streaming with immediate acknowledgements, range adds between them, long
# enough for remove_elements to rotate subwindows several times
CONFIGS["uni_ack"] = S.make_config(streams=4, originals=600, payload_bytes=100, loss_pct=10, recovery_loss_pct=10,
                                   recovery_interval=8, ack_policy=1, add_ranges=1)

SUCCESS, INVALID, NEED_MORE, MAX_PACKETS, DUPLICATE = 0, 1, 2, 3, 4


class Rec(C.Structure):
    _fields_ = [("DeviceData", C.c_void_p), ("DataBytes", C.c_uint), ("FooterBytes", C.c_uint),
                ("Footer", C.c_ubyte * 8), ("Head", C.c_ubyte * 4), ("Producer", C.c_void_p)]


class Orig(C.Structure):
    _fields_ = [("PacketNum", C.c_uint), ("DataBytes", C.c_uint), ("Data", C.c_void_p)]


def open_lib(path):
    L = C.CDLL(path)
    L.sgpu_encoder_create.restype = C.c_void_p
    L.sgpu_device_alloc.restype = C.c_void_p
    L.sgpu_encoder_free.argtypes = [C.c_void_p]
    L.sgpu_decoder_create.restype = C.c_void_p
    L.sgpu_encoder_add_range.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint), C.c_uint, C.c_uint,
                                         C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    assert L.sgpu_init(-1) == 0
    return L


STRIDE = 2048


def stage(L, count, stride=STRIDE):
    dev = L.sgpu_device_alloc(C.c_size_t(stride * count))
    host = bytes((i * 131 + 7) % 251 for i in range(stride * count))
    assert L.sgpu_h2d(C.c_void_p(dev), host, C.c_size_t(len(host))) == 0
    return dev


def add_single(L, enc, dev, first, sizes, stride=STRIDE):
    """sgpu_encoder_add per original until one fails: (result, added, first packet number)."""
    firstNum = None
    for i, b in enumerate(sizes):
        num = C.c_uint(0)
        r = L.sgpu_encoder_add(C.c_void_p(enc), C.c_void_p(dev + stride * (first + i)), C.c_uint(b), C.byref(num))
        if r != SUCCESS:
            return r, i, firstNum
        if firstNum is None:
            firstNum = num.value
    return SUCCESS, len(sizes), firstNum


def add_range(L, enc, dev, first, sizes, stride=STRIDE, fixed=False):
    n = len(sizes)
    firstNum, added = C.c_uint(0), C.c_uint(0)
    lens = None if fixed else (C.c_uint * max(1, n))(*sizes)
    r = L.sgpu_encoder_add_range(enc, C.c_void_p(dev + stride * first), stride, lens, sizes[0] if fixed else 0, n,
                                 C.byref(firstNum), C.byref(added))
    return r, added.value, (firstNum.value if added.value else None)


def encode_bytes(L, enc, count):
    """`count` recovery packets of `enc`, each read back after its own flush."""
    out = []
    for _ in range(count):
        r = Rec()
        res = L.sgpu_encode(C.c_void_p(enc), C.byref(r))
        if res != SUCCESS:
            out.append((res,))
            continue
        assert L.sgpu_flush() == 0
        buf = (C.c_ubyte * max(1, r.DataBytes))()
        srcs = (C.c_void_p * 1)(r.DeviceData)
        lens = (C.c_uint * 1)(r.DataBytes)
        assert L.sgpu_gather(1, srcs, lens, buf) == 0
        out.append((res, bytes(buf[:r.DataBytes]), bytes(r.Footer[:r.FooterBytes]), bytes(r.Head)))
    return out


def _pair(L, script, originals, rows=6):
    """Run `script(add)` on two encoders, `add` being add_range for one and
    add_single for the other; everything either returns, and the recovery
    packets made afterwards, must agree."""
    dev = stage(L, originals)
    seen = []
    for add in (add_range, add_single):
        enc = L.sgpu_encoder_create()
        log = script(L, enc, dev, add)
        log.append(encode_bytes(L, enc, rows))
        L.sgpu_encoder_free(enc)
        assert L.sgpu_flush() == 0
        seen.append(log)
    assert seen[0] == seen[1], "range calls and single calls disagree"


def case_single_then_range(L):
    """One sgpu_encoder_add, then a range: the first subwindow has a record
    already and stays per-element, the second is entered at its first slot."""
    def script(L, enc, dev, add):
        log = [add_single(L, enc, dev, 0, [100])]
        log.append(add(L, enc, dev, 1, [100] * 129))
        return log
    _pair(L, script, 130)


def case_mixed_length(L):
    """lens[] with one other length in the middle of a subwindow: the
    subwindow is entered by the first 20 and demoted by the 21st."""
    def script(L, enc, dev, add):
        return [add(L, enc, dev, 0, [100] * 20 + [90] + [100] * 19)]
    _pair(L, script, 40)


def case_stride(L):
    """The first call fixes the slab's stride (1408: 100 B symbols); the next
    call's symbols of 1500 B do not fit its slots."""
    def script(L, enc, dev, add):
        return [add(L, enc, dev, 0, [100] * 10), add(L, enc, dev, 10, [1500] * 10)]
    _pair(L, script, 20)


def case_bad_length(L):
    """A zero length at position 70 of a range: InvalidInput, 70 added."""
    def script(L, enc, dev, add):
        log = [add(L, enc, dev, 0, [100] * 70 + [0] + [100] * 9)]
        assert log[0][0] == INVALID and log[0][1] == 70
        return log
    _pair(L, script, 80)


def case_max_packets(L):
    """1-byte payloads until the window is full (16000): MaxPacketsReached
    with the same count either way."""
    dev = stage(L, 16100, stride=16)
    seen = []
    for add in (add_range, add_single):
        enc = L.sgpu_encoder_create()
        log = [add(L, enc, dev, 0, [1] * 15990, stride=16), add(L, enc, dev, 15990, [1] * 100, stride=16)]
        assert log[1][0] == MAX_PACKETS and log[1][1] == 10
        log.append(add(L, enc, dev, 0, [1] * 5, stride=16))
        log.append(encode_bytes(L, enc, 1))
        L.sgpu_encoder_free(enc)
        assert L.sgpu_flush() == 0
        seen.append(log)
    assert seen[0] == seen[1]


def case_fixed_block(L):
    """fixedBytes, no lens[]: 130 originals of 100 B in one call."""
    def script(L, enc, dev, add):
        if add is add_range:
            return [add(L, enc, dev, 0, [100] * 130, fixed=True)]
        return [add(L, enc, dev, 0, [100] * 130)]
    _pair(L, script, 130, rows=40)


def case_retransmit(L):
    """A retransmission after a range add stamps one element: its subwindow
    demotes, the packet returned is the one single adds give.  (One wait for
    both encoders, past the initial 500 ms timeout as tests/arq_cases.py.)"""
    import time
    dev = stage(L, 130)
    encs = [L.sgpu_encoder_create(), L.sgpu_encoder_create()]
    logs = [[add(L, enc, dev, 0, [100] * 130)] for enc, add in zip(encs, (add_range, add_single))]
    time.sleep(0.65)
    for enc, log in zip(encs, logs):
        o = Orig()
        r = L.sgpu_encoder_retransmit(C.c_void_p(enc), C.byref(o))
        log.append((r, o.PacketNum, o.DataBytes))
        assert r == SUCCESS and o.DataBytes == 100
        log.append(encode_bytes(L, enc, 4))
        L.sgpu_encoder_free(enc)
        assert L.sgpu_flush() == 0
    assert logs[0] == logs[1]


def case_restart_window(L):
    """Everything acknowledged (remove_before past the last packet), then a
    new range: start_window releases uniform subwindows and they are entered
    again."""
    def script(L, enc, dev, add):
        log = [add(L, enc, dev, 0, [100] * 130)]
        log.append(encode_bytes(L, enc, 2))
        assert L.sgpu_encoder_remove_before(C.c_void_p(enc), 130) == 0
        log.append(add(L, enc, dev, 0, [100] * 70))
        return log
    _pair(L, script, 130)


def dec_add_single(L, dec, dev, first, sizes):
    """sgpu_decoder_add_original per packet, as the range call defines itself:
    a DuplicateData goes on, any other failure stops.  (result, calls, results)."""
    results = []
    for i, b in enumerate(sizes):
        r = L.sgpu_decoder_add_original(C.c_void_p(dec), C.c_uint(first + i), C.c_void_p(dev + STRIDE * (first + i)),
                                        C.c_uint(b))
        results.append(r)
        if r not in (SUCCESS, DUPLICATE):
            return r, len(results), results
    return SUCCESS, len(results), results


def dec_add_range(L, dec, dev, first, sizes):
    n = len(sizes)
    res = (C.c_int * n)(*([-1] * n))
    calls = C.c_uint(0)
    lens = (C.c_uint * n)(*sizes)
    r = L.sgpu_decoder_add_original_range(C.c_void_p(dec), C.c_uint(first), C.c_void_p(dev + STRIDE * first),
                                          C.c_size_t(STRIDE), lens, 0, n, res, C.byref(calls))
    return r, calls.value, list(res[:calls.value])


def decode_bytes(L, dec):
    """sgpu_decode and, after the flush, every recovered packet's number, length and bytes."""
    out = C.POINTER(Orig)()
    count = C.c_uint(0)
    r = L.sgpu_decode(C.c_void_p(dec), C.byref(out), C.byref(count))
    assert L.sgpu_flush() == 0
    got = []
    for i in range(count.value if r == SUCCESS else 0):
        o = out[i]
        buf = (C.c_ubyte * max(1, o.DataBytes))()
        srcs = (C.c_void_p * 1)(o.Data)
        lens = (C.c_uint * 1)(o.DataBytes)
        assert L.sgpu_gather(1, srcs, lens, buf) == 0
        got.append((o.PacketNum, o.DataBytes, bytes(buf[:o.DataBytes])))
    return r, got


def _decoder_pair(L, lost, before, after):
    """A sender of 70 originals of 100 B; two receivers take what `before`
    feeds them (one by range calls, one by single calls), the recovery packets,
    a decode, then what `after` feeds them.  Every call's result, the per-packet
    results, the calls made and the recovered bytes must agree."""
    dev = stage(L, 80)
    enc = L.sgpu_encoder_create()
    assert add_range(L, enc, dev, 0, [100] * 70)[:2] == (SUCCESS, 70)
    decs = [C.c_void_p(L.sgpu_decoder_create()).value for _ in range(2)]
    adds = (dec_add_range, dec_add_single)
    logs = [[before(L, d, dev, a)] for d, a in zip(decs, adds)]
    for _ in range(len(lost) + 1):
        r = Rec()
        assert L.sgpu_encode(C.c_void_p(enc), C.byref(r)) == SUCCESS
        for d in decs:
            assert L.sgpu_decoder_add_recovery(C.c_void_p(d), C.byref(r)) == SUCCESS
        assert L.sgpu_flush() == 0
    for d, a, log in zip(decs, adds, logs):
        res, got = decode_bytes(L, d)
        assert res == SUCCESS and sorted(g[0] for g in got) == sorted(lost)
        assert all(g[1] == 100 for g in got)
        log.append(got)
        log.append(after(L, d, dev, a))
        L.sgpu_decoder_free(C.c_void_p(d))
    L.sgpu_encoder_free(enc)
    assert L.sgpu_flush() == 0
    assert logs[0] == logs[1], "range calls and single calls disagree"
    return logs[0]


def case_dec_duplicate(L):
    """Decoder: ranges fill 0..9 and 11..39 (one uniform subwindow with a
    hole), packet 10 arrives alone (a single add demotes the subwindow), then a
    range over 0..39 holds everything again (DuplicateData for each, the call
    goes on); the second subwindow's range 42..69 is given twice, the second
    time all duplicates of a subwindow that stays uniform.  40 and 41 stay lost."""
    _decoder_pair(L, [40, 41], _dup_before, lambda L, dec, dev, add: [])


def _dup_before(L, dec, dev, add):
    log = [add(L, dec, dev, 0, [100] * 10), add(L, dec, dev, 11, [100] * 29)]
    log.append(dec_add_single(L, dec, dev, 10, [100]))
    log.append(add(L, dec, dev, 0, [100] * 40))
    assert log[3] == (SUCCESS, 40, [DUPLICATE] * 40)
    log.append(add(L, dec, dev, 42, [100] * 28))
    log.append(add(L, dec, dev, 42, [100] * 28))
    assert log[5] == (SUCCESS, 28, [DUPLICATE] * 28)
    return log


def case_dec_after_recovery(L):
    """Decoder: packets 5 and 66 are lost and recovered; then they arrive
    after all, inside ranges with their received neighbours: DuplicateData for
    every packet, the recovered ones included."""
    def before(L, dec, dev, add):
        return [add(L, dec, dev, 0, [100] * 5), add(L, dec, dev, 6, [100] * 60), add(L, dec, dev, 67, [100] * 3)]

    def after(L, dec, dev, add):
        log = [add(L, dec, dev, 3, [100] * 5), add(L, dec, dev, 64, [100] * 6)]
        assert log[0] == (SUCCESS, 5, [DUPLICATE] * 5) and log[1] == (SUCCESS, 6, [DUPLICATE] * 6)
        return log
    _decoder_pair(L, [5, 66], before, after)


API_CASES = {
    "dec_duplicate": case_dec_duplicate,
    "dec_after_recovery": case_dec_after_recovery,
    "single_then_range": case_single_then_range,
    "mixed_length": case_mixed_length,
    "stride": case_stride,
    "bad_length": case_bad_length,
    "max_packets": case_max_packets,
    "fixed_block": case_fixed_block,
    "retransmit": case_retransmit,
    "restart_window": case_restart_window,
}


def run_config(library, name, path):
    """One harness config through `path` (dropin, batch, device_ge, defer):
    digests and status."""
    cfg = CONFIGS[name]
    if path == "dropin":
        res, _, _ = S.run_capi(library, cfg)
    else:
        res, rep = S.run_batch(library, cfg, verify=True, device_ge=path == "device_ge",
                               defer=2 if path == "defer" else 0, threads=2)
        assert rep.mismatches == 0 and rep.checked > 0
    return {"digests": S.digests(res), "status": [int(r.status) for r in res]}


def main(argv):
    library, case = argv[1], argv[2]
    if case in API_CASES:
        API_CASES[case](open_lib(library))
        print(json.dumps({"ok": True}))
    else:
        print(json.dumps(run_config(library, case, argv[3])))


if __name__ == "__main__":
    main(sys.argv)
