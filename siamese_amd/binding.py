"""ctypes binding of the siamese.h C ABI, for any library exporting it.

Used with siamese_amd/libsiamese_amd.so (the product), and in tests with the
upstream reference (oracle/_ref/libsiamese_ref.so) and the CPU test double
(tests/hostsim/libsiamese_hostsim.so), so API-level behaviour can be compared
call by call.
"""
import ctypes

SIAMESE_VERSION = 5
Success, InvalidInput, NeedMoreData, MaxPacketsReached, DuplicateData, Disabled = range(6)
RESULT_NAMES = ["Success", "InvalidInput", "NeedMoreData", "MaxPacketsReached",
                "DuplicateData", "Disabled"]


class OriginalPacket(ctypes.Structure):
    _fields_ = [("PacketNum", ctypes.c_uint), ("DataBytes", ctypes.c_uint),
                ("Data", ctypes.POINTER(ctypes.c_ubyte))]


class RecoveryPacket(ctypes.Structure):
    _fields_ = [("DataBytes", ctypes.c_uint), ("Data", ctypes.POINTER(ctypes.c_ubyte))]


class RowHead(ctypes.Structure):
    """SgpuRowHead (siamese_gpu.h): one frame row's record, 32 bytes."""
    _fields_ = [("FrameBytes", ctypes.c_uint), ("Status", ctypes.c_ubyte), ("Type", ctypes.c_ubyte),
                ("HeaderBytes", ctypes.c_ubyte), ("TailBytes", ctypes.c_ubyte), ("Flow", ctypes.c_uint),
                ("PacketNum", ctypes.c_uint), ("DataBytes", ctypes.c_uint), ("Head", ctypes.c_ubyte * 4),
                ("Tail", ctypes.c_ubyte * 8)]


ROW_EMPTY, ROW_OK, ROW_MALFORMED = 0, 1, 2


def bind_rows_abi(L):
    """Prototypes of the siamese_gpu.h calls that take frame rows where they
    lie in device memory, on a ctypes library that exports the batch ABI."""
    vp, u = ctypes.c_void_p, ctypes.c_uint
    L.sgpu_frames_scan_rows.restype = ctypes.c_longlong
    L.sgpu_frames_scan_rows.argtypes = [vp, ctypes.c_size_t, vp, u, vp]
    L.sgpu_frames_recv_rows.restype = ctypes.c_int
    L.sgpu_frames_recv_rows.argtypes = [vp, u, vp, vp, ctypes.c_size_t, u, vp, vp]
    L.sgpu_gather_wait.restype = ctypes.c_int
    L.sgpu_gather_wait.argtypes = [ctypes.c_longlong]
    return L


class PackedHead(ctypes.Structure):
    """SgpuPackedHead (siamese_gpu.h): one frame of a row that holds several,
    32 bytes; RowHead with the frame's offset in the row for FrameBytes."""
    _fields_ = [("Offset", ctypes.c_uint)] + RowHead._fields_[1:]


PACKED_MORE, PACKED_MALFORMED, PACKED_COUNT_MASK = 0x80000000, 0x40000000, 0xffff


def bind_packed_abi(L):
    """Prototypes of the siamese_gpu.h calls for rows that hold several frames
    (and of bind_rows_abi's calls, which they share tickets with)."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    bind_rows_abi(L)
    L.sgpu_frames_packed_bytes.restype = sz
    L.sgpu_frames_packed_bytes.argtypes = [u, u]
    L.sgpu_frames_scan_packed.restype = ctypes.c_longlong
    L.sgpu_frames_scan_packed.argtypes = [vp, sz, vp, u, u, vp]
    L.sgpu_frames_recv_packed.restype = ctypes.c_int
    L.sgpu_frames_recv_packed.argtypes = [vp, u, vp, u, vp, sz, u, vp, vp]
    L.sgpu_encoder_pack_frames.restype = ctypes.c_int
    L.sgpu_encoder_pack_frames.argtypes = [vp, u, u, u, vp, u, vp, sz, u, vp, vp, vp, vp]
    return L


def bind_dense_abi(L):
    """Prototypes of the dense packed scan (sgpu_frames_scan_dense and
    sgpu_frames_recv_dense) and of bind_packed_abi's calls."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    bind_packed_abi(L)
    L.sgpu_frames_dense_bytes.restype = sz
    L.sgpu_frames_dense_bytes.argtypes = [u, u]
    L.sgpu_frames_dense_records.restype = sz
    L.sgpu_frames_dense_records.argtypes = [u]
    L.sgpu_frames_scan_dense.restype = ctypes.c_longlong
    L.sgpu_frames_scan_dense.argtypes = [vp, sz, vp, u, u, u, vp]
    L.sgpu_frames_recv_dense.restype = ctypes.c_int
    L.sgpu_frames_recv_dense.argtypes = [vp, u, vp, u, u, vp, sz, u, vp, vp, vp]
    return L


STREAM_PARTIAL = 0x20000000


def bind_streams_abi(L):
    """Prototypes of the scan of byte-stream rows (sgpu_frames_scan_streams and
    sgpu_frames_recv_streams) and of bind_dense_abi's calls."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    bind_dense_abi(L)
    L.sgpu_frames_streams_bytes.restype = sz
    L.sgpu_frames_streams_bytes.argtypes = [u, u]
    L.sgpu_frames_streams_next.restype = sz
    L.sgpu_frames_streams_next.argtypes = [u, u]
    L.sgpu_frames_scan_streams.restype = ctypes.c_longlong
    L.sgpu_frames_scan_streams.argtypes = [vp, sz, vp, vp, u, u, u, vp]
    L.sgpu_frames_recv_streams.restype = ctypes.c_int
    L.sgpu_frames_recv_streams.argtypes = [vp, u, vp, u, u, vp, sz, u, vp, vp, vp, vp]
    return L


STREAM_PARTIAL_DUPLEX = 0x10000000


def bind_duplex_streams_abi(L):
    """Prototypes of the scan of duplex byte-stream rows
    (sgpu_frames_scan_duplex_streams and sgpu_frames_recv_duplex_streams)."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    L.sgpu_frames_duplex_streams_bytes.restype = sz
    L.sgpu_frames_duplex_streams_bytes.argtypes = [u, u, u, u]
    L.sgpu_frames_duplex_streams_next.restype = sz
    L.sgpu_frames_duplex_streams_next.argtypes = [u, u, u, u]
    L.sgpu_frames_scan_duplex_streams.restype = ctypes.c_longlong
    L.sgpu_frames_scan_duplex_streams.argtypes = [vp, sz, vp, vp, u, u, u, u, u, u, vp]
    L.sgpu_frames_recv_duplex_streams.restype = ctypes.c_int
    L.sgpu_frames_recv_duplex_streams.argtypes = [vp, u, vp, u, vp, u, u, u, u, u, vp, sz, u, vp, vp, vp, vp, vp]
    return L


def bind_relay_pack_abi(L):
    """Prototype of sgpu_decoder_pack_frames: a decoder's packets as wire
    frames packed several to a row, laid out on the device."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    L.sgpu_decoder_pack_frames.restype = ctypes.c_int
    L.sgpu_decoder_pack_frames.argtypes = [vp, u, u, u, vp, sz, u, vp, vp, vp, vp]
    return L


FRAME_ACK = 2
ROW_TRUNCATED = 3
PACKED_ACKS_DROPPED = 0x20000000


def bind_duplex_abi(L):
    """Prototypes of the ARQ calls of siamese_gpu.h ("Closing the loop"):
    acknowledgements and retransmissions on batch instances, their device rows,
    and the duplex scan that takes rows with ack frames in them."""
    vp, u, sz, i = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t, ctypes.c_int
    bind_packed_abi(L)

    def sig(name, res, args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args

    sig("sgpu_decoder_ack", i, [vp, vp, u, vp])
    sig("sgpu_encoder_acknowledge", i, [vp, ctypes.c_char_p, u, vp])
    sig("sgpu_encoder_retransmit", i, [vp, vp])
    sig("sgpu_encoder_stats", i, [vp, vp, u])
    sig("sgpu_decoder_stats", i, [vp, vp, u])
    sig("sgpu_frame_write_ack", u, [u, ctypes.c_char_p, u, vp, u])
    sig("sgpu_decoders_ack_frames", i, [vp, u, vp, u, vp, sz, vp, vp, vp])
    sig("sgpu_encoder_retransmit_frames", i, [vp, u, u, vp, sz, u, vp, vp, vp, vp])
    sig("sgpu_frames_duplex_bytes", sz, [u, u, u, u])
    sig("sgpu_frames_duplex_slots", sz, [u, u])
    sig("sgpu_frames_scan_duplex", ctypes.c_longlong, [vp, sz, vp, u, u, u, u, vp])
    sig("sgpu_frames_recv_duplex", i, [vp, u, vp, u, vp, u, u, u, vp, sz, u, vp, vp, vp])
    return L


def bind_duplex_dense_abi(L):
    """Prototypes of the dense duplex scan (sgpu_frames_scan_duplex_dense and
    sgpu_frames_recv_duplex_dense) and of bind_duplex_abi's and bind_dense_abi's
    calls."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    bind_duplex_abi(L)
    bind_dense_abi(L)
    L.sgpu_frames_duplex_dense_bytes.restype = sz
    L.sgpu_frames_duplex_dense_bytes.argtypes = [u, u, u, u]
    L.sgpu_frames_duplex_dense_acks.restype = sz
    L.sgpu_frames_duplex_dense_acks.argtypes = [u, u]
    L.sgpu_frames_duplex_dense_slots.restype = sz
    L.sgpu_frames_duplex_dense_slots.argtypes = [u, u]
    L.sgpu_frames_scan_duplex_dense.restype = ctypes.c_longlong
    L.sgpu_frames_scan_duplex_dense.argtypes = [vp, sz, vp, u, u, u, u, u, u, vp]
    L.sgpu_frames_recv_duplex_dense.restype = ctypes.c_int
    L.sgpu_frames_recv_duplex_dense.argtypes = [vp, u, vp, u, vp, u, u, u, u, u, vp, sz, u, vp, vp, vp, vp]
    return L


def bind_stream_abi(L):
    """Prototype of sgpu_decoder_deliver_stream: a decoder's packets as one
    contiguous byte stream at any byte alignment, summed and copied on the
    device."""
    vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
    L.sgpu_decoder_deliver_stream.restype = ctypes.c_int
    L.sgpu_decoder_deliver_stream.argtypes = [vp, u, u, vp, sz, vp, vp, vp, vp]
    return L


class SiameseError(RuntimeError):
    def __init__(self, what, code):
        name = RESULT_NAMES[code] if 0 <= code < 6 else str(code)
        super().__init__("%s -> %s" % (what, name))
        self.code = code


def _bytes(ptr, n):
    return ctypes.string_at(ptr, n) if n else b""


def _buf(data):
    return (ctypes.c_ubyte * max(1, len(data))).from_buffer_copy(data if data else b"\0")


class SiameseLib:
    """All 20 siamese.h entry points of one shared library."""

    def __init__(self, path):
        self.path = path
        L = self.L = ctypes.CDLL(path)
        vp, u, i = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int
        P = ctypes.POINTER

        def sig(name, res, args):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
            return f

        self.init_ = sig("siamese_init_", i, [i])
        self.encoder_create = sig("siamese_encoder_create", vp, [])
        self.encoder_free = sig("siamese_encoder_free", None, [vp])
        self.encoder_is_ready = sig("siamese_encoder_is_ready", i, [vp])
        self.encoder_add = sig("siamese_encoder_add", i, [vp, P(OriginalPacket)])
        self.encoder_get = sig("siamese_encoder_get", i, [vp, P(OriginalPacket)])
        self.encoder_remove_before = sig("siamese_encoder_remove_before", i, [vp, u])
        self.encoder_ack = sig("siamese_encoder_ack", i, [vp, vp, u, P(u)])
        self.encoder_retransmit = sig("siamese_encoder_retransmit", i, [vp, P(OriginalPacket)])
        self.encode = sig("siamese_encode", i, [vp, P(RecoveryPacket)])
        self.encoder_stats = sig("siamese_encoder_stats", i, [vp, P(ctypes.c_uint64), u])
        self.decoder_create = sig("siamese_decoder_create", vp, [])
        self.decoder_free = sig("siamese_decoder_free", None, [vp])
        self.decoder_add_original = sig("siamese_decoder_add_original", i,
                                        [vp, P(OriginalPacket)])
        self.decoder_add_recovery = sig("siamese_decoder_add_recovery", i,
                                        [vp, P(RecoveryPacket)])
        self.decoder_get = sig("siamese_decoder_get", i, [vp, P(OriginalPacket)])
        self.decoder_is_ready = sig("siamese_decoder_is_ready", i, [vp])
        self.decode = sig("siamese_decode", i, [vp, P(P(OriginalPacket)), P(u)])
        self.decoder_ack = sig("siamese_decoder_ack", i, [vp, vp, u, P(u)])
        self.decoder_stats = sig("siamese_decoder_stats", i, [vp, P(ctypes.c_uint64), u])
        self.ready = False

    def init(self):
        if not self.ready:
            rc = self.init_(SIAMESE_VERSION)
            if rc != Success:
                raise RuntimeError("%s: siamese_init failed (%s); an MI355X (gfx950) is "
                                   "required" % (self.path, RESULT_NAMES[rc] if rc < 6 else rc))
            self.ready = True
        return self

    def Encoder(self):
        return Encoder(self)

    def Decoder(self):
        return Decoder(self)


class Encoder:
    def __init__(self, lib):
        self.lib = lib.init()
        self.h = lib.encoder_create()
        if not self.h:
            raise MemoryError("siamese_encoder_create failed")

    def close(self):
        if self.h:
            self.lib.encoder_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def is_ready(self):
        return self.lib.encoder_is_ready(self.h)

    def add_raw(self, data):
        buf = _buf(data)
        p = OriginalPacket(0, len(data), buf)
        rc = self.lib.encoder_add(self.h, ctypes.byref(p))
        return rc, p.PacketNum

    def add(self, data):
        rc, num = self.add_raw(data)
        if rc:
            raise SiameseError("siamese_encoder_add", rc)
        return num

    def encode_raw(self):
        r = RecoveryPacket()
        rc = self.lib.encode(self.h, ctypes.byref(r))
        return rc, (_bytes(r.Data, r.DataBytes) if rc == Success else None)

    def encode(self):
        rc, data = self.encode_raw()
        if rc == NeedMoreData:
            return None
        if rc:
            raise SiameseError("siamese_encode", rc)
        return data

    def remove_before(self, num):
        return self.lib.encoder_remove_before(self.h, num)

    def get(self, num):
        p = OriginalPacket(num, 0, None)
        rc = self.lib.encoder_get(self.h, ctypes.byref(p))
        return rc, (_bytes(p.Data, p.DataBytes) if rc == Success else None)

    def ack(self, message):
        nxt = ctypes.c_uint()
        buf = _buf(message)
        rc = self.lib.encoder_ack(self.h, ctypes.cast(buf, ctypes.c_void_p), len(message),
                                  ctypes.byref(nxt))
        return rc, nxt.value

    def retransmit(self):
        p = OriginalPacket()
        rc = self.lib.encoder_retransmit(self.h, ctypes.byref(p))
        return rc, ((p.PacketNum, _bytes(p.Data, p.DataBytes)) if rc == Success else None)

    def stats(self):
        out = (ctypes.c_uint64 * 9)()
        self.lib.encoder_stats(self.h, out, 9)
        return list(out)


class Decoder:
    def __init__(self, lib):
        self.lib = lib.init()
        self.h = lib.decoder_create()
        if not self.h:
            raise MemoryError("siamese_decoder_create failed")

    def close(self):
        if self.h:
            self.lib.decoder_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_original(self, num, data):
        buf = _buf(data)
        p = OriginalPacket(num, len(data), buf)
        return self.lib.decoder_add_original(self.h, ctypes.byref(p))

    def add_recovery(self, data):
        buf = _buf(data)
        r = RecoveryPacket(len(data), buf)
        return self.lib.decoder_add_recovery(self.h, ctypes.byref(r))

    def is_ready(self):
        return self.lib.decoder_is_ready(self.h)

    def decode_raw(self):
        pkts = ctypes.POINTER(OriginalPacket)()
        n = ctypes.c_uint()
        rc = self.lib.decode(self.h, ctypes.byref(pkts), ctypes.byref(n))
        out = None
        if rc == Success:
            out = [(pkts[k].PacketNum, _bytes(pkts[k].Data, pkts[k].DataBytes))
                   for k in range(n.value)]
        return rc, out

    def decode(self):
        rc, out = self.decode_raw()
        if rc == NeedMoreData:
            return None
        if rc:
            raise SiameseError("siamese_decode", rc)
        return out

    def get(self, num):
        p = OriginalPacket(num, 0, None)
        rc = self.lib.decoder_get(self.h, ctypes.byref(p))
        return rc, (_bytes(p.Data, p.DataBytes) if rc == Success else None)

    def ack(self, limit=1024):
        buf = ctypes.create_string_buffer(limit)
        used = ctypes.c_uint()
        rc = self.lib.decoder_ack(self.h, buf, limit, ctypes.byref(used))
        return rc, (buf.raw[:used.value] if rc == Success else None)

    def stats(self):
        out = (ctypes.c_uint64 * 11)()
        self.lib.decoder_stats(self.h, out, 11)
        return list(out)
