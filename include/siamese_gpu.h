/*
    siamese_gpu.h -- device-resident batch API of libsiamese_amd (additive;
    not part of the upstream interface).

    siamese.h moves every packet through host memory and waits for the GPU on
    each siamese_encode / siamese_decode, which is the drop-in contract.  This
    header exposes the same codec with packets that stay in HBM:

      * originals are ingested from device pointers;
      * siamese_encode's result is a device-resident recovery packet that can
        be handed straight to a decoder on the same GPU;
      * nothing waits for the GPU until sgpu_flush(), so thousands of
        independent encoder/decoder pairs are driven per kernel launch.

    Per-instance call semantics, result codes and outputs are those of the
    corresponding siamese.h call (reference siamese.h:213-483); only the data
    location and the completion point differ.  Recovered packets returned by
    sgpu_decode carry device pointers whose DataBytes are exact after the
    next sgpu_flush() (they read 0 until then).

    Device pointer lifetime: a symbol an instance drops (a decoder sliding its
    window past delivered packets, a freed instance) is recycled once the
    submission holding that call has completed, and any later submission may
    then rewrite it.  Read (sgpu_gather_async / sgpu_gather_completed) the
    bytes behind a pointer from sgpu_decode, sgpu_decoder_get or sgpu_encode
    after the submission that produced them completes and before the next
    submission is enqueued; the gather's reads are ordered before that
    submission's device work.

    Threading: instances may be driven from many host threads at once, each
    instance by one thread at a time (handing a recovery packet to a decoder
    also touches the encoder that produced it).  Per-instance calls take no
    global lock.  sgpu_init, sgpu_flush, sgpu_submit, sgpu_enqueue,
    sgpu_gather, sgpu_h2d, and sgpu_decoder_get on a packet whose length is
    still pending (it flushes) must not run concurrently with any other call;
    sgpu_h2d_async and sgpu_gather_completed may run beside instance calls.

    Pipelined submission: sgpu_enqueue() hands all queued work to the
    library's launcher thread and returns a ticket at once; sgpu_wait(ticket)
    returns when that submission (and every earlier one) has run on the GPU
    and its results are delivered.  sgpu_wait may run while other threads
    drive instances.  An instance may be driven on while its earlier
    submissions are still in flight (a single stream keeps the GPU busy with
    one submission while the host prepares the next): completions never
    touch an instance's state behind its back, each call first applies the
    completions that have arrived.

    Deferred outputs: sgpu_decode_deferred and sgpu_decoder_get_deferred
    never wait for the GPU.  They write into entries the caller owns; an
    entry whose packet is still being solved gets its Data and DataBytes
    when the submission carrying the solve completes, before sgpu_query /
    sgpu_wait report that submission (or a later one) done.  The caller keeps
    such entries alive until then (freeing the decoder does not cancel them).
*/
#ifndef SIAMESE_GPU_H
#define SIAMESE_GPU_H

#include "siamese.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SgpuEncoderImpl { int impl; }* SgpuEncoder;
typedef struct SgpuDecoderImpl { int impl; }* SgpuDecoder;

/// Device-resident recovery packet (valid until the next sgpu_encode on the
/// same encoder).  Footer/Head are host copies the decoder parses directly.
typedef struct SgpuRecoveryPacket
{
    const unsigned char* DeviceData;   ///< payload + footer in HBM
    unsigned DataBytes;
    unsigned FooterBytes;
    unsigned char Footer[8];
    unsigned char Head[4];
    void* Producer;                    ///< internal: encoder that owns DeviceData
} SgpuRecoveryPacket;

/// Initialise the library on HIP device `device` (<0: current device).
SIAMESE_EXPORT int sgpu_init(int device);

SIAMESE_EXPORT SgpuEncoder sgpu_encoder_create(void);
SIAMESE_EXPORT void sgpu_encoder_free(SgpuEncoder encoder);
SIAMESE_EXPORT SiameseResult sgpu_encoder_add(SgpuEncoder encoder, const void* deviceData,
                                              unsigned bytes, unsigned* packetNumOut);
/// `count` sgpu_encoder_add calls in one: original k's payload at
/// deviceData + k * stride, bytes[k] bytes (fixedBytes for all when bytes is
/// NULL).  Identical to the calls made in order until one fails, whose
/// result is returned (Success if none did); *addedOut = originals added,
/// the first as packet *firstPacketNumOut and the others after it.  The
/// originals of one subwindow fill one slab: a run of adds costs one
/// allocation and one ingest descriptor (the reference's per-packet
/// siamese_encoder_add, siamese.cpp:96-108).
SIAMESE_EXPORT SiameseResult sgpu_encoder_add_range(SgpuEncoder encoder, const void* deviceData, size_t stride,
                                                    const unsigned* bytes, unsigned fixedBytes, unsigned count,
                                                    unsigned* firstPacketNumOut, unsigned* addedOut);
SIAMESE_EXPORT SiameseResult sgpu_encoder_remove_before(SgpuEncoder encoder, unsigned firstKept);
SIAMESE_EXPORT SiameseResult sgpu_encode(SgpuEncoder encoder, SgpuRecoveryPacket* out);
/// `count` sgpu_encode calls in one: out[k] = what the k-th call returns,
/// until a call does not succeed, whose result is returned (Success if none
/// failed; that call's out[k].DataBytes = 0); *producedOut = packets made.
/// Every packet of the call stays valid until the next sgpu_encode /
/// sgpu_encode_range on the same encoder.  Bit-exact with the single calls
/// (the reference's siamese_encode, siamese.cpp:159-168, per packet,
/// SiameseEncoder.cpp:1146-1254): a block-mode sender that knows how many
/// recovery packets it needs asks for them in one call.
SIAMESE_EXPORT SiameseResult sgpu_encode_range(SgpuEncoder encoder, SgpuRecoveryPacket* out, unsigned count,
                                               unsigned* producedOut);

SIAMESE_EXPORT SgpuDecoder sgpu_decoder_create(void);
SIAMESE_EXPORT void sgpu_decoder_free(SgpuDecoder decoder);
SIAMESE_EXPORT SiameseResult sgpu_decoder_add_original(SgpuDecoder decoder, unsigned packetNum,
                                                       const void* deviceData, unsigned bytes);
/// `count` sgpu_decoder_add_original calls in one: packet firstPacketNum + k
/// with its payload at deviceData + k * stride, bytes[k] bytes (fixedBytes
/// when bytes is NULL).  results[k] (optional) = call k's result; like the
/// calls, DuplicateData goes on and any other failure stops the run, its
/// result returned (Success if none stopped it); *callsOut = calls made.
/// (siamese_decoder_add_original, siamese.cpp:207-220, per packet.)
SIAMESE_EXPORT SiameseResult sgpu_decoder_add_original_range(SgpuDecoder decoder, unsigned firstPacketNum,
                                                             const void* deviceData, size_t stride,
                                                             const unsigned* bytes, unsigned fixedBytes,
                                                             unsigned count, SiameseResult* results,
                                                             unsigned* callsOut);
SIAMESE_EXPORT SiameseResult sgpu_decoder_add_recovery(SgpuDecoder decoder,
                                                       const SgpuRecoveryPacket* packet);
SIAMESE_EXPORT SiameseResult sgpu_decoder_is_ready(SgpuDecoder decoder);
SIAMESE_EXPORT SiameseResult sgpu_decode(SgpuDecoder decoder, SiameseOriginalPacket** packetsOut,
                                         unsigned* countOut);
/// sgpu_decode with the recovery matrix on the device: when the decode would
/// start a fresh elimination (GenerateMatrix + GaussianElimination,
/// reference SiameseDecoder.cpp:2157-2531) of at most 255 lost columns and
/// 256 recovery rows, the matrix job is queued and SGPU_DECODE_PENDING is
/// returned.  Flush (sgpu_flush, or wait for a later sgpu_enqueue ticket),
/// then call sgpu_decode_device again with the same arguments: it returns
/// what sgpu_decode would have returned, with the same outputs (an
/// elimination that stopped short of a pivot is repeated on the host, which
/// keeps the state the next attempt resumes from).  A square matrix of rows
/// of one length (a block decode) is chained, rows with wide LDPC sums
/// (windows of 512 originals or more) included: the elimination of received
/// data (with the wide rows' LDPC picks) and the solve ride in the same
/// submission, gated on the device elimination's outcome, so the packets
/// this second call returns already carry their exact lengths.  While a job is pending, every other call on
/// this decoder returns Siamese_InvalidInput.  Any other decode runs as
/// sgpu_decode does.
#define SGPU_DECODE_PENDING ((SiameseResult)6)
SIAMESE_EXPORT SiameseResult sgpu_decode_device(SgpuDecoder decoder, SiameseOriginalPacket** packetsOut,
                                                unsigned* countOut);
/// Returns a device pointer; waits for outstanding work if the packet's
/// exact length is still being computed.
SIAMESE_EXPORT SiameseResult sgpu_decoder_get(SgpuDecoder decoder, SiameseOriginalPacket* packet);
/// sgpu_decoder_get for packets firstPacketNum, firstPacketNum + 1, ... into
/// packets[0, count) until one does not return Success; *gotOut = packets
/// returned.  Returns the result of the get that stopped (Success if none).
SIAMESE_EXPORT SiameseResult sgpu_decoder_get_range(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                    SiameseOriginalPacket* packets, unsigned* gotOut);
/// Queue the delivery of packets firstPacketNum .. firstPacketNum+count-1 into
/// caller-owned device memory: packet k's payload (no length prefix) at
/// deviceDst + k*stride, bytes [len, stride) of that row zero, and its length
/// in deviceLens[k] (uint32, device memory).  Never waits for the GPU: rows and
/// lengths are in place when the submission that carries this call completes
/// (sgpu_flush / sgpu_wait / sgpu_query == 1).  The counterpart of
/// sgpu_decoder_add_original_range on the way out.
///
/// Present packets (received or recovered, including one whose solve is
/// queued in this same submission and whose length is still pending): row
/// and length are written, results[k] = Siamese_Success.
/// Absent packets: results[k] = Siamese_NeedMoreData, deviceLens[k] = 0 is
/// written and the row is left untouched, so a stream may be delivered into
/// one buffer again and again as it fills in.  *queuedOut = the number of
/// present packets; the call returns Siamese_Success even when some are
/// absent.
/// deviceLens[k] == 0 always means "row k holds no packet" (a packet is never
/// 0 bytes).  A packet that is present but does not fit, which only the
/// device can see for a packet still being solved -- a corrupt recovered
/// length prefix, a length past the symbol's capacity, a length above stride
/// -- gets a zeroed row and deviceLens[k] = 0; the decoder itself reports a
/// corrupt prefix as it always does (Siamese_Disabled once the submission has
/// completed).
///
/// Siamese_InvalidInput, with nothing queued: a null decoder; null deviceDst
/// or deviceLens with count > 0; deviceDst not 16-byte aligned; stride zero,
/// not a multiple of 16 or above 4 GiB; deviceLens not 4-byte aligned;
/// firstPacketNum > SIAMESE_PACKET_NUM_MAX; a packet of the range whose exact
/// length is already known and exceeds stride; a decoder with a device matrix
/// job pending (sgpu_decode_device).  A dead decoder returns
/// Siamese_Disabled.  count == 0 returns Siamese_Success with *queuedOut = 0.
///
/// The caller guarantees that nothing else reads or writes the rows or the
/// lengths from this call until that submission completes; two deliveries
/// into overlapping rows in one submission are undefined.  The arena's
/// lifetime rule is unchanged and the caller need not think about it here:
/// the delivery reads the symbols after every other device launch of its
/// submission, and a symbol that a later call of the same submission drops
/// (the window sliding on, the decoder freed) is recycled only after the
/// submission has completed.  An encoder's packets leave through
/// sgpu_encoder_deliver_range / sgpu_frames_deliver_recovery (below); a list
/// (non-range) form is not offered.
SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_range(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                        void* deviceDst, size_t stride, unsigned* deviceLens,
                                                        SiameseResult* results /* host, optional */,
                                                        unsigned* queuedOut);
/// sgpu_decoder_deliver_range with each present packet written as a wire frame
/// ("Framed datagrams" below): what a decode-and-forward relay sends on.  For
/// packet k of n payload bytes, with h = sgpu_frame_header_bytes(
/// SGPU_FRAME_ORIGINAL, n): bytes [0, h) of row k are what
/// sgpu_frame_write_header(SGPU_FRAME_ORIGINAL, flow, packetNum_k, n, ...)
/// writes, bytes [h, h + n) the payload, bytes [h + n, stride) zero, and
/// deviceLens[k] = h + n.  The row is byte for byte the row
/// sgpu_encoder_deliver_range wrote for the same packet and flow at the sender,
/// and valid input for sgpu_frames_parse, sgpu_frames_recv,
/// sgpu_frames_scan_rows and sgpu_frames_scan_packed.  packetNum_k =
/// (firstPacketNum + k) mod 2^22, as sgpu_decoder_get_range numbers its packets.
/// The header is computed on the device from the length read there, so a packet
/// whose solve is queued in this same submission is framed without a wait.
///
/// Everything else is sgpu_decoder_deliver_range's contract: the call never
/// waits; rows and lengths are in place when the carrying submission
/// completes; absent packets get results[k] = Siamese_NeedMoreData,
/// deviceLens[k] = 0 and an untouched row; the call returns Siamese_Success
/// with *queuedOut = the number of present packets; the lifetime and overlap
/// rules are the same, and the launch runs after every other launch of its
/// submission.  A present packet that does not fit, which only the device can
/// see while its length is pending -- an unreadable or zero prefix, symbol
/// header plus length past the symbol's capacity, h + n > stride (or a frame
/// length 7 + n above 2^29 - 1, which no frame can state) -- gets a zeroed row
/// and deviceLens[k] = 0.  The limit is h + n, not n: a packet that fits
/// sgpu_decoder_deliver_range's row of the same stride may not fit here.
///
/// Siamese_InvalidInput, with nothing queued: sgpu_decoder_deliver_range's
/// pointer, alignment, stride, packet number and pending-matrix-job rules;
/// flow > 2^24 - 1 (SGPU_FRAME_NONE included: the bare form is
/// sgpu_decoder_deliver_range); a packet of the range whose exact length is
/// already known and does not fit as above.  A dead decoder returns
/// Siamese_Disabled.  count == 0 returns Siamese_Success with *queuedOut = 0.
/// The form that packs several frames into one row is sgpu_decoder_pack_frames.
SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_frames(SgpuDecoder decoder, unsigned flow, unsigned firstPacketNum,
                                                         unsigned count, void* deviceDst, size_t stride,
                                                         unsigned* deviceLens,
                                                         SiameseResult* results /* host, optional */,
                                                         unsigned* queuedOut);
/// sgpu_decode without waiting (see "Deferred outputs" above): the recovered
/// packets are written to out[0, *countOut), PacketNum at once, Data and
/// DataBytes at once or when the solve's submission completes.  capacity must
/// be at least 255 (the most one solve recovers) and at least the packets
/// held by single-packet recoveries since the last decode; Siamese_InvalidInput
/// otherwise, with nothing consumed.
SIAMESE_EXPORT SiameseResult sgpu_decode_deferred(SgpuDecoder decoder, SiameseOriginalPacket* out,
                                                  unsigned capacity, unsigned* countOut);
/// sgpu_decoder_get without waiting: Success / NeedMoreData as
/// sgpu_decoder_get returns them; for a packet still being solved, *packet's
/// Data and DataBytes are written when the solve's submission completes.
SIAMESE_EXPORT SiameseResult sgpu_decoder_get_deferred(SgpuDecoder decoder, SiameseOriginalPacket* packet);
/// Non-blocking lookup: Success if the packet is present (length may still
/// be pending), NeedMoreData if not.
SIAMESE_EXPORT SiameseResult sgpu_decoder_has(SgpuDecoder decoder, unsigned packetNum);

/// Submit all queued device work of every instance and wait for it.
SIAMESE_EXPORT int sgpu_flush(void);
/// Submit, then complete the previous submission (one submission in flight).
SIAMESE_EXPORT int sgpu_submit(void);
/// Submit without waiting: returns the submission's ticket (>= 0; 0 when
/// nothing was ever queued), -1 once the device has failed.
SIAMESE_EXPORT long long sgpu_enqueue(void);
/// Wait for submission `ticket` and every earlier one; nonzero on a device
/// failure (sticky: every instance reports Siamese_Disabled afterwards).
SIAMESE_EXPORT int sgpu_wait(long long ticket);
/// Non-blocking: 1 if submission `ticket` has completed (as sgpu_wait would
/// return), 0 if it is still in flight, -1 once the device has failed.
SIAMESE_EXPORT int sgpu_query(long long ticket);
/// Run fn(ctx, i) for i in [0, count) on the library's host worker threads
/// (the caller takes part) and return when all calls are done.  Lets an
/// application drive many instances on the threads the library placed next
/// to the GPU.
SIAMESE_EXPORT void sgpu_parallel_for(unsigned count, void (*fn)(void* ctx, unsigned index),
                                      void* ctx);

/// Device memory helpers for applications and the benchmark harness.
SIAMESE_EXPORT void* sgpu_device_alloc(size_t bytes);
SIAMESE_EXPORT void sgpu_device_free(void* p);
/// Page-locked host memory (packet staging for DMA to and from the GPU).
SIAMESE_EXPORT void* sgpu_host_alloc(size_t bytes);
SIAMESE_EXPORT void sgpu_host_free(void* p);
SIAMESE_EXPORT int sgpu_h2d(void* deviceDst, const void* hostSrc, size_t bytes);
/// Gather `count` device ranges into one host buffer (concatenated in order).
/// Runs immediately; queued-but-unflushed codec work is left untouched.
/// Exactly the sum of bytes[] is written; a range of 0 bytes moves nothing
/// (its pointer is not read), and a call without a byte to move returns 0.
SIAMESE_EXPORT int sgpu_gather(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                               void* hostOut);

/// Asynchronous host -> device copy for packets arriving in pinned host
/// memory: issued at once on the library's staging stream; every submission
/// enqueued after this call waits for it on the device (the host never
/// blocks), so the copy overlaps the device work already in flight.  The
/// caller guarantees that no unfinished submission reads or writes deviceDst.
SIAMESE_EXPORT int sgpu_h2d_async(void* deviceDst, const void* hostSrc, size_t bytes);
/// Gather `count` device ranges produced by COMPLETED submissions into pinned
/// host memory (sgpu_host_alloc) on the library's gather stream, without
/// waiting for submissions still in flight.  Range i lands at offset
/// sum over k < i of align16(bytes[k]) (16-byte aligned, one DMA for all).
/// The bytes between a range's end and the next multiple of 16 are written
/// as zero, and nothing is written at or past the sum of all align16(bytes[k]);
/// a range of 0 bytes takes no room and moves nothing.  The device words read
/// are the aligned 16-byte words that hold a byte of a range, whole.
SIAMESE_EXPORT int sgpu_gather_completed(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                                         void* pinnedOut);
/// sgpu_gather_completed without waiting for the copy: returns a gather
/// ticket (> 0; -1 on failure) at once.  The sources are read before the
/// device work of any later submission runs (that work waits for them on the
/// device), so the instances owning them may be driven on right away;
/// pinnedOut holds the bytes once sgpu_gather_wait(ticket) returns 0.  May
/// run beside instance calls, like sgpu_gather_completed.  Every call's
/// ticket is larger than any earlier one; a call with count == 0, or whose ranges are all empty, moves
/// nothing and still returns a ticket that sgpu_gather_wait takes.
SIAMESE_EXPORT long long sgpu_gather_async(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                                           void* pinnedOut);
/// Wait until gather `ticket` and every earlier one have landed in host
/// memory.  0 on success, -1 after a device fault.
SIAMESE_EXPORT int sgpu_gather_wait(long long ticket);

/*
    Framed datagrams: packet ingest and egress in bulk (the UDP side of an
    application; replaces nothing in siamese.h).  A frame carries one
    datagram:
      [L: byte length of the rest, in the symbol length-prefix format of
          the reference (SiameseSerializers.h:566-593), 1-4 bytes]
      [type: 1 byte, SGPU_FRAME_ORIGINAL, SGPU_FRAME_RECOVERY or SGPU_FRAME_ACK]
      [flow: 3 bytes little-endian, the application's stream id]
      original:  [PacketNum: 3 bytes LE] [payload]
      recovery:  [the recovery packet, its metadata footer included
                  (SiameseSerializers.h:736-800)]
      ack:       [the acknowledgement message, exactly as sgpu_decoder_ack
                  wrote it: at least 1 byte, so L >= 5; no upper bound but the
                  frame format's]
    Frames follow each other directly; a zero byte where a frame would start
    is an empty frame and is skipped (senders pad frames with zeros).
    Ack frames are taken by the duplex calls alone ("Closing the loop" below):
    sgpu_frames_parse, sgpu_frames_recv, sgpu_frames_scan_rows,
    sgpu_frames_scan_packed, sgpu_frames_recv_rows, sgpu_frames_recv_packed,
    sgpu_frame_header_bytes and sgpu_frame_write_header know two types and call
    type 2 malformed.
*/
#define SGPU_FRAME_ORIGINAL 0
#define SGPU_FRAME_RECOVERY 1
#define SGPU_FRAME_ACK      2

typedef struct SgpuFrame
{
    unsigned Type;        ///< SGPU_FRAME_ORIGINAL / SGPU_FRAME_RECOVERY
    unsigned Flow;
    unsigned PacketNum;   ///< originals
    unsigned Offset;      ///< byte offset of the data (payload / recovery packet) in the buffer
    unsigned Bytes;       ///< data bytes
} SgpuFrame;

/// Header bytes a frame of `type` carrying `dataBytes` puts before its data.
SIAMESE_EXPORT unsigned sgpu_frame_header_bytes(unsigned type, unsigned dataBytes);
/// Write a frame header to `out` (sgpu_frame_header_bytes bytes); the data
/// follows it.  Returns the header size, 0 on invalid input.
SIAMESE_EXPORT unsigned sgpu_frame_write_header(unsigned type, unsigned flow, unsigned packetNum,
                                                unsigned dataBytes, void* out);
/// Parse up to maxFrames frames of frames[0, bytes) (host memory, bytes <
/// 4 GiB).  InvalidInput on a malformed frame or when more frames remain;
/// the frames before a malformed one are still returned (*countOut).
SIAMESE_EXPORT SiameseResult sgpu_frames_parse(const void* frames, size_t bytes, SgpuFrame* out,
                                               unsigned maxFrames, unsigned* countOut);
/// Packet ingest: the frames in hostFrames[0, bytes) (pinned host memory)
/// whose identical copy the caller staged at deviceFrames with
/// sgpu_h2d_async.  Parses them in bulk and hands each datagram to
/// decoders[flow]: originals to sgpu_decoder_add_original, recovery packets
/// to sgpu_decoder_add_recovery (footer and head read from the host copy,
/// the bytes copied from the device copy by the next submission, which
/// waits for the staging copy on the device).  results[i] (optional) is the
/// call's result for frame i (InvalidInput for a flow without a decoder).
/// A malformed frame ends the call: every frame before it is delivered and
/// counted in *countOut, and the call returns InvalidInput.  bytes < 4 GiB.
/// The decoders must not be driven concurrently with this call; deviceFrames
/// stays untouched until the next submission has completed.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv(const SgpuDecoder* decoders, unsigned decoderCount,
                                              const void* hostFrames, const void* deviceFrames, size_t bytes,
                                              SiameseResult* results, unsigned maxFrames, unsigned* countOut);
/// Packet egress: frame `count` recovery packets (flows[i] their stream ids)
/// into pinned host memory without waiting (a gather, as
/// sgpu_gather_async: same lifetime rule for the packets).  Frame i starts
/// at a 16-byte boundary, zero padding between frames.  *bytesOut = the
/// frame stream's length (<= capacity).  Returns a gather ticket for
/// sgpu_gather_wait, -1 on failure (capacity too small, a packet of 0 or more
/// than SIAMESE_MAX_PACKET_BYTES bytes, device fault).
SIAMESE_EXPORT long long sgpu_frames_send(unsigned count, const SgpuRecoveryPacket* packets, const unsigned* flows,
                                          void* pinnedOut, size_t capacity, size_t* bytesOut);

/*
    Packets out of the sender, into caller-owned device rows: the wire
    datagrams of a stream, originals and recovery packets, placed by the same
    submission that encodes them, without a second device pass and without
    waiting (sgpu_frames_send gathers packets of completed submissions into
    host memory; the originals it cannot frame at all).

    Row contract of both calls: row k starts at deviceDst + k*stride.  Bytes
    [0, h) are the frame header exactly as sgpu_frame_write_header writes it
    (h = 0 for a bare packet), bytes [h, h+n) the packet -- a recovery packet's
    payload and footer (n = DataBytes), an original's payload without its
    symbol length prefix -- and bytes [h+n, stride) are zero; deviceLens[k] =
    h+n (uint32, device memory).  Rows are multiples of 16 bytes with zero
    tails, so the whole buffer read as one byte string is a valid frame stream
    for sgpu_frames_parse / sgpu_frames_recv: ready for one copy to the host,
    for a NIC that reads device memory, or for a decoder on the same GPU
    (sgpu_frames_scan_rows + sgpu_frames_recv_rows below take the rows where
    they lie).

    Neither call ever waits for the GPU: rows and lengths are in place when
    the submission that carries the call completes (sgpu_flush / sgpu_wait /
    sgpu_query == 1).  A recovery packet made by an sgpu_encode of the same
    submission is delivered from its final bytes, an original added in the same
    submission is delivered too.

    Siamese_InvalidInput, with nothing queued: null deviceDst or deviceLens
    with count > 0; deviceDst not 16-byte aligned; stride zero, not a multiple
    of 16 or above 4 GiB; deviceLens not 4-byte aligned; a flow above 2^24-1
    other than SGPU_FRAME_NONE; any packet whose h+n exceeds stride (every
    length is known on the host, so this is always caught by the call).
    count == 0 returns Siamese_Success with *queuedOut = 0.

    The caller guarantees that nothing else reads or writes the rows or the
    lengths from the call until that submission completes; two deliveries into
    overlapping rows in one submission are undefined.  The arena's lifetime
    rule needs no thought here: the frames are read after every other device
    launch of their submission, and a packet that a later call of the same
    submission drops (the next sgpu_encode, sgpu_encoder_remove_before, the
    encoder freed) is recycled only after the submission has completed.
*/
/// No frame header: rows hold the bare packet (flow argument of the calls below).
#define SGPU_FRAME_NONE 0xffffffffu

/// Queue `count` recovery packets (as sgpu_encode / sgpu_encode_range returned
/// them, each still its encoder's current output) into caller-owned device
/// rows, packet k framed as SGPU_FRAME_RECOVERY for flows[k] (flows == NULL, or
/// flows[k] == SGPU_FRAME_NONE: the bare packet).  Touches each packet's
/// producing encoder, the same threading rule as sgpu_decoder_add_recovery.
/// Also Siamese_InvalidInput, every packet being checked before any is queued:
/// null packets with count > 0; a packet with null DeviceData, null Producer,
/// or DataBytes of 0 or more than SIAMESE_MAX_PACKET_BYTES.  Siamese_Disabled
/// once the device has failed.  *queuedOut = count on success.
SIAMESE_EXPORT SiameseResult sgpu_frames_deliver_recovery(unsigned count, const SgpuRecoveryPacket* packets,
                                                          const unsigned* flows, void* deviceDst, size_t stride,
                                                          unsigned* deviceLens, unsigned* queuedOut);
/// Queue originals firstPacketNum .. firstPacketNum+count-1 held by `encoder`
/// into caller-owned device rows, framed as SGPU_FRAME_ORIGINAL for `flow`
/// (SGPU_FRAME_NONE: bare payloads): what a sender retransmitting a NACKed
/// range needs, without a copy of its own of every original.
/// Absent originals (never added, or already removed from the window by
/// sgpu_encoder_remove_before): results[k] = Siamese_NeedMoreData,
/// deviceLens[k] = 0 is written and the row is left untouched, as in
/// sgpu_decoder_deliver_range -- an untouched row may still hold an older
/// frame, so the lengths decide which rows to send.  Present ones: results[k] =
/// Siamese_Success.  The call returns Siamese_Success even when some are
/// absent; *queuedOut = the number present.
/// Also Siamese_InvalidInput: a null encoder; firstPacketNum >
/// SIAMESE_PACKET_NUM_MAX.  A disabled encoder returns Siamese_Disabled.
SIAMESE_EXPORT SiameseResult sgpu_encoder_deliver_range(SgpuEncoder encoder, unsigned firstPacketNum, unsigned count,
                                                        unsigned flow, void* deviceDst, size_t stride,
                                                        unsigned* deviceLens,
                                                        SiameseResult* results /* host, optional */,
                                                        unsigned* queuedOut);

/*
    Frame rows that exist only in device memory, into decoders: the way in
    that matches the two calls above (and a NIC that writes datagrams into
    HBM).  sgpu_frames_recv needs an identical host copy of the whole frame
    stream; here the host gets 32 bytes per row and the payloads never leave
    the device.  sgpu_frames_scan_rows has the device read each row's frame
    header, and for a recovery packet its first and last bytes, into one
    SgpuRowHead; sgpu_frames_recv_rows routes the rows to their decoders from
    those records:

        ticket = sgpu_frames_scan_rows(rows, stride, lens, count, heads);
        sgpu_gather_wait(ticket);
        sgpu_frames_recv_rows(decoders, n, heads, rows, stride, count, results, &accepted);

    Row k starts at deviceRows + k*stride and holds one frame from its first
    byte (the row contract of the deliver calls above, or any datagram of the
    "Framed datagrams" format), rows 16-byte aligned, stride a multiple of 16.
*/
#define SGPU_ROW_EMPTY     0   /* no frame in the row */
#define SGPU_ROW_OK        1
#define SGPU_ROW_MALFORMED 2

/// One row's record: 32 bytes, every field little-endian as the host reads
/// it, records 16-byte aligned in pinnedOut.  An empty or malformed row's
/// record is zero but for Status.
typedef struct SgpuRowHead
{
    unsigned      FrameBytes;  ///< header + data bytes of the frame in this row (its prefix + L); 0: empty or malformed row
    unsigned char Status;      ///< SGPU_ROW_OK / SGPU_ROW_EMPTY / SGPU_ROW_MALFORMED
    unsigned char Type;        ///< SGPU_FRAME_ORIGINAL / SGPU_FRAME_RECOVERY
    unsigned char HeaderBytes; ///< offset of the data in the row (<= 11)
    unsigned char TailBytes;   ///< valid bytes in Tail: min(8, DataBytes); originals: 0
    unsigned      Flow;
    unsigned      PacketNum;   ///< originals (recovery packets: 0)
    unsigned      DataBytes;
    unsigned char Head[4];     ///< recovery: first min(4, DataBytes) bytes of the packet, rest zero
    unsigned char Tail[8];     ///< recovery: the packet's last TailBytes bytes, right-aligned, rest zero
} SgpuRowHead;
#if defined(__cplusplus)
static_assert(sizeof(SgpuRowHead) == 32, "SgpuRowHead is 32 bytes");
#else
_Static_assert(sizeof(SgpuRowHead) == 32, "SgpuRowHead is 32 bytes");
#endif

/// Scan `count` frame rows into pinnedOut[0, count) (pinned host memory,
/// sgpu_host_alloc) with one kernel launch.  A gather, with the contract of
/// sgpu_gather_async and sgpu_frames_send: never waits, returns a gather
/// ticket (> 0) for sgpu_gather_wait, may run beside instance calls;
/// pinnedOut[k] is valid once sgpu_gather_wait(ticket) returns 0.  The rows
/// were written by COMPLETED submissions or by something outside the library;
/// they are read before the device work of any later submission runs.
///
/// deviceLens (optional, uint32 in device memory, as the deliver calls write
/// them): deviceLens[k] == 0 makes row k empty whatever bytes it still holds
/// (the lengths decide); a non-zero length must equal the frame's own
/// prefix + L, or the row is malformed.  deviceLens == NULL: a zero first byte
/// is an empty row, otherwise the frame's own length prefix decides.
/// A row is malformed when: its length prefix gives L = 0 or prefix + L >
/// stride (the prefix is judged exactly as sgpu_frames_parse judges it, which
/// accepts a prefix wider than its L needs); type > 1; L is not larger than
/// the type's inner header (4 bytes, an original's 7); an original's
/// PacketNum > SIAMESE_PACKET_NUM_MAX; DataBytes > SIAMESE_MAX_PACKET_BYTES.
/// Each row stands alone: a malformed row never stops the scan.
///
/// Returns -1, with nothing queued: null deviceRows or pinnedOut with
/// count > 0; deviceRows not 16-byte aligned; stride zero, not a multiple of
/// 16 or above 4 GiB; deviceLens not 4-byte aligned; pinnedOut not 16-byte
/// aligned; a failed device.  count == 0 returns a valid ticket that is
/// already complete.
SIAMESE_EXPORT long long sgpu_frames_scan_rows(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                               unsigned count, SgpuRowHead* pinnedOut);
/// Host only: hand the rows to their decoders from their records, queueing
/// work like sgpu_frames_recv and waiting for nothing.  For row k with Status
/// OK, the data at deviceRows + k*stride + HeaderBytes goes to decoders[Flow]:
/// an original to sgpu_decoder_add_original, a recovery packet to
/// sgpu_decoder_add_recovery (its footer parsed from Tail, its head taken from
/// Head; the bytes are copied from the row by the next submission).
/// results[k] (optional) = that call's result; Siamese_InvalidInput for a flow
/// without a decoder or a decoder with a device matrix job pending
/// (sgpu_decode_device), as in sgpu_frames_recv.  Empty rows: results[k] =
/// Siamese_NeedMoreData, skipped.  Malformed rows: Siamese_InvalidInput,
/// skipped; the rows after them are still delivered.  The records are caller
/// data and never trusted: one whose Status is unknown, whose HeaderBytes +
/// DataBytes exceeds stride or FrameBytes, or whose Type, HeaderBytes,
/// TailBytes, DataBytes, Flow or PacketNum the format cannot produce, counts as
/// malformed.  *acceptedOut = the rows handed to a decoder.
/// Returns Siamese_InvalidInput, with nothing queued, for a null acceptedOut
/// and for null decoders, heads or deviceRows with count > 0, heads not
/// 4-byte aligned, and the scan's rules for deviceRows and stride; otherwise
/// the first per-row result that is neither Success nor NeedMoreData (Success
/// if none).  For well-formed rows the decoders end in the state
/// sgpu_frames_recv leaves them in when given a host copy of the same bytes.
/// The decoders must not be driven concurrently with this call; the rows stay
/// untouched until the next submission has completed.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_rows(const SgpuDecoder* decoders, unsigned decoderCount,
                                                   const SgpuRowHead* heads, const void* deviceRows, size_t stride,
                                                   unsigned count, SiameseResult* results /* optional */,
                                                   unsigned* acceptedOut);

/*
    Rows that hold several frames: an MTU-sized datagram that carries a few
    small originals and the recovery packet that protects them, frames
    following each other as "Framed datagrams" allows (zero bytes between
    them are skipped).  The two calls above take one frame per row from the
    row's first byte; these take every frame of a row, at any byte offset:

        bytes  = sgpu_frames_packed_bytes(count, maxFrames);      // pinned, sgpu_host_alloc
        ticket = sgpu_frames_scan_packed(rows, stride, lens, count, maxFrames, out);
        sgpu_gather_wait(ticket);
        sgpu_frames_recv_packed(decoders, n, out, maxFrames, rows, stride, count, results, &accepted);

    out holds count * maxFrames SgpuPackedHead records, row k's at index
    k * maxFrames, and after them count uint32 row words: SGPU_PACKED_COUNT
    records of the row are SGPU_ROW_OK (its first ones, in the order of the
    frames), every other record is zero.  sgpu_encoder_pack_frames (below)
    builds such rows on the device.
*/
#define SGPU_PACKED_MORE      0x80000000u  /* frames (non-zero bytes) remain after maxFrames records */
#define SGPU_PACKED_MALFORMED 0x40000000u  /* the walk stopped at a frame it could not accept */
#define SGPU_PACKED_COUNT(w)  ((w) & 0xffffu)

/// One frame's record: 32 bytes, SgpuRowHead with Offset in place of FrameBytes.
typedef struct SgpuPackedHead
{
    unsigned      Offset;      ///< byte offset of the frame's first byte (its length prefix) in the row
    unsigned char Status;      ///< SGPU_ROW_OK; SGPU_ROW_EMPTY (a zero record) past the row's last frame
    unsigned char Type;        ///< as SgpuRowHead
    unsigned char HeaderBytes; ///< the data is at Offset + HeaderBytes (HeaderBytes <= 11)
    unsigned char TailBytes;
    unsigned      Flow;
    unsigned      PacketNum;
    unsigned      DataBytes;
    unsigned char Head[4];
    unsigned char Tail[8];
} SgpuPackedHead;
#if defined(__cplusplus)
static_assert(sizeof(SgpuPackedHead) == 32, "SgpuPackedHead is 32 bytes");
#else
_Static_assert(sizeof(SgpuPackedHead) == 32, "SgpuPackedHead is 32 bytes");
#endif

/// Bytes of a packed scan's output: count * maxFrames records, then count row
/// words (0 for maxFrames outside 1..256).
SIAMESE_EXPORT size_t sgpu_frames_packed_bytes(unsigned count, unsigned maxFrames);
/// Scan `count` rows of up to maxFrames (1..256) frames each into pinnedOut
/// (pinned, 16-byte aligned, sgpu_frames_packed_bytes) with one kernel launch:
/// a gather with sgpu_frames_scan_rows' contract, tickets and arguments.  Every
/// record and every row word is written by every scan.
///
/// Row k, with end = deviceLens ? deviceLens[k] : stride:
///   - deviceLens[k] == 0: an empty row whatever bytes it holds, row word 0;
///   - deviceLens[k] > stride: row word SGPU_PACKED_MALFORMED, no records;
///   - otherwise the records are the frames sgpu_frames_parse finds in
///     row[0, end), in order: zero bytes where a frame would start are skipped,
///     the prefix is judged with the bytes that remain before end, and a frame
///     is accepted under sgpu_frames_scan_rows' per-frame rules with
///     Offset + HeaderBytes + DataBytes <= end.  The first frame that is not
///     accepted ends the row's walk: the frames before it are reported and
///     SGPU_PACKED_MALFORMED is set.  It never affects another row.
///   - after maxFrames records the walk stops, and SGPU_PACKED_MORE is set if a
///     non-zero byte remains before end (scan again with a larger maxFrames).
/// Bytes in [end, stride) are ignored (they may be read); nothing outside
/// [row, row + stride) and the row's length word is read.
///
/// Returns -1, with nothing queued, as sgpu_frames_scan_rows does, and for
/// maxFrames outside 1..256 or an output above 4 GiB.  count == 0 returns a
/// valid ticket that is already complete.
SIAMESE_EXPORT long long sgpu_frames_scan_packed(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                 unsigned count, unsigned maxFrames, void* pinnedOut);
/// Host only: sgpu_frames_recv_rows for a packed scan's output (`heads`, 4-byte
/// aligned): for row k the first min(SGPU_PACKED_COUNT(word k), maxFrames)
/// records are routed in order, record j's data being at deviceRows + k*stride
/// + Offset + HeaderBytes.  results[k*maxFrames + j] (optional, count *
/// maxFrames entries) = the result for record j of row k, as
/// sgpu_frames_recv_rows gives it; unused slots get Siamese_NeedMoreData.  A row
/// whose word has SGPU_PACKED_MALFORMED contributes Siamese_InvalidInput to the
/// return value after its good frames have been delivered.  The records and
/// words are caller data and never trusted: each is copied and checked against
/// stride before use; a record that fails, or a word whose count exceeds
/// maxFrames, counts as malformed.  *acceptedOut = the frames handed to a
/// decoder.  Arguments are refused as in sgpu_frames_recv_rows, and for
/// maxFrames outside 1..256.  For well-formed rows the decoders end in the
/// state sgpu_frames_recv leaves them in, given a host copy of the same bytes.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_packed(const SgpuDecoder* decoders, unsigned decoderCount,
                                                     const void* heads, unsigned maxFrames, const void* deviceRows,
                                                     size_t stride, unsigned count,
                                                     SiameseResult* results /* count*maxFrames, optional */,
                                                     unsigned* acceptedOut);
/*
    The packed scan in dense form.  sgpu_frames_scan_packed's output is sized by
    the fullest row the receiver might see: count * maxFrames records cross to
    the host whatever the rows hold.  The dense scan runs the same walk under
    the same per-frame rules and puts the accepted records of all rows back to
    back, so the caller sizes the output by the frames it expects in all:

        bytes  = sgpu_frames_dense_bytes(count, maxRecords);      // pinned, sgpu_host_alloc
        ticket = sgpu_frames_scan_dense(rows, stride, lens, count, maxFrames, maxRecords, out);
        sgpu_gather_wait(ticket);
        sgpu_frames_recv_dense(decoders, n, out, maxFrames, maxRecords, rows, stride, count,
                               results, &rowsDone, &accepted);
        // rowsDone < count: scan again from row rowsDone

    out holds, little-endian and in this order:
      - info, four uint32 {T, W, c, 0};
      - count row words, word k exactly what sgpu_frames_scan_packed writes for
        row k with the same maxFrames;
      - count + 1 start words: start[0] = 0, start[k+1] = start[k] +
        SGPU_PACKED_COUNT(word k), T = start[count];
      - zeros up to the next 16-byte boundary, sgpu_frames_dense_records(count);
      - maxRecords SgpuPackedHead records.
    Rows are all or nothing: c is the largest value with start[c] <= maxRecords
    and W = start[c].  Records [start[k], start[k+1]) for k < c are byte for
    byte the first records the packed scan writes for row k (Offset stays
    relative to that row); records [W, maxRecords) are zero.  Every byte is
    written by every scan.  maxRecords >= maxFrames, so a scan of at least one
    row completes at least one row.
*/
/// Bytes of a dense scan's output (0 for maxRecords == 0 or above count * 256).
SIAMESE_EXPORT size_t sgpu_frames_dense_bytes(unsigned count, unsigned maxRecords);
/// Byte offset of record 0 in a dense scan's output.
SIAMESE_EXPORT size_t sgpu_frames_dense_records(unsigned count);
/// sgpu_frames_scan_packed into the dense layout above (pinnedOut: pinned,
/// 16-byte aligned, sgpu_frames_dense_bytes), with three kernel launches and
/// one copy: the gather ticket, sgpu_gather_wait, what may be read and what
/// later submissions wait for are the packed scan's.  Returns -1, with nothing
/// queued, where sgpu_frames_scan_packed does, for maxFrames outside 1..256,
/// maxRecords < maxFrames, maxRecords > count * maxFrames (no scan can need
/// that many) or an output of 4 GiB or more.  count == 0 returns a valid ticket
/// that is already complete, and nothing is written.
SIAMESE_EXPORT long long sgpu_frames_scan_dense(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                unsigned count, unsigned maxFrames, unsigned maxRecords,
                                                void* pinnedOut);
/// Host only: sgpu_frames_recv_packed for a dense scan's output (`heads`, 4-byte
/// aligned).  The records of rows [0, c) are routed in order, record i of row k
/// having its data at deviceRows + k*stride + Offset + HeaderBytes.  results[i]
/// (optional, maxRecords entries) = the result for record i;
/// Siamese_NeedMoreData for slots from W on.  *rowsOut = c, the rows routed:
/// when it is below count, scan again from that row.  *acceptedOut = the frames
/// handed to a decoder.  A row whose word has SGPU_PACKED_MALFORMED contributes
/// Siamese_InvalidInput to the return value after its good frames have been
/// delivered.  The output is caller data and never trusted: info is copied, and
/// c <= count, W <= maxRecords, start[0] == 0, non-decreasing starts,
/// start[k+1] - start[k] == min(SGPU_PACKED_COUNT(word k), maxFrames) for
/// k < c and start[c] == W are checked before a row's records are touched, and
/// each record is copied and checked against stride as sgpu_frames_recv_packed
/// checks one.  At the first start that fails, routing stops, *rowsOut = the
/// rows routed before it and the call returns Siamese_InvalidInput; a record
/// that fails, or a word whose count exceeds maxFrames, counts as malformed.
/// Arguments are refused as in sgpu_frames_recv_packed, for a null rowsOut and
/// for the sizes sgpu_frames_scan_dense refuses.  For well-formed rows the
/// decoders end in the state sgpu_frames_recv_packed leaves them in on the same
/// rows.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_dense(const SgpuDecoder* decoders, unsigned decoderCount,
                                                    const void* heads, unsigned maxFrames, unsigned maxRecords,
                                                    const void* deviceRows, size_t stride, unsigned count,
                                                    SiameseResult* results /* maxRecords, optional */,
                                                    unsigned* rowsOut, unsigned* acceptedOut);
/*
    Rows that are byte streams.  The scans above take a row as one datagram: a
    frame that does not end inside it is malformed.  A per-connection receive
    buffer in device memory (a stream transport, an RDMA ring, a relay's
    sgpu_frames_send-style stream landing on another GPU) holds frames back to
    back instead, and its last frame is usually still arriving.  The stream scan
    walks row bytes [start, end), tells a frame that the data does not yet hold
    whole (partial) from one that is wrong (malformed), and says for every row
    where its next scan starts:

        bytes  = sgpu_frames_streams_bytes(count, maxRecords);    // pinned, sgpu_host_alloc
        for (;;) {
            // the transport has advanced ends[k]; starts[k] is where row k's last scan stopped
            ticket = sgpu_frames_scan_streams(rows, stride, starts, ends, count, maxFrames, maxRecords, out);
            sgpu_gather_wait(ticket);
            sgpu_frames_recv_streams(decoders, n, out, maxFrames, maxRecords, rows, stride, count,
                                     results, consumed, &rowsDone, &accepted);
            // consumed[k], k < rowsDone, is row k's next start: write it back to starts[k]
            // (rows from rowsDone on keep their old starts and are scanned again);
            // when a start nears stride, move the row's bytes [start, end) to its front
        }

    out holds sgpu_frames_scan_dense's layout, sgpu_frames_dense_bytes(count,
    maxRecords) bytes of it, and then, at sgpu_frames_streams_next(count,
    maxRecords), count uint32 next words and zeros up to the next 16-byte
    boundary.  Every byte is written by every scan.  A record's Offset is
    relative to the row's first byte, not to start.  Still not offered: a ring
    that wraps around inside a row (compact it, or map it twice) and more than
    256 frames per row and scan (resume from the next word).  Ack frames in
    stream rows are malformed here; sgpu_frames_scan_duplex_streams takes them.
*/
#define SGPU_STREAM_PARTIAL 0x20000000u  /* row word: the walk stopped at a frame the data does not yet hold whole */

/// Bytes of a stream scan's output (0 where sgpu_frames_dense_bytes is 0).
SIAMESE_EXPORT size_t sgpu_frames_streams_bytes(unsigned count, unsigned maxRecords);
/// Byte offset of the next words in a stream scan's output: sgpu_frames_dense_bytes(count, maxRecords).
SIAMESE_EXPORT size_t sgpu_frames_streams_next(unsigned count, unsigned maxRecords);
/// Scan `count` byte-stream rows into pinnedOut (pinned, 16-byte aligned,
/// sgpu_frames_streams_bytes): a gather with sgpu_frames_scan_dense's ticket,
/// ordering and lifetime contract, its rows, stride, maxFrames and maxRecords.
///
/// Row k is walked over its bytes [start, end), start = deviceStarts ?
/// deviceStarts[k] : 0 and end = deviceEnds ? deviceEnds[k] : stride (uint32
/// arrays in device memory, 4-byte aligned; byte offsets from the row's first
/// byte, at any alignment), as sgpu_frames_scan_packed walks a row from 0: zero
/// bytes where a frame would start are skipped, the prefix is judged with the
/// bytes left before end, and a frame is accepted under sgpu_frames_scan_rows'
/// per-frame rules (types 0 and 1).  Row word k and next word k say how the walk
/// ended:
///   - start > end or end > stride: SGPU_PACKED_MALFORMED, no records, next =
///     min(start, stride);
///   - only zero bytes were left: the count n, next = end;
///   - n == maxFrames and a non-zero byte is left: n | SGPU_PACKED_MORE, next =
///     that byte's offset;
///   - a partial frame at `at`: n | SGPU_STREAM_PARTIAL, next = at.  With left =
///     end - at, the frame is partial when its first byte announces a prefix of
///     w bytes and left < w, or the prefix gives L >= 1 and w + L > left, and
///     nothing that is present is wrong already;
///   - a frame at `at` that is whole and fails a rule (L == 0 included), or that
///     is cut off and can never become valid -- w + L > stride, a type byte that
///     is present and above 1, a type byte that is present with L not above the
///     type's inner header, an original whose three PacketNum bytes are present
///     and exceed SIAMESE_PACKET_NUM_MAX -- : n | SGPU_PACKED_MALFORMED, next =
///     at, so that a connection never stalls on junk.
/// (With a null deviceEnds and a stride of 4 GiB, next = end is stated as 2^32 -
/// 1.)  With start 0 and no partial frame the first sgpu_frames_dense_bytes bytes
/// are sgpu_frames_scan_dense's on the same rows and sizes, byte for byte.
/// Nothing outside [row, row + stride) and the row's two words is read.
///
/// Returns -1, with nothing queued, where sgpu_frames_scan_dense does, for a
/// misaligned deviceStarts or deviceEnds and for an output of 4 GiB or more.
/// count == 0 returns a valid ticket that is already complete.
SIAMESE_EXPORT long long sgpu_frames_scan_streams(const void* deviceRows, size_t stride,
                                                  const unsigned* deviceStarts, const unsigned* deviceEnds,
                                                  unsigned count, unsigned maxFrames, unsigned maxRecords,
                                                  void* pinnedOut);
/// Host only: sgpu_frames_recv_dense for a stream scan's output, with the same
/// routing, results, *rowsOut and *acceptedOut and the same checks of info,
/// words, starts and records.  A word may carry SGPU_STREAM_PARTIAL, which is no
/// error and adds nothing to the return value; SGPU_PACKED_MALFORMED contributes
/// Siamese_InvalidInput after the row's good frames, as there.  For a row k < c,
/// next[k] <= stride and, when the row has records, next[k] >= the end of its
/// last record are checked before the row's records are touched: a next word
/// that fails stops the routing as a start that fails does.  consumedOut[k] =
/// next[k] for k < *rowsOut; the entries from *rowsOut on are left untouched
/// (scan those rows again from their old starts).  Arguments are refused as in
/// sgpu_frames_recv_dense, and a null consumedOut with count > 0.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_streams(const SgpuDecoder* decoders, unsigned decoderCount,
                                                      const void* heads, unsigned maxFrames, unsigned maxRecords,
                                                      const void* deviceRows, size_t stride, unsigned count,
                                                      SiameseResult* results /* maxRecords, optional */,
                                                      unsigned* consumedOut /* count, host */,
                                                      unsigned* rowsOut, unsigned* acceptedOut);
/// Queue a stream's frames packed into MTU-sized rows: the present originals
/// firstPacketNum .. firstPacketNum+originalCount-1 of `encoder`, ascending, as
/// SGPU_FRAME_ORIGINAL, then `recovery` (this encoder's current output) as
/// SGPU_FRAME_RECOVERY, all for `flow`.  Absent originals get results[k] =
/// Siamese_NeedMoreData and take no space.
///
/// The layout is decided here, by one rule: a cursor (row, off) starts at
/// (0, 0); a frame of T = header + data bytes that does not fit (off + T >
/// stride) moves to (row + 1, 0); the frame is placed at off and off becomes
/// align16(off + T).  So frames start on 16-byte boundaries with zeros between
/// them.  Rows [0, *rowsOut) are written whole (zero between the frames and to
/// the row's end), deviceLens[row] = the end of the row's last frame;
/// deviceLens[r] = 0 for r in [*rowsOut, maxRows) and those rows are left
/// untouched.  The buffer is a valid frame stream for sgpu_frames_parse /
/// sgpu_frames_recv and valid input for sgpu_frames_scan_packed.  *framesOut =
/// the frames queued.  Never waits; the rows and lengths are in place when the
/// call's submission has completed (the lifetime rule of the deliver calls).
///
/// Siamese_InvalidInput, with nothing queued: the deliver calls' pointer,
/// alignment and stride rules (deviceDst and deviceLens may be null only when
/// maxRows is 0); a null encoder, rowsOut or framesOut; null recovery with
/// recoveryCount > 0; flow > 2^24-1 (SGPU_FRAME_NONE included: bare packets
/// cannot be delimited); firstPacketNum > SIAMESE_PACKET_NUM_MAX; a frame with
/// T > stride; a recovery packet that is not this encoder's (or is empty);
/// more rows needed than maxRows, *rowsOut then saying how many were needed.
/// A disabled encoder returns Siamese_Disabled.
SIAMESE_EXPORT SiameseResult sgpu_encoder_pack_frames(SgpuEncoder encoder, unsigned flow, unsigned firstPacketNum,
                                                      unsigned originalCount, const SgpuRecoveryPacket* recovery,
                                                      unsigned recoveryCount, void* deviceDst, size_t stride,
                                                      unsigned maxRows, unsigned* deviceLens,
                                                      SiameseResult* results /* host, originalCount, optional */,
                                                      unsigned* rowsOut, unsigned* framesOut);
/// sgpu_encoder_pack_frames at a relay: the present packets firstPacketNum ..
/// firstPacketNum+count-1 of `decoder`, ascending, each as the
/// SGPU_FRAME_ORIGINAL frame sgpu_decoder_deliver_frames writes for it (header
/// from sgpu_frame_write_header for `flow` and (firstPacketNum + k) mod 2^22,
/// then the payload), laid out by the rule above.  The layout is made on the
/// device, from the lengths it reads there, so a packet whose solve is queued
/// in this same submission (sgpu_decode, sgpu_decode_device) is packed without
/// a wait and the host learns the row count only from deviceInfo.
///
/// An absent packet takes no space and gets results[k] = Siamese_NeedMoreData.
/// A present packet that does not fit, as sgpu_decoder_deliver_frames defines
/// it for a row of `stride` bytes (an unreadable or zero prefix, a length past
/// the symbol's capacity, T > stride, a frame length above 2^29 - 1), which
/// only the device can see while its length is pending, takes no space either.
///
/// With rows = the rows the layout needs: rows [0, min(rows, maxRows)) are
/// written whole (zero between the frames and to each row's end) and
/// deviceLens[r] = the end of row r's last frame; deviceLens[r] = 0 for the
/// other r < maxRows and those rows are left untouched.  deviceInfo[0] = rows
/// (it may exceed maxRows), [1] = the frames written, [2] = the present packets
/// skipped as not fitting, [3] = the frames not written because their row was
/// >= maxRows; nothing at or past row maxRows is touched.  The written rows are
/// a valid frame stream for sgpu_frames_parse / sgpu_frames_recv and valid
/// input for sgpu_frames_scan_packed; when the decoder holds exactly the
/// packets the sender holds they are, with the lengths, byte for byte what
/// sgpu_encoder_pack_frames(encoder, flow, firstPacketNum, count, NULL, 0, ...)
/// wrote there.  Never waits; everything is in place when the carrying
/// submission completes; the lifetime and overlap rules are
/// sgpu_decoder_deliver_frames', deviceInfo included.
///
/// Returns Siamese_Success with *queuedOut = the number of present packets.
/// Siamese_InvalidInput, with nothing queued: sgpu_decoder_deliver_frames'
/// pointer, alignment, stride, packet number and pending-matrix-job rules
/// (deviceDst and deviceLens may be null only when maxRows is 0); deviceInfo
/// null or not 16-byte aligned; flow > 2^24 - 1 (SGPU_FRAME_NONE included);
/// count > 65535; a packet whose length is already known and does not fit.  A
/// dead decoder returns Siamese_Disabled.  count == 0 returns Siamese_Success,
/// writes no row, zeroes the maxRows length words and writes a zero deviceInfo.
/// Recovery frames are not carried (a relay re-encodes: INTEGRATION).
SIAMESE_EXPORT SiameseResult sgpu_decoder_pack_frames(SgpuDecoder decoder, unsigned flow, unsigned firstPacketNum,
                                                      unsigned count, void* deviceDst, size_t stride, unsigned maxRows,
                                                      unsigned* deviceLens,
                                                      unsigned* deviceInfo /* 4 x uint32, device, 16-byte aligned */,
                                                      SiameseResult* results /* host, count, optional */,
                                                      unsigned* queuedOut);
/// The last leg of the receive path: the packets firstPacketNum ..
/// firstPacketNum+count-1 of `decoder` as the in-order byte stream the
/// application is owed, payloads back to back in deviceDst[0, capacity) with no
/// holes, no padding and no framing -- what sgpu_encoder_add_range(stride =
/// fixedBytes) segmented at the sender, reassembled.  deviceDst may have any
/// byte alignment: a receiver appends at its write cursor, buf + bytesSoFar.
/// The offsets are summed on the device, from the lengths it reads there, so a
/// packet whose solve is queued in this same submission (sgpu_decode,
/// sgpu_decode_device) is delivered without a wait.
///
/// Host side.  p = the leading present packets of the range, presence as in
/// sgpu_decoder_deliver_range (a packet whose solve is queued in this
/// submission counts).  results[k] = Siamese_Success for k < p and
/// Siamese_NeedMoreData for k >= p: the stream cannot reach a packet behind a
/// hole, whose length is unknown.  *queuedOut = p.
///
/// Device side.  Packet k < p has payload length n_k, valid as
/// sgpu_decoder_deliver_range judges it (a readable prefix, n >= 1, within the
/// symbol's capacity).  With off_0 = 0, packet k is delivered when every packet
/// before it was, it is valid and off_k + n_k <= capacity; then
/// deviceDst[off_k, off_k + n_k) is its payload and off_{k+1} = off_k + n_k.
/// Whole packets only.  With d packets delivered and B = off_d:
/// deviceOffsets[k] = off_k for k <= d and B for d < k <= count, so
/// deviceOffsets[k+1] - deviceOffsets[k] is always the delivered length of
/// packet k; deviceInfo = {d, B, stop, p} with stop 0 when d == p, 1 when
/// packet d is invalid (a corrupt recovered prefix: the decoder reports it as
/// it always does) and 2 when it is valid but does not fit capacity.  No byte
/// of deviceDst outside [0, B) is written, below deviceDst and at or past
/// deviceDst + B included: a word shared with bytes the caller already holds is
/// never read and rewritten.  Never waits; everything is in place when the
/// carrying submission completes; the launch runs after every other launch of
/// its submission; the lifetime and overlap rules are
/// sgpu_decoder_deliver_range's, deviceOffsets and deviceInfo included.
///
/// Siamese_InvalidInput, with nothing queued: a null decoder, queuedOut,
/// deviceOffsets or deviceInfo; deviceOffsets not 4-byte aligned; deviceInfo
/// not 16-byte aligned; null deviceDst with capacity > 0; capacity > 2^32 - 1;
/// count > 65535; firstPacketNum > SIAMESE_PACKET_NUM_MAX; a decoder with a
/// device matrix job pending.  A dead decoder returns Siamese_Disabled.
/// count == 0 returns Siamese_Success, writes deviceOffsets[0] = 0 and a zero
/// deviceInfo and copies nothing.  Lengths known on the host are not checked
/// against capacity: a full buffer is an ordinary stop (2), not an error, and
/// the next call appends from packet firstPacketNum + d.  Delivery past a hole,
/// framing inside the stream, a counterpart on the encoder or in the drop-in
/// ABI, and a capacity of 4 GiB or more are not offered.
SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_stream(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                         void* deviceDst, size_t capacity,
                                                         unsigned* deviceOffsets /* count + 1 uint32, device */,
                                                         unsigned* deviceInfo /* 4 x uint32, device, 16-byte aligned */,
                                                         SiameseResult* results /* host, count, optional */,
                                                         unsigned* queuedOut);

/*
    Closing the loop: the ARQ half of the codec for batch instances.  The
    receiver states what it still misses, the sender slides its window on
    that, learns a round-trip time, and resends what stays missing after its
    retransmission timeout.  The first five calls are siamese.h's, on batch
    instances; the others move acknowledgements and retransmissions through
    device rows like every other packet of this header.

    Threading and dead instances as for the other per-instance calls; none of
    these calls waits for the GPU.
*/
/// siamese_decoder_ack (siamese.h) on a batch decoder: the acknowledgement
/// message into buffer[0, byteLimit), *usedOut its bytes.  Siamese_InvalidInput
/// for a null argument, byteLimit < SIAMESE_ACK_MIN_BYTES, or a decoder with a
/// device matrix job pending; Siamese_NeedMoreData (*usedOut = 0) before the
/// first packet has arrived.
SIAMESE_EXPORT SiameseResult sgpu_decoder_ack(SgpuDecoder decoder, void* buffer, unsigned byteLimit,
                                              unsigned* usedOut);
/// siamese_encoder_ack on a batch encoder: takes a message sgpu_decoder_ack
/// wrote; *nextExpectedOut = the first packet the receiver still waits for.
/// The originals the message releases are recycled under the device pointer
/// lifetime rule above: after the submission that holds this call.
SIAMESE_EXPORT SiameseResult sgpu_encoder_acknowledge(SgpuEncoder encoder, const void* buffer, unsigned bytes,
                                                      unsigned* nextExpectedOut);
/// siamese_encoder_retransmit on a batch encoder: the next original whose
/// retransmission timeout has passed (Siamese_NeedMoreData: none now).
/// out->Data is a device pointer, under the device pointer lifetime rule.
SIAMESE_EXPORT SiameseResult sgpu_encoder_retransmit(SgpuEncoder encoder, SiameseOriginalPacket* out);
/// siamese_encoder_stats / siamese_decoder_stats on batch instances
/// (SiameseEncoderStats_* / SiameseDecoderStats_* indices).
SIAMESE_EXPORT SiameseResult sgpu_encoder_stats(SgpuEncoder encoder, uint64_t* statsOut, unsigned statsCount);
SIAMESE_EXPORT SiameseResult sgpu_decoder_stats(SgpuDecoder decoder, uint64_t* statsOut, unsigned statsCount);

/// Host helper: the SGPU_FRAME_ACK frame for `flow` around msg[0, bytes) into
/// out[0, capacity).  Returns the frame's bytes; 0 for a null pointer, an empty
/// message, a flow above 2^24-1, a message whose L no prefix can state, or a
/// frame longer than capacity.
SIAMESE_EXPORT unsigned sgpu_frame_write_ack(unsigned flow, const void* msg, unsigned bytes, void* out,
                                             unsigned capacity);

/// Acks out: queue decoder k's acknowledgement (sgpu_decoder_ack with
/// byteLimit) as an SGPU_FRAME_ACK frame for flows[k] into row k of
/// caller-owned device rows.  The message is made here, on the host, and rides
/// in the submission's upload; k_frame places it.  The row contract is the
/// deliver calls': row k = what sgpu_frame_write_ack(flows[k], message) writes,
/// then zeros to the row's end, deviceLens[k] = the frame's bytes, in place when
/// the carrying submission completes; the call never waits.  A decoder that
/// answers Siamese_NeedMoreData (nothing received yet) gets results[k] =
/// NeedMoreData, deviceLens[k] = 0 and an untouched row; so does a dead one,
/// with results[k] = Siamese_Disabled, which the call then returns.  Otherwise
/// the call returns Siamese_Success, *queuedOut = the frames queued.
/// Siamese_InvalidInput, with nothing queued: the deliver calls' pointer,
/// alignment and stride rules; null decoders or flows with count > 0; a null
/// decoder or one with a device matrix job pending; a flow above 2^24-1;
/// byteLimit < SIAMESE_ACK_MIN_BYTES; a frame of byteLimit message bytes longer
/// than stride.
SIAMESE_EXPORT SiameseResult sgpu_decoders_ack_frames(const SgpuDecoder* decoders, unsigned count,
                                                      const unsigned* flows, unsigned byteLimit, void* deviceDst,
                                                      size_t stride, unsigned* deviceLens,
                                                      SiameseResult* results /* host, optional */,
                                                      unsigned* queuedOut);
/// Retransmits out: sgpu_encoder_retransmit until it answers
/// Siamese_NeedMoreData or maxPackets packets were returned, each queued as an
/// SGPU_FRAME_ORIGINAL frame for `flow`, packed into MTU-sized rows by
/// sgpu_encoder_pack_frames' cursor rule with its zero fill and its length
/// words (deviceLens[r] = 0 and an untouched row for r in [*rowsOut, maxRows)).
/// packetNumsOut[i] (host, optional, maxPackets entries) = frame i's PacketNum;
/// *framesOut = the frames queued.  The written rows are valid input for
/// sgpu_frames_parse and sgpu_frames_scan_packed.
///
/// A retransmission restarts its packet's timer, so none is consumed that
/// cannot be placed: before each one, a frame of the longest original of the
/// unacknowledged window must still fit the rows that are left; if not, the
/// call stops and returns Siamese_Success with what it has (call again with
/// more rows for the rest).  If such a frame does not fit `stride` at all:
/// Siamese_InvalidInput, nothing consumed.  Also Siamese_InvalidInput, with
/// nothing queued: sgpu_encoder_pack_frames' pointer, alignment, stride and
/// flow rules; a null encoder, rowsOut or framesOut.  A disabled encoder
/// returns Siamese_Disabled.
SIAMESE_EXPORT SiameseResult sgpu_encoder_retransmit_frames(SgpuEncoder encoder, unsigned flow, unsigned maxPackets,
                                                            void* deviceDst, size_t stride, unsigned maxRows,
                                                            unsigned* deviceLens,
                                                            unsigned* packetNumsOut /* host, optional */,
                                                            unsigned* rowsOut, unsigned* framesOut);

/*
    Acks (and everything else) in: datagram rows of a bidirectional flow mix
    originals, recovery packets and acks.  The duplex scan is the packed scan
    with ack frames accepted, and the whole message of each in a slot:

        bytes  = sgpu_frames_duplex_bytes(count, maxFrames, ackSlots, ackBytes);   // pinned
        ticket = sgpu_frames_scan_duplex(rows, stride, lens, count, maxFrames, ackSlots, ackBytes, out);
        sgpu_gather_wait(ticket);
        sgpu_frames_recv_duplex(decoders, nd, encoders, ne, out, maxFrames, ackSlots, ackBytes, rows, stride,
                                count, results, nextExpected, &accepted);

    out is sgpu_frames_scan_packed's output unchanged (count * maxFrames
    SgpuPackedHead records, then count row words) and then, from the next
    16-byte boundary on (sgpu_frames_duplex_slots(count, maxFrames) bytes into
    out), count * ackSlots message slots of ackBytes bytes, row k's at slot
    index k * ackSlots.  ackBytes is a multiple of 16 in 16..1024, ackSlots in
    1..maxFrames.

    The row's a-th ack frame (a from 0), of D message bytes, has a record with
    Type = SGPU_FRAME_ACK, PacketNum = a, DataBytes = D, HeaderBytes = its
    prefix + 4, and zero TailBytes, Head and Tail.  When a < ackSlots, slot a
    holds the message's first min(D, ackBytes) bytes and zeros after them.  Its
    Status is SGPU_ROW_OK when it has a slot that holds the whole message;
    otherwise (D > ackBytes, or a >= ackSlots) it is SGPU_ROW_TRUNCATED and the
    row word carries SGPU_PACKED_ACKS_DROPPED.  Either way the walk goes on, so
    the data frames behind the ack are kept.  Slots without an ack are zero.
*/
#define SGPU_ROW_TRUNCATED       3            /* an ack record whose message is not (whole) in a slot */
#define SGPU_PACKED_ACKS_DROPPED 0x20000000u  /* the row has an SGPU_ROW_TRUNCATED record */

/// Bytes of a duplex scan's output (0 for arguments sgpu_frames_scan_duplex refuses).
SIAMESE_EXPORT size_t sgpu_frames_duplex_bytes(unsigned count, unsigned maxFrames, unsigned ackSlots,
                                               unsigned ackBytes);
/// Byte offset of the first message slot in a duplex scan's output.
SIAMESE_EXPORT size_t sgpu_frames_duplex_slots(unsigned count, unsigned maxFrames);
/// sgpu_frames_scan_packed for rows that may hold ack frames (one k_ackwalk
/// launch): the same contract, tickets, arguments and deviceLens rules (the
/// empty row, the row longer than stride, the end of the walk), the same walk
/// with type 2 accepted when L > 4, and records for originals and recovery
/// frames that are byte for byte the packed scan's.  Every record, every row
/// word and every slot is written by every scan; nothing outside
/// [row, row + stride) and the row's length word is read.  Returns -1 also for
/// ackSlots outside 1..maxFrames and ackBytes not a multiple of 16 in 16..1024.
SIAMESE_EXPORT long long sgpu_frames_scan_duplex(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                 unsigned count, unsigned maxFrames, unsigned ackSlots,
                                                 unsigned ackBytes, void* pinnedOut);
/// Host only: sgpu_frames_recv_packed for a duplex scan's output.  Originals
/// and recovery frames go to decoders[Flow] exactly as there; an ack record
/// with Status SGPU_ROW_OK goes to sgpu_encoder_acknowledge(encoders[Flow], its
/// slot, DataBytes), the answer's next expected packet into
/// nextExpectedOut[k * maxFrames + j] (optional, count * maxFrames entries;
/// other entries are left alone).  results as in sgpu_frames_recv_packed.
/// Siamese_InvalidInput for: a truncated ack (it is never handed to an
/// encoder: cut short, a message states a different loss list); a flow without
/// an encoder; an ack record the scan could not have produced (PacketNum not
/// the number of ack records before it in its row, DataBytes or the frame
/// outside its bounds, a Status that disagrees with its slot).  The records,
/// words and slots are caller data and never trusted: each is copied and
/// checked before use.  *acceptedOut = the frames handed to a decoder or an
/// encoder.  decoders (encoders) may be null when decoderCount (encoderCount)
/// is 0; otherwise arguments are refused as in sgpu_frames_recv_packed and as
/// in the scan.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex(const SgpuDecoder* decoders, unsigned decoderCount,
                                                     const SgpuEncoder* encoders, unsigned encoderCount,
                                                     const void* heads, unsigned maxFrames, unsigned ackSlots,
                                                     unsigned ackBytes, const void* deviceRows, size_t stride,
                                                     unsigned count,
                                                     SiameseResult* results /* count*maxFrames, optional */,
                                                     unsigned* nextExpectedOut /* count*maxFrames, optional */,
                                                     unsigned* acceptedOut);
/*
    The duplex scan in dense form.  sgpu_frames_scan_duplex ships count *
    maxFrames records and count * ackSlots slots whatever the rows hold, and
    acknowledgements are rare.  The dense duplex scan runs the same walk under
    the same per-frame and per-ack rules and puts the accepted records of all
    rows back to back, as sgpu_frames_scan_dense does, and the used slots of all
    rows back to back behind a second table:

        bytes  = sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes);   // pinned
        ticket = sgpu_frames_scan_duplex_dense(rows, stride, lens, count, maxFrames, ackSlots, ackBytes,
                                               maxRecords, maxAcks, out);
        sgpu_gather_wait(ticket);
        sgpu_frames_recv_duplex_dense(decoders, nd, encoders, ne, out, maxFrames, ackSlots, ackBytes,
                                      maxRecords, maxAcks, rows, stride, count, results, nextExpected,
                                      &rowsDone, &accepted);
        // rowsDone < count: scan again from row rowsDone

    out holds, little-endian and in this order:
      - info, four uint32 {T, W, c, WA};
      - count row words, word k exactly what sgpu_frames_scan_duplex writes for
        row k with the same maxFrames, ackSlots and ackBytes;
      - count + 1 start words: start[0] = 0, start[k+1] = start[k] +
        SGPU_PACKED_COUNT(word k), T = start[count];
      - zeros up to sgpu_frames_dense_records(count);
      - maxRecords SgpuPackedHead records;
      - count + 1 ack start words, from sgpu_frames_duplex_dense_acks(count,
        maxRecords): astart[0] = 0, astart[k+1] = astart[k] + min(ack frames of
        row k, ackSlots);
      - zeros up to the next 16-byte boundary, sgpu_frames_duplex_dense_slots(
        count, maxRecords);
      - maxAcks slots of ackBytes bytes.
    Up to the end of the records this is sgpu_frames_scan_dense's layout with
    info word 3 = WA.  Rows are all or nothing over both budgets: c is the
    largest value with start[c] <= maxRecords and astart[c] <= maxAcks, W =
    start[c] and WA = astart[c].  Records [start[k], start[k+1]) for k < c are
    byte for byte the first records the duplex scan writes for row k (Offset
    relative to that row, PacketNum = the ack's number within its row, Status
    SGPU_ROW_TRUNCATED under the same per-row ackSlots and ackBytes rule); slot
    astart[k] + a, for k < c and a < min(acks of row k, ackSlots), is byte for
    byte row k's slot a of the duplex scan.  An ack with a >= ackSlots has a
    record and no slot.  Records from W on and slots from WA on are zero.  Every
    byte is written by every scan.  maxRecords >= maxFrames and maxAcks >=
    ackSlots, so a scan of at least one row completes at least one row.
*/
/// Bytes of a dense duplex scan's output (0 for a maxRecords or maxAcks of 0 or
/// above count * 256, an ackBytes the duplex scan refuses, or 4 GiB or more).
SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_bytes(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                     unsigned ackBytes);
/// Byte offset of astart[0] in a dense duplex scan's output (0 where
/// sgpu_frames_dense_bytes(count, maxRecords) is).
SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_acks(unsigned count, unsigned maxRecords);
/// Byte offset of slot 0 in a dense duplex scan's output (0 likewise).
SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_slots(unsigned count, unsigned maxRecords);
/// sgpu_frames_scan_duplex into the dense layout above (pinnedOut: pinned,
/// 16-byte aligned, sgpu_frames_duplex_dense_bytes), with four kernel launches
/// and one copy: the gather ticket, sgpu_gather_wait, what may be read, what
/// later submissions wait for and the threading rule are sgpu_frames_scan_dense's.
/// Returns -1, with nothing queued, where sgpu_frames_scan_duplex does, for
/// maxRecords < maxFrames, maxRecords > count * maxFrames, maxAcks < ackSlots,
/// maxAcks > count * ackSlots or an output of 4 GiB or more.  count == 0 returns
/// a valid ticket that is already complete, and nothing is written.
SIAMESE_EXPORT long long sgpu_frames_scan_duplex_dense(const void* deviceRows, size_t stride,
                                                       const unsigned* deviceLens, unsigned count,
                                                       unsigned maxFrames, unsigned ackSlots, unsigned ackBytes,
                                                       unsigned maxRecords, unsigned maxAcks, void* pinnedOut);
/// Host only: sgpu_frames_recv_duplex for a dense duplex scan's output (`heads`,
/// 4-byte aligned).  The records of rows [0, c) are routed in order and exactly
/// as sgpu_frames_recv_duplex routes them: data frames to decoders[Flow], an
/// SGPU_ROW_OK ack from its slot to sgpu_encoder_acknowledge(encoders[Flow]);
/// a truncated ack and a flow without an instance give Siamese_InvalidInput.
/// results[i] and nextExpectedOut[i] (optional, maxRecords entries each) belong
/// to record i; results are Siamese_NeedMoreData for slots from W on.  *rowsOut
/// = c, the rows routed: when it is below count, scan again from that row.
/// *acceptedOut = the frames handed to a decoder or an encoder.  The output is
/// caller data and never trusted: info and every table word are copied; c <=
/// count, W <= maxRecords, WA <= maxAcks, start[0] == astart[0] == 0,
/// non-decreasing starts with start[k+1] - start[k] == min(SGPU_PACKED_COUNT(
/// word k), maxFrames), non-decreasing ack starts with astart[k+1] - astart[k]
/// == the ack records of row k with PacketNum < ackSlots, start[c] == W and
/// astart[c] == WA are checked before a row's records are routed, each record is
/// copied and checked as sgpu_frames_recv_duplex checks one, and no slot outside
/// the row's own [astart[k], astart[k+1]) is read.  At the first start of either
/// table that fails, routing stops, *rowsOut = the rows routed before it and the
/// call returns Siamese_InvalidInput; a record that fails, or a word whose count
/// exceeds maxFrames, counts as malformed.  Arguments are refused as in
/// sgpu_frames_recv_duplex, for a null rowsOut and for the sizes the scan
/// refuses.  For well-formed rows the decoders and encoders end in the state
/// sgpu_frames_recv_duplex leaves them in on the same rows.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex_dense(const SgpuDecoder* decoders, unsigned decoderCount,
                                                           const SgpuEncoder* encoders, unsigned encoderCount,
                                                           const void* heads, unsigned maxFrames, unsigned ackSlots,
                                                           unsigned ackBytes, unsigned maxRecords, unsigned maxAcks,
                                                           const void* deviceRows, size_t stride, unsigned count,
                                                           SiameseResult* results /* maxRecords, optional */,
                                                           unsigned* nextExpectedOut /* maxRecords, optional */,
                                                           unsigned* rowsOut, unsigned* acceptedOut);
/*
    Duplex rows that are byte streams.  A stream transport is bidirectional, and
    ARQ runs over it: a connection's receive buffer in device memory holds the
    peer's data frames and its acknowledgements back to back, and the last frame
    is usually still arriving.  The duplex stream scan is the dense duplex scan
    over row bytes [start, end), with sgpu_frames_scan_streams' partial frame and
    next words:

        bytes  = sgpu_frames_duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes);   // pinned
        for (;;) {
            // the transport has advanced ends[k]; starts[k] is where row k's last scan stopped
            ticket = sgpu_frames_scan_duplex_streams(rows, stride, starts, ends, count, maxFrames, ackSlots,
                                                     ackBytes, maxRecords, maxAcks, out);
            sgpu_gather_wait(ticket);
            sgpu_frames_recv_duplex_streams(decoders, nd, encoders, ne, out, maxFrames, ackSlots, ackBytes,
                                            maxRecords, maxAcks, rows, stride, count, results, nextExpected,
                                            consumed, &rowsDone, &accepted);
            // consumed[k], k < rowsDone, is row k's next start: write it back to starts[k]
            // (rows from rowsDone on keep their old starts and are scanned again);
            // answer with sgpu_decoders_ack_frames and sgpu_encoder_retransmit_frames as in the datagram loop
        }

    out holds sgpu_frames_scan_duplex_dense's layout, all
    sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes) bytes of
    it -- info {T, W, c, WA}, both start tables, records and slots, rows all or
    nothing over both budgets -- and then, at sgpu_frames_duplex_streams_next(...),
    count uint32 next words and zeros up to the next 16-byte boundary.  Every byte
    is written by every scan.  A record's Offset is relative to the row's first
    byte, not to start.  A row word may carry SGPU_STREAM_PARTIAL_DUPLEX, which
    has a bit of its own: SGPU_STREAM_PARTIAL shares SGPU_PACKED_ACKS_DROPPED's
    bit and keeps its value and meaning in sgpu_frames_scan_streams, and a duplex
    stream row can drop an ack and stop at a partial frame in one scan.  Acks
    are numbered within the scan: the row's a-th ack of this scan has PacketNum
    a and slot a.  An ack dropped for lack of a slot (SGPU_ROW_TRUNCATED) lies
    behind the row's next word and is not seen again by the next scan; a caller
    that wants it scans the row again from that record's Offset with more slots.
    Still not offered: a ring that wraps around inside a row, more than 256
    frames per row and scan (resume from the next word), and a walk that stops
    at an ack without a slot.
*/
#define SGPU_STREAM_PARTIAL_DUPLEX 0x10000000u  /* row word of a duplex stream scan: stopped at a frame not yet whole */

/// Bytes of a duplex stream scan's output (0 where sgpu_frames_duplex_dense_bytes is 0).
SIAMESE_EXPORT size_t sgpu_frames_duplex_streams_bytes(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                       unsigned ackBytes);
/// Byte offset of the next words in a duplex stream scan's output:
/// sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes).
SIAMESE_EXPORT size_t sgpu_frames_duplex_streams_next(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                      unsigned ackBytes);
/// Scan `count` duplex byte-stream rows into pinnedOut (pinned, 16-byte aligned,
/// sgpu_frames_duplex_streams_bytes): a gather with
/// sgpu_frames_scan_duplex_dense's ticket, ordering and lifetime contract, its
/// rows, stride, maxFrames, ackSlots, ackBytes, maxRecords and maxAcks.
///
/// Row k is walked over its bytes [start, end), start = deviceStarts ?
/// deviceStarts[k] : 0 and end = deviceEnds ? deviceEnds[k] : stride (uint32
/// arrays in device memory, 4-byte aligned; byte offsets from the row's first
/// byte, at any alignment), as sgpu_frames_scan_duplex walks a row from 0: zero
/// bytes where a frame would start are skipped, and a frame of type 0, 1 or 2 is
/// accepted under that scan's rules.  The row's a-th ack, counted within this
/// scan, has PacketNum a; slot a receives the first min(D, ackBytes) bytes of
/// its message; with a >= ackSlots or D > ackBytes its Status is
/// SGPU_ROW_TRUNCATED, the word gets SGPU_PACKED_ACKS_DROPPED and the walk goes
/// on behind it.  Row word k and next word k say how the walk ended:
///   - start > end or end > stride: SGPU_PACKED_MALFORMED, no records, no acks,
///     next = min(start, stride);
///   - only zero bytes were left: the count n, next = end;
///   - n == maxFrames and a non-zero byte is left: n | SGPU_PACKED_MORE, next =
///     that byte's offset;
///   - a partial frame at `at`: n | SGPU_STREAM_PARTIAL_DUPLEX, next = at.  With
///     left = end - at, the frame is partial when its first byte announces a
///     prefix of w bytes and left < w, or the prefix gives L >= 1 and w + L >
///     left, and nothing that is present is wrong already.  A partial ack
///     writes no slot, gets no record and does not count as one of the row's
///     acks;
///   - a frame at `at` that is whole and fails a rule (L == 0 included), or that
///     is cut off and can never become valid -- w + L > stride, a type byte that
///     is present and above 2, a type byte that is present with L not above the
///     type's inner header (7, 4, 4), an original whose three PacketNum bytes are
///     present and exceed SIAMESE_PACKET_NUM_MAX -- : n | SGPU_PACKED_MALFORMED,
///     next = at.
/// A word may carry SGPU_PACKED_ACKS_DROPPED together with any one of the three
/// stop flags.  Next word k is written for every row, also for k >= c.  (With a
/// null deviceEnds and a stride of 4 GiB, next = end is stated as 2^32 - 1.)
/// With start 0 and no partial frame the first sgpu_frames_duplex_dense_bytes
/// bytes are sgpu_frames_scan_duplex_dense's on the same rows with lens = ends
/// and the same sizes, byte for byte.  Nothing outside [row, row + stride) and
/// the row's two words is read, and the bytes before start and from end on --
/// stale ring content -- influence no output bit.
///
/// Returns -1, with nothing queued, where sgpu_frames_scan_duplex_dense does, for
/// a misaligned deviceStarts or deviceEnds and for an output of 4 GiB or more.
/// count == 0 returns a valid ticket that is already complete, and nothing is
/// written.
SIAMESE_EXPORT long long sgpu_frames_scan_duplex_streams(const void* deviceRows, size_t stride,
                                                         const unsigned* deviceStarts, const unsigned* deviceEnds,
                                                         unsigned count, unsigned maxFrames, unsigned ackSlots,
                                                         unsigned ackBytes, unsigned maxRecords, unsigned maxAcks,
                                                         void* pinnedOut);
/// Host only: sgpu_frames_recv_duplex_dense for a duplex stream scan's output,
/// with the same routing, results, nextExpectedOut, *rowsOut and *acceptedOut
/// and the same copies and checks of info, words, both start tables, records and
/// slots.  A word may carry SGPU_STREAM_PARTIAL_DUPLEX, which is no error and
/// adds nothing to the return value; SGPU_PACKED_MALFORMED contributes
/// Siamese_InvalidInput after the row's good frames, as there.  For a row k < c,
/// next[k] <= stride and, when the row has records, next[k] >= the end of its
/// last record are checked before any of the row's records are routed: a next
/// word that fails stops the routing as a start that fails does.  consumedOut[k]
/// = next[k] for k < *rowsOut; the entries from *rowsOut on are left untouched
/// (scan those rows again from their old starts).  Arguments are refused as in
/// sgpu_frames_recv_duplex_dense, and a null consumedOut with count > 0.
SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex_streams(const SgpuDecoder* decoders, unsigned decoderCount,
                                                             const SgpuEncoder* encoders, unsigned encoderCount,
                                                             const void* heads, unsigned maxFrames,
                                                             unsigned ackSlots, unsigned ackBytes,
                                                             unsigned maxRecords, unsigned maxAcks,
                                                             const void* deviceRows, size_t stride, unsigned count,
                                                             SiameseResult* results /* maxRecords, optional */,
                                                             unsigned* nextExpectedOut /* maxRecords, optional */,
                                                             unsigned* consumedOut /* count, host */,
                                                             unsigned* rowsOut, unsigned* acceptedOut);

/// Device timing of flushed work since the last reset (milliseconds).
SIAMESE_EXPORT void sgpu_timing(int enable, int reset, double* execMs, double* totalMs);
/// Device milliseconds per kernel class since the last sgpu_timing reset,
/// while timing is enabled: [0] k_ingest, [1] k_exec, [2] k_ldpc, [3] the
/// solve kernels (k_solve_pre + k_solve_tr + k_solve_main on launches of
/// >= 16 solves, k_solve_main alone below that), [4] k_ge (sgpu_decode_device),
/// [5] k_deliver (sgpu_decoder_deliver_range), [6] k_frame
/// (sgpu_frames_deliver_recovery, sgpu_encoder_deliver_range), [7] k_scan
/// (sgpu_frames_scan_rows: launched on the gather stream, counted once its
/// gather has been waited for), [8] k_walk (sgpu_frames_scan_packed,
/// likewise), [9] k_relay (sgpu_decoder_deliver_frames), [10] k_plan and [11]
/// k_pack (sgpu_decoder_pack_frames), [12] k_ackwalk (sgpu_frames_scan_duplex,
/// counted as k_walk is), [13] k_offsets and [14] k_concat
/// (sgpu_decoder_deliver_stream), [15] k_rowsum and [16] k_compact
/// (sgpu_frames_scan_dense, counted as k_walk is; the dense scan's walk is
/// counted under [8]), [17] k_rowsum2 and [18] k_slots
/// (sgpu_frames_scan_duplex_dense, likewise; its walk is counted under [12] and
/// its record copy under [16]), [19] k_streamwalk (sgpu_frames_scan_streams,
/// likewise; its k_rowsum and k_compact are counted under [15] and [16]), [20]
/// k_ackstreamwalk (sgpu_frames_scan_duplex_streams, likewise; its k_rowsum2,
/// k_compact and k_slots are counted under [17], [16] and [18]); count entries
/// at most.
SIAMESE_EXPORT void sgpu_timing_kernels(double* msOut, unsigned count);
/// Engine counters (15 values): flushes, launches, ops, terms, solves,
/// ingests, upload bytes, algorithmic op bytes, algorithmic output bytes,
/// the part of the algorithmic bytes handled by the solve kernels, then host
/// nanoseconds spent assembling flushes, waiting for the device,
/// running completions, and reclaiming released buffers, then the number of
/// executor launches.
SIAMESE_EXPORT void sgpu_engine_stats(uint64_t* out15);
/// sgpu_engine_stats' 15 values, then the algorithmic bytes of k_ldpc (the
/// wide rows' picks, part of the algorithmic op bytes), then the executor
/// launches' compulsory bytes (see sgpu_measure_unique), then the device
/// recovery-matrix jobs (sgpu_decode_device), those of them chained into
/// their decode's submission, and the chained ones whose matrix was singular
/// (the host repeated the elimination), then the chained jobs whose decode
/// carried gated wide-row picks (k_ldpc items), then [21] the delivery items
/// queued (sgpu_decoder_deliver_range: one per packet of each range, absent
/// ones included, counted when their submission is laid out), then [22] the
/// frame items queued likewise (sgpu_frames_deliver_recovery,
/// sgpu_encoder_deliver_range), then [23] the rows scanned
/// (sgpu_frames_scan_rows, counted when the scan is queued), then [24] the
/// rows scanned by sgpu_frames_scan_packed, counted likewise, then [25] the
/// relay items queued (sgpu_decoder_deliver_frames: counted as [21]), then
/// [26] the pack items queued (sgpu_decoder_pack_frames: one per packet of the
/// range, absent ones included), then [27] the rows scanned by
/// sgpu_frames_scan_duplex, counted as [24], then [28] the ack frames queued
/// (sgpu_decoders_ack_frames, counted by the call), then [29] the stream items
/// queued (sgpu_decoder_deliver_stream: one per packet of the range's leading
/// present run, counted as [26]), then the Siamese row batches by the executor
/// mode their shape selects, counted when their submission is laid out: [30]
/// the batches, [31] those in which a row reads a lane sum that a later row's
/// originals were folded into (versioned batches: rows made one after another
/// while originals are added), [32] the rows of those, [33] the batches whose
/// descriptors exceed the executor's on-chip table, [34] the batches whose
/// window exceeds the executor's on-chip stage, and [35] a constant: the
/// window elements that stage holds on this device (0: no stage; [34] then
/// stays 0), then [36] the rows scanned by sgpu_frames_scan_dense, counted as
/// [24], then [37] the recovery-matrix eliminations that met a zero pivot and
/// went on with row pivoting, on the host or in a device job (its pivot order
/// is not the identity, or it stopped short of the last column), counted when
/// the elimination's outcome is known -- a singular device job counts here
/// once, and the host's repeat of its elimination, which pivots again, once
/// more -- and [38] the device jobs, chained or not, that came back singular,
/// then [39] the rows scanned by sgpu_frames_scan_duplex_dense, counted as [36],
/// then, counted when a solve's submission has completed, [40] the solves
/// whose product (X = T R) had non-zero bytes past a recovered length, so that
/// the exact sweeps redid them (inconsistent recovery data; always 0 where no
/// product solve runs), and [41] the solves that stopped at an invalid
/// recovered length prefix (the decoder is disabled, as the reference's), then
/// [42] the rows scanned by sgpu_frames_scan_streams, counted as [36], then [43]
/// the rows scanned by sgpu_frames_scan_duplex_streams, likewise; count entries
/// at most.
SIAMESE_EXPORT void sgpu_engine_stats_ex(uint64_t* out, unsigned count);
/// Measurement aid: while on, flush assembly counts the executor launches'
/// compulsory bytes -- each distinct source symbol read once, each
/// destination written once, the op stream once -- into sgpu_engine_stats_ex
/// [16].  The algorithmic bytes count every re-read of a symbol the reference
/// performs; this is the traffic a kernel that re-reads nothing from HBM
/// would move.  Off by default (it sorts every segment's operands).
SIAMESE_EXPORT void sgpu_measure_unique(int on);

/// Device bytes the engine's symbol arena has taken from hipMalloc so far
/// (grows while warming up, then stays flat: buffers are recycled).
SIAMESE_EXPORT uint64_t sgpu_arena_bytes(void);
/// Keep at least `bytes` of untouched arena memory in reserve (allocated now,
/// counted in sgpu_arena_bytes), so later growth of the working set takes it
/// instead of calling hipMalloc inside a latency-sensitive phase.
SIAMESE_EXPORT int sgpu_arena_reserve(size_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* SIAMESE_GPU_H */
