// frames.h -- framed datagrams: the wire format the batch API's packet
// ingest and egress use (include/siamese_gpu.h, "Framed datagrams").
//
// A frame carries one datagram:
//   [L: length of the rest, the symbol length prefix format
//       (reference SiameseSerializers.h:566-593), 1-4 bytes]
//   [type: 1 byte]  kFrameOriginal / kFrameRecovery / kFrameAck
//   [flow: 3 bytes little-endian]  the application's stream id
//   original:  [PacketNum: 3 bytes LE (22 bits)] [payload]
//   recovery:  [the recovery packet: payload + its metadata footer
//               (reference SiameseSerializers.h:736-800)]
//   ack:       [the acknowledgement message, exactly as the decoder wrote it
//               (reference SiameseDecoder.cpp:125-255): at least one byte, so
//               L >= 5, and no upper bound but the frame format's]
// Only the duplex scan (ack_walk below) accepts an ack frame; frames_parse,
// row_head_scan and row_walk call type 2 malformed.
// Frames follow each other directly; a zero byte where a frame would start
// is an empty frame (L = 0) and is skipped, so senders may pad frames to
// any alignment with zeros (the egress gather places each frame at a 16-byte
// boundary).
#pragma once

#include "codedef.h"
#include "ops.h"
#include "../../include/siamese.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sgpu {

constexpr uint8_t kFrameOriginal = 0;
constexpr uint8_t kFrameRecovery = 1;
constexpr uint8_t kFrameAck = 2;
constexpr unsigned kFrameFlowBytes = 3;
constexpr unsigned kFrameMaxFlow = (1u << 24) - 1;
/// Bytes between a frame's length prefix and its data.
constexpr unsigned kFrameOriginalInner = 1 + kFrameFlowBytes + 3;   // type, flow, PacketNum
constexpr unsigned kFrameRecoveryInner = 1 + kFrameFlowBytes;       // type, flow
constexpr unsigned kFrameAckInner = 1 + kFrameFlowBytes;            // type, flow

/// One parsed frame: byte offsets into the buffer it was parsed from.
struct FrameInfo
{
    uint32_t type;
    uint32_t flow;
    uint32_t packetNum;   // originals
    uint32_t offset;      // first data byte (payload, or the recovery packet)
    uint32_t bytes;       // data bytes
};

/// Header bytes before the data of a frame of `type` holding `dataBytes`.
/// (This and frame_write_header are defined here: relay_row is built from
/// them, and the test double is also built without frames.cpp.)
inline unsigned frame_header_bytes(unsigned type, unsigned dataBytes)
{
    const unsigned inner = type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
    const unsigned length = inner + dataBytes;
    return (length < 0x80 ? 1 : length < 0x4000 ? 2 : length < 0x200000 ? 3 : 4) + inner;
}
/// Writes the header; returns its size (frame_header_bytes).
inline unsigned frame_write_header(unsigned type, unsigned flow, unsigned packetNum, unsigned dataBytes, uint8_t* out)
{
    const unsigned inner = type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
    unsigned n = write_length_prefix(inner + dataBytes, out);
    out[n++] = (uint8_t)type;
    out[n++] = (uint8_t)flow;
    out[n++] = (uint8_t)(flow >> 8);
    out[n++] = (uint8_t)(flow >> 16);
    if (type == kFrameOriginal) {
        out[n++] = (uint8_t)packetNum;
        out[n++] = (uint8_t)(packetNum >> 8);
        out[n++] = (uint8_t)(packetNum >> 16);
    }
    return n;
}
/// The header of an ack frame for `flow` whose message has `bytes` bytes (1 ..
/// kFrameMaxLength - 4), at most 8 bytes: returns its size.
inline unsigned frame_write_ack_header(unsigned flow, unsigned bytes, uint8_t* out)
{
    unsigned n = write_length_prefix(kFrameAckInner + bytes, out);
    out[n++] = kFrameAck;
    out[n++] = (uint8_t)flow;
    out[n++] = (uint8_t)(flow >> 8);
    out[n++] = (uint8_t)(flow >> 16);
    return n;
}
/// An ack frame for `flow` around msg[0, bytes) into out[0, capacity): returns
/// the frame's bytes, 0 when there is no message, the flow has more than three
/// bytes, L cannot be stated or the frame does not fit.
inline unsigned frame_write_ack(unsigned flow, const uint8_t* msg, unsigned bytes, uint8_t* out, size_t capacity)
{
    if (!msg || !out || bytes < 1 || flow > kFrameMaxFlow || bytes > kFrameMaxLength - kFrameAckInner)
        return 0;
    if ((uint64_t)frame_header_bytes(kFrameAck, bytes) + bytes > capacity)
        return 0;
    const unsigned n = frame_write_ack_header(flow, bytes, out);
    std::memcpy(out + n, msg, bytes);
    return n + bytes;
}
/// No malformed frame was met (frames_parse's *badOffset).
constexpr size_t kNoBadFrame = ~(size_t)0;
/// Parses frames from buf[0, bytes) (bytes < 4 GiB: offsets are 32-bit).
/// Returns the number of frames written to out (at most maxFrames).  Stops
/// at a malformed frame with *badOffset = where it starts (kNoBadFrame
/// otherwise): the frames before it are in out and *consumed = *badOffset.
/// Stops early (returning maxFrames) when out is full: *consumed says how far.
long frames_parse(const uint8_t* buf, size_t bytes, FrameInfo* out, size_t maxFrames, size_t* consumed,
                  size_t* badOffset);

/// Frame rows in device memory (ops.h RowHead, sgpu_frames_scan_rows /
/// sgpu_frames_recv_rows).  The one definition of a record that may be acted
/// on, for a row of `stride` bytes: status kRowOk; a type the format has; at
/// least one data byte (L > the type's inner header) and at most
/// SIAMESE_MAX_PACKET_BYTES; a header of the type's inner bytes plus a 1-4
/// byte prefix; header + data within the stride and within frameBytes; a flow
/// of three bytes; an original's PacketNum <= SIAMESE_PACKET_NUM_MAX;
/// tailBytes = min(8, dataBytes) for a recovery packet, 0 for an original.
/// sgpu_frames_recv_rows trusts no record that fails it, and row_head_scan
/// (so the test double of k_scan) reports such a row malformed.  (Defined
/// here: the test double is also built without frames.cpp.)
inline bool row_head_valid(const RowHead& r, uint64_t stride)
{
    if (r.status != kRowOk || r.type > kFrameRecovery)
        return false;
    const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
    if (r.dataBytes < 1 || r.dataBytes > SIAMESE_MAX_PACKET_BYTES)
        return false;
    if (r.headerBytes < inner + 1 || r.headerBytes > inner + 4)
        return false;
    const uint64_t end = (uint64_t)r.headerBytes + r.dataBytes;
    if (end > stride || end > r.frameBytes)
        return false;
    if (r.flow > kFrameMaxFlow)
        return false;
    if (r.type == kFrameOriginal)
        return r.packetNum <= SIAMESE_PACKET_NUM_MAX && r.tailBytes == 0;
    return r.tailBytes == (r.dataBytes < 8 ? r.dataBytes : 8u);
}

/// What k_scan computes for one row: row[0, stride) in host memory, len = the
/// row's length word or null.  The prefix is judged as frames_parse judges it
/// (a zero L is malformed, a prefix wider than its L needs is not).
inline void row_head_scan(const uint8_t* row, uint64_t stride, const uint32_t* len, RowHead* out)
{
    std::memset(out, 0, sizeof(*out));
    if (len ? *len == 0 : row[0] == 0)
        return;   // kRowEmpty
    RowHead r;
    std::memset(&r, 0, sizeof(r));
    unsigned length = 0;
    const int h = read_length_prefix(row, 4, &length);   // (a row has 16 bytes at least)
    bool ok = h >= 1 && length >= 1 && (!len || *len == (uint64_t)h + length);
    if (ok) {
        const uint8_t* f = row + h;   // type, flow, PacketNum: within the row's first 11 bytes
        r.status = kRowOk;
        r.type = f[0];
        const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
        r.frameBytes = (uint32_t)h + length;
        r.headerBytes = (uint8_t)(h + inner);
        r.flow = f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16);
        r.packetNum = r.type == kFrameOriginal ? f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) : 0;
        r.dataBytes = length > inner ? length - inner : 0;
        r.tailBytes = r.type == kFrameRecovery ? (uint8_t)(r.dataBytes < 8 ? r.dataBytes : 8) : 0;
        ok = row_head_valid(r, stride);
    }
    if (!ok) {
        out->status = kRowMalformed;
        return;
    }
    if (r.type == kFrameRecovery) {
        const uint8_t* data = row + r.headerBytes;
        std::memcpy(r.head, data, r.dataBytes < 4 ? r.dataBytes : 4);
        std::memcpy(r.tail + 8 - r.tailBytes, data + r.dataBytes - r.tailBytes, r.tailBytes);
    }
    *out = r;
}

/// Rows that hold several frames (ops.h PackedHead, sgpu_frames_scan_packed /
/// sgpu_frames_recv_packed).  row_head_valid restated for a frame at an
/// offset: the same checks, with offset + headerBytes + dataBytes within the
/// stride.  sgpu_frames_recv_packed acts on no record that fails it.
inline bool packed_head_valid(const PackedHead& r, uint64_t stride)
{
    if (r.status != kRowOk || r.type > kFrameRecovery)
        return false;
    const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
    if (r.dataBytes < 1 || r.dataBytes > SIAMESE_MAX_PACKET_BYTES)
        return false;
    if (r.headerBytes < inner + 1 || r.headerBytes > inner + 4)
        return false;
    if ((uint64_t)r.offset + r.headerBytes + r.dataBytes > stride)
        return false;
    if (r.flow > kFrameMaxFlow)
        return false;
    if (r.type == kFrameOriginal)
        return r.packetNum <= SIAMESE_PACKET_NUM_MAX && r.tailBytes == 0;
    return r.tailBytes == (r.dataBytes < 8 ? r.dataBytes : 8u);
}

/// What k_walk computes for one row: row[0, stride) in host memory, len = the
/// row's length word or null, out = the row's maxFrames records.  With
/// end = len ? *len : stride: end == 0 is an empty row and end > stride a
/// malformed one without records.  Otherwise row[0, end) is walked as
/// frames_parse walks it: a zero byte where a frame would start is skipped,
/// the prefix is read from the bytes left before end, and a frame is accepted
/// when frames_parse accepts it and packed_head_valid does (which adds the
/// PacketNum range).  The first frame that is not accepted ends the walk with
/// kPackedMalformed; after maxFrames records it ends with kPackedMore if a
/// non-zero byte is left before end.  Records past the last accepted frame
/// are zero.  Returns the row word.
inline uint32_t row_walk(const uint8_t* row, uint64_t stride, const uint32_t* len, uint32_t maxFrames,
                         PackedHead* out)
{
    std::memset(out, 0, (size_t)maxFrames * sizeof(*out));
    const uint64_t end = len ? *len : stride;
    if (end > stride)
        return kPackedMalformed;
    uint64_t at = 0;
    uint32_t n = 0;
    while (at < end) {
        if (row[at] == 0) {
            ++at;
            continue;
        }
        if (n == maxFrames)
            return n | kPackedMore;
        const uint64_t left = end - at;
        unsigned length = 0;
        const int h = read_length_prefix(row + at, left < 4 ? (unsigned)left : 4u, &length);
        if (h < 1 || length < 1 || (uint64_t)h + length > left)
            return n | kPackedMalformed;
        const uint8_t* f = row + at + h;   // type, flow, PacketNum: before end when L > inner
        PackedHead r;
        std::memset(&r, 0, sizeof(r));
        r.offset = (uint32_t)at;
        r.status = kRowOk;
        r.type = f[0];
        const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
        if (r.type > kFrameRecovery || length <= inner)
            return n | kPackedMalformed;
        r.headerBytes = (uint8_t)(h + inner);
        r.flow = f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16);
        r.packetNum = r.type == kFrameOriginal ? f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) : 0;
        r.dataBytes = length - inner;
        r.tailBytes = r.type == kFrameRecovery ? (uint8_t)(r.dataBytes < 8 ? r.dataBytes : 8) : 0;
        if (!packed_head_valid(r, end))
            return n | kPackedMalformed;
        if (r.type == kFrameRecovery) {
            const uint8_t* data = row + at + r.headerBytes;
            std::memcpy(r.head, data, r.dataBytes < 4 ? r.dataBytes : 4);
            std::memcpy(r.tail + 8 - r.tailBytes, data + r.dataBytes - r.tailBytes, r.tailBytes);
        }
        out[n++] = r;
        at += (uint64_t)h + length;
    }
    return n;
}

/// What k_streamwalk computes for one row of a byte stream (ops.h kStreamPartial,
/// sgpu_frames_scan_streams / sgpu_frames_recv_streams): row[0, stride) in host
/// memory, out = the row's maxFrames records, *next = the row offset from which
/// the row's next scan must start.  start > end or end > stride is a malformed
/// row without records and *next = min(start, stride).  Otherwise row[start,
/// end) is walked as row_walk walks row[0, end), with one more outcome: a frame
/// at `at` that the left = end - at bytes do not hold whole -- left is less than
/// the w bytes its first byte announces for the prefix, or the prefix gives L >=
/// 1 with w + L > left -- ends the walk with kStreamPartial when nothing that is
/// already there can make it invalid, and with kPackedMalformed when something
/// can: w + L > stride (no row will ever hold it), a type byte that is present
/// and above kFrameRecovery, a type byte that is present with L <= the type's
/// inner header, or an original whose three PacketNum bytes are all present and
/// exceed SIAMESE_PACKET_NUM_MAX.  *next is `end` when only zero bytes were left,
/// and otherwise the offset of the byte the walk stopped at: the non-zero byte
/// behind the maxFrames-th record (kPackedMore), or the first byte of the frame
/// that is partial or malformed.  (A next word has 32 bits: an `end` of 4 GiB,
/// which only a null end array with that stride gives, is stated as 2^32 - 1.)
/// Records past the last accepted frame are zero.  Returns the row word.
inline uint32_t stream_walk(const uint8_t* row, uint64_t stride, uint64_t start, uint64_t end, uint32_t maxFrames,
                            PackedHead* out, uint32_t* next)
{
    std::memset(out, 0, (size_t)maxFrames * sizeof(*out));
    if (start > end || end > stride) {
        *next = (uint32_t)(start < stride ? start : stride);
        return kPackedMalformed;
    }
    uint64_t at = start;
    uint32_t n = 0;
    while (at < end) {
        if (row[at] == 0) {
            ++at;
            continue;
        }
        *next = (uint32_t)at;
        if (n == maxFrames)
            return n | kPackedMore;
        const uint64_t left = end - at;
        unsigned length = 0;
        const int h = read_length_prefix(row + at, left < 4 ? (unsigned)left : 4u, &length);
        if (h < 1)
            return n | kStreamPartial;   // (the prefix itself is cut off)
        if (length < 1)
            return n | kPackedMalformed;
        const uint8_t* f = row + at + h;   // type, flow, PacketNum: the first left - h of them are there
        if ((uint64_t)h + length > left) {
            const uint64_t have = left - h;
            bool never = (uint64_t)h + length > stride;
            if (have >= 1) {
                const unsigned inner = f[0] == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
                never = never || f[0] > kFrameRecovery || length <= inner;
                if (f[0] == kFrameOriginal && have >= kFrameOriginalInner)
                    never = never || (f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16)) > SIAMESE_PACKET_NUM_MAX;
            }
            return n | (never ? kPackedMalformed : kStreamPartial);
        }
        PackedHead r;
        std::memset(&r, 0, sizeof(r));
        r.offset = (uint32_t)at;
        r.status = kRowOk;
        r.type = f[0];
        const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
        if (r.type > kFrameRecovery || length <= inner)
            return n | kPackedMalformed;
        r.headerBytes = (uint8_t)(h + inner);
        r.flow = f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16);
        r.packetNum = r.type == kFrameOriginal ? f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) : 0;
        r.dataBytes = length - inner;
        r.tailBytes = r.type == kFrameRecovery ? (uint8_t)(r.dataBytes < 8 ? r.dataBytes : 8) : 0;
        if (!packed_head_valid(r, end))
            return n | kPackedMalformed;
        if (r.type == kFrameRecovery) {
            const uint8_t* data = row + at + r.headerBytes;
            std::memcpy(r.head, data, r.dataBytes < 4 ? r.dataBytes : 4);
            std::memcpy(r.tail + 8 - r.tailBytes, data + r.dataBytes - r.tailBytes, r.tailBytes);
        }
        out[n++] = r;
        at += (uint64_t)h + length;
    }
    *next = end < 0xffffffffu ? (uint32_t)end : 0xffffffffu;   // (end = stride = 4 GiB: the row's last byte, a zero)
    return n;
}

/// The next words behind a stream scan's dense part (ops.h streams_bytes): out =
/// streams_bytes(count, maxRecords) bytes whose first dense_bytes(count,
/// maxRecords) dense_compact has written.
inline void streams_put_next(const uint32_t* next, uint32_t count, uint32_t maxRecords, uint8_t* out)
{
    uint8_t* at = out + (size_t)streams_next_offset(count, maxRecords);
    std::memset(at, 0, (size_t)(streams_bytes(count, maxRecords) - streams_next_offset(count, maxRecords)));
    std::memcpy(at, next, (size_t)count * 4);
}

/// What k_rowsum and k_compact compute from the walk's output (ops.h
/// dense_bytes states the layout, sgpu_frames_scan_dense / sgpu_frames_recv_dense
/// use it): words = the count row words, rowRecs = maxFrames records per row as
/// row_walk writes them, out = dense_bytes(count, maxRecords) bytes, every one of
/// which is written.  The starts are the exclusive prefix sum of the words'
/// counts (a count above maxFrames, which no walk writes, counts as maxFrames);
/// rows are all or nothing: c is the largest value with start[c] <= maxRecords,
/// the records of rows [0, c) lie back to back from record 0 and the records
/// from W = start[c] on are zero.
inline void dense_compact(const uint32_t* words, const PackedHead* rowRecs, uint32_t count, uint32_t maxFrames,
                          uint32_t maxRecords, uint8_t* out)
{
    const size_t recAt = (size_t)dense_records_offset(count);
    std::memset(out, 0, (size_t)dense_bytes(count, maxRecords));
    uint8_t* wordsOut = out + 16;
    uint8_t* starts = wordsOut + (size_t)count * 4;
    uint32_t sum = 0, c = 0, W = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t w = words[k];
        uint32_t n = w & kPackedCountMask;
        if (n > maxFrames)
            n = maxFrames;
        std::memcpy(wordsOut + (size_t)k * 4, &w, 4);
        std::memcpy(starts + (size_t)k * 4, &sum, 4);
        if ((uint64_t)sum + n <= maxRecords) {   // (the sums only grow: false once, false ever after)
            std::memcpy(out + recAt + (size_t)sum * sizeof(PackedHead), rowRecs + (size_t)k * maxFrames,
                        (size_t)n * sizeof(PackedHead));
            c = k + 1;
            W = sum + n;
        }
        sum += n;
    }
    std::memcpy(starts + (size_t)count * 4, &sum, 4);
    const uint32_t info[4] = {sum, W, c, 0};
    std::memcpy(out, info, 16);
}

/// Rows of a bidirectional flow (ops.h kRowTruncated, sgpu_frames_scan_duplex /
/// sgpu_frames_recv_duplex).  The one definition of an ack record that a duplex
/// scan with these ackSlots and ackBytes can have produced for a row of
/// `stride` bytes: type kFrameAck; at least one message byte; a header of the
/// four inner bytes plus a 1-4 byte prefix; the frame within the stride; a flow
/// of three bytes; no tail and no head; packetNum = nth, the ack records before
/// it in its row; status kRowOk with a slot (packetNum < ackSlots) that holds
/// the whole message (dataBytes <= ackBytes), or kRowTruncated with one of the
/// two failing.  sgpu_frames_recv_duplex trusts no ack record that fails it,
/// and hands only the kRowOk ones to an encoder.
inline bool ack_head_valid(const PackedHead& r, uint64_t stride, uint32_t ackSlots, uint32_t ackBytes, uint32_t nth)
{
    if (r.type != kFrameAck || r.packetNum != nth || (r.status != kRowOk && r.status != kRowTruncated))
        return false;
    if (r.dataBytes < 1 || r.dataBytes > kFrameMaxLength - kFrameAckInner)
        return false;
    if (r.headerBytes < kFrameAckInner + 1 || r.headerBytes > kFrameAckInner + 4 || r.tailBytes != 0)
        return false;
    if ((uint64_t)r.offset + r.headerBytes + r.dataBytes > stride || r.flow > kFrameMaxFlow)
        return false;
    for (unsigned i = 0; i < 4; ++i)
        if (r.head[i] | r.tail[i] | r.tail[4 + i])
            return false;
    const bool whole = r.packetNum < ackSlots && r.dataBytes <= ackBytes;
    return whole == (r.status == kRowOk);
}

/// What k_ackwalk computes for one row: row_walk's arguments, and slots = the
/// row's ackSlots message slots of ackBytes bytes each.  The walk is row_walk's
/// with one more type: a frame of type kFrameAck with L > 4 is accepted, as the
/// row's a-th ack (a counts from 0).  Its record is what ack_head_valid
/// describes, with packetNum = a and dataBytes = D = L - 4; slot a, when a <
/// ackSlots, gets the message's first min(D, ackBytes) bytes.  An ack without a
/// slot, or longer than its slot, has status kRowTruncated and sets
/// kPackedAcksDropped in the row word; the walk goes on behind it.  Originals
/// and recovery frames give row_walk's records.  Every record and every slot
/// byte is written: records past the last frame and slot bytes past a message
/// are zero.  Returns the row word.
inline uint32_t ack_walk(const uint8_t* row, uint64_t stride, const uint32_t* len, uint32_t maxFrames,
                         uint32_t ackSlots, uint32_t ackBytes, PackedHead* out, uint8_t* slots)
{
    std::memset(out, 0, (size_t)maxFrames * sizeof(*out));
    std::memset(slots, 0, (size_t)ackSlots * ackBytes);
    const uint64_t end = len ? *len : stride;
    if (end > stride)
        return kPackedMalformed;
    uint64_t at = 0;
    uint32_t n = 0, acks = 0, flags = 0;
    while (at < end) {
        if (row[at] == 0) {
            ++at;
            continue;
        }
        if (n == maxFrames)
            return n | flags | kPackedMore;
        const uint64_t left = end - at;
        unsigned length = 0;
        const int h = read_length_prefix(row + at, left < 4 ? (unsigned)left : 4u, &length);
        if (h < 1 || length < 1 || (uint64_t)h + length > left)
            return n | flags | kPackedMalformed;
        const uint8_t* f = row + at + h;   // type, flow, PacketNum: before end when L > inner
        PackedHead r;
        std::memset(&r, 0, sizeof(r));
        r.offset = (uint32_t)at;
        r.status = kRowOk;
        r.type = f[0];
        const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
        if (r.type > kFrameAck || length <= inner)
            return n | flags | kPackedMalformed;
        r.headerBytes = (uint8_t)(h + inner);
        r.flow = f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16);
        r.dataBytes = length - inner;
        if (r.type == kFrameAck) {
            r.packetNum = acks;
            if (acks < ackSlots)
                std::memcpy(slots + (size_t)acks * ackBytes, row + at + r.headerBytes,
                            r.dataBytes < ackBytes ? r.dataBytes : ackBytes);
            if (acks >= ackSlots || r.dataBytes > ackBytes) {
                r.status = kRowTruncated;
                flags |= kPackedAcksDropped;
            }
            ++acks;
        } else {
            r.packetNum = r.type == kFrameOriginal ? f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) : 0;
            r.tailBytes = r.type == kFrameRecovery ? (uint8_t)(r.dataBytes < 8 ? r.dataBytes : 8) : 0;
            if (!packed_head_valid(r, end))
                return n | flags | kPackedMalformed;
            if (r.type == kFrameRecovery) {
                const uint8_t* data = row + at + r.headerBytes;
                std::memcpy(r.head, data, r.dataBytes < 4 ? r.dataBytes : 4);
                std::memcpy(r.tail + 8 - r.tailBytes, data + r.dataBytes - r.tailBytes, r.tailBytes);
            }
        }
        out[n++] = r;
        at += (uint64_t)h + length;
    }
    return n | flags;
}

/// What k_ackstreamwalk computes for one row of a duplex byte stream (ops.h
/// kStreamPartialDuplex, sgpu_frames_scan_duplex_streams /
/// sgpu_frames_recv_duplex_streams): ack_walk and stream_walk as one function.
/// row[0, stride) in host memory, out = the row's maxFrames records, slots = its
/// ackSlots message slots of ackBytes bytes, *next = the row offset from which
/// the row's next scan must start.  start > end or end > stride is a malformed
/// row without records or acks and *next = min(start, stride).  Otherwise
/// row[start, end) is walked as ack_walk walks row[0, end) -- types 0, 1 and 2,
/// the row's a-th ack of this scan with packetNum = a, slot a and the truncated
/// rule -- with stream_walk's outcomes: a frame at `at` that the left = end - at
/// bytes do not hold whole ends the walk with kStreamPartialDuplex, or with
/// kPackedMalformed when something present can never become valid (w + L >
/// stride, a type byte that is present and above kFrameAck, a type byte that is
/// present with L <= the type's inner header, an original whose three PacketNum
/// bytes are present and exceed SIAMESE_PACKET_NUM_MAX).  A partial ack writes
/// no slot, gets no record and is not counted.  *next is stream_walk's.  The word
/// may carry kPackedAcksDropped beside any one stop flag.  Every record and
/// every slot byte is written.  Returns the row word.
inline uint32_t ack_stream_walk(const uint8_t* row, uint64_t stride, uint64_t start, uint64_t end, uint32_t maxFrames,
                                uint32_t ackSlots, uint32_t ackBytes, PackedHead* out, uint8_t* slots, uint32_t* next)
{
    std::memset(out, 0, (size_t)maxFrames * sizeof(*out));
    std::memset(slots, 0, (size_t)ackSlots * ackBytes);
    if (start > end || end > stride) {
        *next = (uint32_t)(start < stride ? start : stride);
        return kPackedMalformed;
    }
    uint64_t at = start;
    uint32_t n = 0, acks = 0, flags = 0;
    while (at < end) {
        if (row[at] == 0) {
            ++at;
            continue;
        }
        *next = (uint32_t)at;
        if (n == maxFrames)
            return n | flags | kPackedMore;
        const uint64_t left = end - at;
        unsigned length = 0;
        const int h = read_length_prefix(row + at, left < 4 ? (unsigned)left : 4u, &length);
        if (h < 1)
            return n | flags | kStreamPartialDuplex;   // (the prefix itself is cut off)
        if (length < 1)
            return n | flags | kPackedMalformed;
        const uint8_t* f = row + at + h;   // type, flow, PacketNum: the first left - h of them are there
        if ((uint64_t)h + length > left) {
            const uint64_t have = left - h;
            bool never = (uint64_t)h + length > stride;
            if (have >= 1) {
                const unsigned inner = f[0] == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
                never = never || f[0] > kFrameAck || length <= inner;
                if (f[0] == kFrameOriginal && have >= kFrameOriginalInner)
                    never = never || (f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16)) > SIAMESE_PACKET_NUM_MAX;
            }
            return n | flags | (never ? kPackedMalformed : kStreamPartialDuplex);
        }
        PackedHead r;
        std::memset(&r, 0, sizeof(r));
        r.offset = (uint32_t)at;
        r.status = kRowOk;
        r.type = f[0];
        const unsigned inner = r.type == kFrameOriginal ? kFrameOriginalInner : kFrameRecoveryInner;
        if (r.type > kFrameAck || length <= inner)
            return n | flags | kPackedMalformed;
        r.headerBytes = (uint8_t)(h + inner);
        r.flow = f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16);
        r.dataBytes = length - inner;
        if (r.type == kFrameAck) {
            r.packetNum = acks;
            if (acks < ackSlots)
                std::memcpy(slots + (size_t)acks * ackBytes, row + at + r.headerBytes,
                            r.dataBytes < ackBytes ? r.dataBytes : ackBytes);
            if (acks >= ackSlots || r.dataBytes > ackBytes) {
                r.status = kRowTruncated;
                flags |= kPackedAcksDropped;
            }
            ++acks;
        } else {
            r.packetNum = r.type == kFrameOriginal ? f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) : 0;
            r.tailBytes = r.type == kFrameRecovery ? (uint8_t)(r.dataBytes < 8 ? r.dataBytes : 8) : 0;
            if (!packed_head_valid(r, end))
                return n | flags | kPackedMalformed;
            if (r.type == kFrameRecovery) {
                const uint8_t* data = row + at + r.headerBytes;
                std::memcpy(r.head, data, r.dataBytes < 4 ? r.dataBytes : 4);
                std::memcpy(r.tail + 8 - r.tailBytes, data + r.dataBytes - r.tailBytes, r.tailBytes);
            }
        }
        out[n++] = r;
        at += (uint64_t)h + length;
    }
    *next = end < 0xffffffffu ? (uint32_t)end : 0xffffffffu;   // (end = stride = 4 GiB: the row's last byte, a zero)
    return n | flags;
}

/// The next words behind a duplex stream scan's dense part (ops.h
/// duplex_streams_bytes): out = duplex_streams_bytes(...) bytes whose first
/// duplex_dense_bytes(...) duplex_dense_compact has written.
inline void duplex_streams_put_next(const uint32_t* next, uint32_t count, uint32_t maxRecords, uint32_t maxAcks,
                                    uint32_t ackBytes, uint8_t* out)
{
    const size_t at = (size_t)duplex_streams_next_offset(count, maxRecords, maxAcks, ackBytes);
    std::memset(out + at, 0, (size_t)duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes) - at);
    std::memcpy(out + at, next, (size_t)count * 4);
}

/// What k_rowsum2, k_compact and k_slots compute from ack_walk's output (ops.h
/// duplex_dense_bytes states the layout, sgpu_frames_scan_duplex_dense /
/// sgpu_frames_recv_duplex_dense use it): words = the count row words, rowRecs =
/// maxFrames records per row and rowSlots = ackSlots slots of ackBytes bytes per
/// row as ack_walk writes them, out = duplex_dense_bytes(count, maxRecords,
/// maxAcks, ackBytes) bytes, every one of which is written.  Row k's share of
/// the slots is a_k = the ack records among its first n_k, at most ackSlots
/// (n_k clamped to maxFrames as in dense_compact).  start[] and astart[] are the
/// exclusive prefix sums of n_k and a_k; rows are all or nothing over both
/// budgets: c is the largest value with start[c] <= maxRecords and astart[c] <=
/// maxAcks, the records and slots of rows [0, c) lie back to back from record 0
/// and slot 0, and records from W = start[c] and slots from WA = astart[c] on
/// are zero.
inline void duplex_dense_compact(const uint32_t* words, const PackedHead* rowRecs, const uint8_t* rowSlots,
                                 uint32_t count, uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes,
                                 uint32_t maxRecords, uint32_t maxAcks, uint8_t* out)
{
    const size_t recAt = (size_t)dense_records_offset(count);
    const size_t slotAt = (size_t)duplex_dense_slots_offset(count, maxRecords);
    std::memset(out, 0, (size_t)duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes));
    uint8_t* wordsOut = out + 16;
    uint8_t* starts = wordsOut + (size_t)count * 4;
    uint8_t* astarts = out + (size_t)duplex_dense_acks_offset(count, maxRecords);
    uint32_t sum = 0, asum = 0, c = 0, W = 0, WA = 0;
    bool open = true;   // (both sums only grow: a row that does not fit closes the prefix)
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t w = words[k];
        uint32_t n = w & kPackedCountMask;
        if (n > maxFrames)
            n = maxFrames;
        uint32_t a = 0;
        for (uint32_t j = 0; j < n; ++j)
            a += rowRecs[(size_t)k * maxFrames + j].type == kFrameAck;
        if (a > ackSlots)
            a = ackSlots;
        std::memcpy(wordsOut + (size_t)k * 4, &w, 4);
        std::memcpy(starts + (size_t)k * 4, &sum, 4);
        std::memcpy(astarts + (size_t)k * 4, &asum, 4);
        open = open && (uint64_t)sum + n <= maxRecords && (uint64_t)asum + a <= maxAcks;
        if (open) {
            std::memcpy(out + recAt + (size_t)sum * sizeof(PackedHead), rowRecs + (size_t)k * maxFrames,
                        (size_t)n * sizeof(PackedHead));
            std::memcpy(out + slotAt + (size_t)asum * ackBytes, rowSlots + (size_t)k * ackSlots * ackBytes,
                        (size_t)a * ackBytes);
            c = k + 1;
            W = sum + n;
            WA = asum + a;
        }
        sum += n;
        asum += a;
    }
    std::memcpy(starts + (size_t)count * 4, &sum, 4);
    std::memcpy(astarts + (size_t)count * 4, &asum, 4);
    const uint32_t info[4] = {sum, W, c, WA};
    std::memcpy(out, info, 16);
}

/// What k_relay computes for one present item (ops.h RelayItem): the symbol
/// sym, of which cap bytes may be read, as the wire frame of original
/// packetNum of `flow` in row[0, stride), its length in *len.  With hs and n
/// the symbol's prefix bytes and length and hf = frame_header_bytes(
/// kFrameOriginal, n), the packet fits when the prefix can be read from
/// min(cap, 4) bytes, n >= 1, hs + n <= cap, hf + n <= stride and the frame's
/// own L = 7 + n fits a length prefix (kFrameMaxLength); then row[0, hf) is
/// frame_write_header's header, row[hf, hf + n) = sym[hs, hs + n), the rest of
/// the row is zero and *len = hf + n.  A packet that does not fit gets a zero
/// row and *len = 0.  Reads only sym[0, min(cap, hs + n)), writes only
/// row[0, stride) and *len.
inline bool relay_fits(unsigned hs, unsigned n, uint32_t cap, uint64_t stride)
{
    return n >= 1 && (uint64_t)hs + n <= cap && (uint64_t)n + kFrameOriginalInner <= kFrameMaxLength &&
           (uint64_t)frame_header_bytes(kFrameOriginal, n) + n <= stride;
}
inline void relay_row(const uint8_t* sym, uint32_t cap, uint32_t flow, uint32_t packetNum, uint8_t* row,
                      uint64_t stride, uint32_t* len)
{
    uint8_t hdr[kFrameMaxHeader];
    unsigned hs = 0, hf = 0, n = 0, length = 0;
    const int h = read_length_prefix(sym, cap < 4 ? cap : 4u, &length);
    if (h >= 1 && relay_fits((unsigned)h, length, cap, stride)) {
        hs = (unsigned)h;
        n = length;
        hf = frame_write_header(kFrameOriginal, flow, packetNum, n, hdr);
    }
    std::memcpy(row, hdr, hf);
    std::memcpy(row + hf, sym + hs, n);
    std::memset(row + hf + n, 0, (size_t)(stride - hf - n));
    *len = hf + n;
}

/// What k_plan computes for one job (ops.h PackJob): syms[k] is item k's symbol
/// (null: absent), of which caps[k] bytes may be read.  Item k is a frame of
/// T = hf + n bytes when relay_row would fill a row of `stride` bytes from it,
/// and takes no space otherwise.  The frames are laid out in item order by the
/// packer's rule (encoder.h pack_frames): a cursor (row, off) starts at (0, 0);
/// a frame with off + T > stride moves to (row + 1, 0); it is placed at off and
/// off becomes align16(off + T).  recs[k] gets the frame's row, its offset and
/// its span (to the next frame of the row, or to the row's end) in 16-byte
/// units, and kPlanWrite when row < maxRows; an item that is no frame gets a
/// zero record.  lens[r], r < maxRows, is the end of row r's last frame, zero
/// for a row without one.  info = {rows the layout needs, frames with
/// kPlanWrite, present items that do not fit, frames without kPlanWrite}.
/// k_pack then is relay_row(sym, cap, flow, packetNum, rows + row * stride +
/// 16 * off16, 16 * span16, ...) for every record with kPlanWrite.  Reads only
/// syms[k][0, min(caps[k], 4)), writes only recs[0, count), lens[0, maxRows)
/// and info[0, 4).
inline void pack_plan(const uint8_t* const* syms, const uint32_t* caps, uint32_t count, uint64_t stride,
                      uint32_t maxRows, PlanRec* recs, uint32_t* lens, uint32_t* info)
{
    uint64_t row = 0, off = 0;
    uint32_t frames = 0, written = 0, unfit = 0;
    uint32_t prev = count;   // the last frame placed: its span is still open
    uint64_t prevOff = 0, prevEnd = 0;
    for (uint32_t r = 0; r < maxRows; ++r)
        lens[r] = 0;
    for (uint32_t k = 0; k < count; ++k) {
        std::memset(&recs[k], 0, sizeof(PlanRec));
        if (!syms[k])
            continue;
        unsigned length = 0;
        const int h = read_length_prefix(syms[k], caps[k] < 4 ? caps[k] : 4u, &length);
        if (h < 1 || !relay_fits((unsigned)h, length, caps[k], stride)) {
            ++unfit;
            continue;
        }
        const uint64_t T = (uint64_t)frame_header_bytes(kFrameOriginal, length) + length;
        if (off + T > stride) {   // (never at off = 0: T <= stride)
            ++row;
            off = 0;
        }
        if (prev != count) {
            recs[prev].span16 = (uint32_t)(((recs[prev].row == row ? off : stride) - prevOff) >> 4);
            if (recs[prev].row != row && recs[prev].row < maxRows)
                lens[recs[prev].row] = (uint32_t)prevEnd;
        }
        recs[k].row = (uint32_t)row;
        recs[k].off16 = (uint32_t)(off >> 4);
        recs[k].flags = row < maxRows ? kPlanWrite : 0;
        written += row < maxRows;
        ++frames;
        prev = k;
        prevOff = off;
        prevEnd = off + T;
        off = (off + T + 15) & ~(uint64_t)15;
    }
    if (prev != count) {
        recs[prev].span16 = (uint32_t)((stride - prevOff) >> 4);
        if (recs[prev].row < maxRows)
            lens[recs[prev].row] = (uint32_t)prevEnd;
    }
    info[0] = frames ? (uint32_t)row + 1 : 0;
    info[1] = written;
    info[2] = unfit;
    info[3] = frames - written;
}

/// What k_offsets computes for one job (ops.h ConcatJob): syms[k] is packet k's
/// symbol (null: absent), of which caps[k] bytes may be read.  p = the leading
/// non-null syms: the stream cannot reach a packet behind a hole.  Packet k < p
/// has prefix bytes hs and length n, and is valid as k_deliver judges it: the
/// prefix can be read from min(cap, 4) bytes, n >= 1 and hs + n <= cap.  With
/// off_0 = 0, packet k is delivered when every packet before it was, it is
/// valid and off_k + n <= capacity; then off_{k+1} = off_k + n.  d = the packets
/// delivered, B = off_d.  offsets[k] = off_k for k <= d and B for d < k <=
/// count; recs[k], k < p, is {off_k, n, hs, kConcatWrite} for k < d and zero
/// otherwise; info = {d, B, stop, p} with stop 0 when d == p, 1 when packet d
/// is invalid and 2 when it is valid and does not fit.  The sums are 64-bit:
/// 65535 lengths of up to 2^29 - 1 pass 2^32.  Reads only syms[k][0,
/// min(caps[k], 4)), writes only offsets[0, count], recs[0, p) and info[0, 4).
inline void concat_plan(const uint8_t* const* syms, const uint32_t* caps, uint32_t count, uint64_t capacity,
                        uint32_t* offsets, ConcatRec* recs, uint32_t* info)
{
    uint32_t p = 0;
    while (p < count && syms[p])
        ++p;
    uint64_t off = 0;
    uint32_t d = 0, stop = 0;
    for (; d < p; ++d) {
        unsigned length = 0;
        const int h = read_length_prefix(syms[d], caps[d] < 4 ? caps[d] : 4u, &length);
        if (h < 1 || length < 1 || (uint64_t)h + length > caps[d]) {
            stop = 1;
            break;
        }
        if (off + length > capacity) {
            stop = 2;
            break;
        }
        offsets[d] = (uint32_t)off;
        recs[d].off = (uint32_t)off;
        recs[d].n = length;
        recs[d].hs = (uint32_t)h;
        recs[d].flags = kConcatWrite;
        off += length;
    }
    for (uint32_t k = d; k <= count; ++k)
        offsets[k] = (uint32_t)off;
    for (uint32_t k = d; k < p; ++k)
        std::memset(&recs[k], 0, sizeof(ConcatRec));
    info[0] = d;
    info[1] = (uint32_t)off;
    info[2] = stop;
    info[3] = p;
}

/// What k_concat computes for one record with kConcatWrite: dst[rec.off,
/// rec.off + rec.n) = sym[rec.hs, rec.hs + rec.n), dst the job's stream at any
/// byte alignment.  No other byte is written, or read.
inline void concat_copy(const uint8_t* sym, const ConcatRec& rec, uint8_t* dst)
{
    if (rec.flags & kConcatWrite)
        std::memcpy(dst + rec.off, sym + rec.hs, rec.n);
}

} // namespace sgpu
