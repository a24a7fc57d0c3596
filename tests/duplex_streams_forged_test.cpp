// tests/duplex_streams_forged_test.cpp -- TEST ONLY (test_duplex_streams_cpu.py).
//
// sgpu_frames_recv_duplex_streams on output no scan could have written, as a
// stand-alone host program: the library's host sources and the CPU test double
// of the backend are linked in, and everything is built with
// -fsanitize=address,undefined.  A real duplex stream scan of six rows, each an
// original and an acknowledgement, gives the good output; each forgery is
// applied to a copy in a heap block of exactly sgpu_frames_duplex_streams_bytes
// bytes, so the sanitizer sees any read past it -- a slot index or a record
// index taken from a forged word included -- and the row area is a block of
// exactly count * stride bytes.  The program checks the return value, the rows
// routed, the frames accepted and consumedOut itself.
#include "../include/siamese_gpu.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace {
constexpr unsigned kStride = 128, kMaxFrames = 2, kAckSlots = 1, kAckBytes = 16, kCount = 6;
constexpr unsigned kMaxRecords = kCount * kMaxFrames, kMaxAcks = kCount * kAckSlots, kPackets = 12;
constexpr unsigned kUntouched = 0xdeadbeefu;

int g_failures = 0;
void expect(bool ok, const char* what, const char* detail)
{
    if (!ok) {
        std::printf("FAILED %s: %s\n", what, detail);
        ++g_failures;
    }
}

// an original's wire frame: prefix, type 0, flow 0, PacketNum, data
std::vector<uint8_t> original(unsigned num, unsigned bytes)
{
    std::vector<uint8_t> f;
    f.push_back((uint8_t)(7 + bytes));
    f.push_back(0);
    f.insert(f.end(), {0, 0, 0});
    f.insert(f.end(), {(uint8_t)num, (uint8_t)(num >> 8), (uint8_t)(num >> 16)});
    for (unsigned i = 0; i < bytes; ++i)
        f.push_back((uint8_t)(num * 7 + i + 1));
    return f;
}

void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) { std::memcpy(b.data() + at, &v, 4); }

// a sender with kPackets originals of 20 bytes each, from device memory
SgpuEncoder sender(const void* devData)
{
    SgpuEncoder e = sgpu_encoder_create();
    for (unsigned i = 0; i < kPackets; ++i) {
        unsigned num = 0;
        sgpu_encoder_add(e, static_cast<const uint8_t*>(devData) + 32 * i, 20, &num);
    }
    return e;
}
} // namespace

int main()
{
    if (sgpu_init(-1) != 0) {
        std::printf("sgpu_init failed\n");
        return 2;
    }
    // the acknowledgement of a receiver that holds packets 0 and 2 of the sender's
    std::vector<uint8_t> packets(32 * kPackets);
    for (size_t i = 0; i < packets.size(); ++i)
        packets[i] = (uint8_t)(i * 13 + 5);
    void* devData = sgpu_device_alloc(packets.size());
    if (!devData)
        return 2;
    sgpu_h2d(devData, packets.data(), packets.size());
    SgpuDecoder receiver = sgpu_decoder_create();
    sgpu_decoder_add_original(receiver, 0, devData, 20);
    sgpu_decoder_add_original(receiver, 2, static_cast<uint8_t*>(devData) + 64, 20);
    uint8_t msg[kAckBytes];
    unsigned msgBytes = 0;
    if (sgpu_decoder_ack(receiver, msg, kAckBytes, &msgBytes) != Siamese_Success || msgBytes == 0)
        return 2;
    uint8_t ackFrame[kAckBytes + 8];
    const unsigned ackFrameBytes = sgpu_frame_write_ack(0, msg, msgBytes, ackFrame, sizeof(ackFrame));
    if (ackFrameBytes == 0)
        return 2;

    // six rows: original 50 + k, a gap, the ack frame; the bytes behind each row's end are stale 0xff
    std::vector<uint8_t> rows((size_t)kCount * kStride, 0xff);
    std::vector<unsigned> ends(kCount);
    for (unsigned k = 0; k < kCount; ++k) {
        const std::vector<uint8_t> a = original(50 + k, 12 + k);
        uint8_t* row = rows.data() + (size_t)k * kStride;
        ends[k] = (unsigned)(a.size() + 1 + k + ackFrameBytes);
        std::memset(row, 0, ends[k]);
        std::memcpy(row, a.data(), a.size());
        std::memcpy(row + a.size() + 1 + k, ackFrame, ackFrameBytes);
    }
    void* dev = sgpu_device_alloc(rows.size());
    void* devEnds = sgpu_device_alloc(4 * kCount);
    const size_t bytes = sgpu_frames_duplex_streams_bytes(kCount, kMaxRecords, kMaxAcks, kAckBytes);
    const size_t nextAt = sgpu_frames_duplex_streams_next(kCount, kMaxRecords, kMaxAcks, kAckBytes);
    void* pinned = sgpu_host_alloc(bytes);
    if (!dev || !devEnds || !pinned || bytes == 0 || nextAt == 0)
        return 2;
    sgpu_h2d(dev, rows.data(), rows.size());
    sgpu_h2d(devEnds, ends.data(), 4 * kCount);
    const long long t = sgpu_frames_scan_duplex_streams(dev, kStride, nullptr, static_cast<unsigned*>(devEnds), kCount,
                                                        kMaxFrames, kAckSlots, kAckBytes, kMaxRecords, kMaxAcks, pinned);
    if (t <= 0 || sgpu_gather_wait(t) != 0)
        return 2;
    const std::vector<uint8_t> good(static_cast<uint8_t*>(pinned), static_cast<uint8_t*>(pinned) + bytes);
    const size_t startAt = 16 + 4 * kCount, recAt = sgpu_frames_dense_records(kCount);
    const size_t ackAt = sgpu_frames_duplex_dense_acks(kCount, kMaxRecords);
    // (SgpuPackedHead: Offset at 0, Status at 4, Type at 5, PacketNum at 12, DataBytes at 16)
    auto rec = [&](unsigned i) { return recAt + 32 * (size_t)i; };

    struct Case
    {
        const char* what;
        std::function<void(std::vector<uint8_t>&)> forge;
        bool ok;
        unsigned rows, accepted;
    };
    const std::vector<Case> cases = {
        {"nothing forged", [](std::vector<uint8_t>&) {}, true, kCount, kMaxRecords},
        {"a next word above the stride", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 2, kStride + 1); }, false,
         2, 4},
        {"a huge next word", [&](std::vector<uint8_t>& b) { put32(b, nextAt, 0xffffffffu); }, false, 0, 0},
        {"a next word below the end of the row's last record",
         [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 3, ends[3] - 1); }, false, 3, 6},
        {"a next word of zero behind records", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 5, 0); }, false, 5,
         10},
        {"a next word at the stride", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 4, kStride); }, true, kCount,
         kMaxRecords},
        {"an astart step that disagrees with the row's ack records",
         [&](std::vector<uint8_t>& b) { put32(b, ackAt + 8, 3); }, false, 1, 2},
        {"a huge astart", [&](std::vector<uint8_t>& b) { put32(b, ackAt + 4, 0xfffffff0u); }, false, 0, 0},
        {"a start beyond W", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4 * 3, kMaxRecords + 1); }, false, 2, 4},
        {"a huge start", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4, 0xfffffff0u); }, false, 0, 0},
        {"c > count", [&](std::vector<uint8_t>& b) { put32(b, 8, kCount + 1); }, false, 0, 0},
        {"c far above count", [&](std::vector<uint8_t>& b) { put32(b, 8, 0xffffffffu); }, false, 0, 0},
        {"a slot index outside the row's span", [&](std::vector<uint8_t>& b) { put32(b, rec(3) + 12, 1); }, false, 1, 2},
        {"a slot index of 2^31", [&](std::vector<uint8_t>& b) { put32(b, rec(3) + 12, 1u << 31); }, false, 1, 2},
        {"a word count above maxFrames", [&](std::vector<uint8_t>& b) { put32(b, 16, 0xffffu); }, false, kCount,
         kMaxRecords - kMaxFrames},
        {"the partial flag on a complete row",
         [&](std::vector<uint8_t>& b) { put32(b, 16 + 4, 2 | SGPU_STREAM_PARTIAL_DUPLEX); }, true, kCount, kMaxRecords},
        {"the partial flag together with a forged record",
         [&](std::vector<uint8_t>& b) {
             put32(b, 16 + 4, 2 | SGPU_STREAM_PARTIAL_DUPLEX);
             put32(b, rec(2), kStride - 8);
         },
         false, kCount, kMaxRecords - 1},
    };
    for (const Case& c : cases) {
        // (a heap block of exactly the output's bytes: a read past it is reported)
        std::vector<uint8_t> b(good);
        c.forge(b);
        uint8_t* heap = static_cast<uint8_t*>(std::malloc(b.size()));
        std::memcpy(heap, b.data(), b.size());
        SgpuDecoder dec = sgpu_decoder_create();
        SgpuEncoder enc = sender(devData);
        std::vector<SiameseResult> results(kMaxRecords, Siamese_Disabled);
        std::vector<unsigned> next(kMaxRecords, 0), consumed(kCount, kUntouched);
        unsigned rowsOut = 99, accepted = 99;
        const SiameseResult r = sgpu_frames_recv_duplex_streams(
            &dec, 1, &enc, 1, heap, kMaxFrames, kAckSlots, kAckBytes, kMaxRecords, kMaxAcks, dev, kStride, kCount,
            results.data(), next.data(), consumed.data(), &rowsOut, &accepted);
        char detail[128];
        std::snprintf(detail, sizeof(detail), "returned %d, %u rows, %u accepted", (int)r, rowsOut, accepted);
        expect(r == (c.ok ? Siamese_Success : Siamese_InvalidInput), c.what, detail);
        expect(rowsOut == c.rows && accepted == c.accepted, c.what, detail);
        for (unsigned k = 0; k < kCount; ++k) {
            uint32_t w;
            std::memcpy(&w, b.data() + nextAt + 4 * k, 4);
            expect(consumed[k] == (k < rowsOut ? w : kUntouched), c.what, "consumedOut");
        }
        sgpu_flush();
        sgpu_decoder_free(dec);
        sgpu_encoder_free(enc);
        sgpu_flush();
        std::free(heap);
    }
    // a null consumedOut is refused before anything is read
    {
        SgpuDecoder dec = sgpu_decoder_create();
        SgpuEncoder enc = sender(devData);
        unsigned rowsOut = 99, accepted = 99;
        const SiameseResult r = sgpu_frames_recv_duplex_streams(&dec, 1, &enc, 1, pinned, kMaxFrames, kAckSlots,
                                                                kAckBytes, kMaxRecords, kMaxAcks, dev, kStride, kCount,
                                                                nullptr, nullptr, nullptr, &rowsOut, &accepted);
        expect(r == Siamese_InvalidInput && rowsOut == 0 && accepted == 0, "a null consumedOut", "not refused");
        sgpu_decoder_free(dec);
        sgpu_encoder_free(enc);
        sgpu_flush();
    }
    sgpu_decoder_free(receiver);
    sgpu_flush();
    sgpu_host_free(pinned);
    sgpu_device_free(dev);
    sgpu_device_free(devEnds);
    sgpu_device_free(devData);
    if (g_failures)
        return 1;
    std::printf("duplex streams forged ok: %zu cases\n", cases.size());
    return 0;
}
