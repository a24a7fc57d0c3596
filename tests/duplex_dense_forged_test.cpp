// tests/duplex_dense_forged_test.cpp -- TEST ONLY (test_duplex_dense_cpu.py).
//
// sgpu_frames_recv_duplex_dense on output no scan could have written, as a
// stand-alone host program: the library's host sources and the CPU test double
// of the backend are linked in, and everything is built with
// -fsanitize=address,undefined.  A real dense duplex scan of six rows, each an
// original and an acknowledgement, gives the good output; each forgery is
// applied to a copy in a heap block of exactly sgpu_frames_duplex_dense_bytes
// bytes, so the sanitizer sees any read past it -- a slot index taken from a
// forged record or table included -- and the row area is a block of exactly
// count * stride bytes.  The program checks the return value, the rows routed
// and the frames accepted itself.
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

    // six rows: original 50 + k, a gap, the ack frame
    std::vector<uint8_t> rows((size_t)kCount * kStride, 0);
    std::vector<unsigned> lens(kCount);
    for (unsigned k = 0; k < kCount; ++k) {
        const std::vector<uint8_t> a = original(50 + k, 12 + k);
        uint8_t* row = rows.data() + (size_t)k * kStride;
        std::memcpy(row, a.data(), a.size());
        std::memcpy(row + a.size() + 1 + k, ackFrame, ackFrameBytes);
        lens[k] = (unsigned)(a.size() + 1 + k + ackFrameBytes);
    }
    void* dev = sgpu_device_alloc(rows.size());
    void* devLens = sgpu_device_alloc(4 * kCount);
    const size_t bytes = sgpu_frames_duplex_dense_bytes(kCount, kMaxRecords, kMaxAcks, kAckBytes);
    void* pinned = sgpu_host_alloc(bytes);
    if (!dev || !devLens || !pinned || bytes == 0)
        return 2;
    sgpu_h2d(dev, rows.data(), rows.size());
    sgpu_h2d(devLens, lens.data(), 4 * kCount);
    const long long t = sgpu_frames_scan_duplex_dense(dev, kStride, static_cast<unsigned*>(devLens), kCount, kMaxFrames,
                                                      kAckSlots, kAckBytes, kMaxRecords, kMaxAcks, pinned);
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
        unsigned rows, accepted;
    };
    const std::vector<Case> cases = {
        {"nothing forged", [](std::vector<uint8_t>&) {}, kCount, kMaxRecords},
        {"c > count", [&](std::vector<uint8_t>& b) { put32(b, 8, kCount + 1); }, 0, 0},
        {"c far above count", [&](std::vector<uint8_t>& b) { put32(b, 8, 0xffffffffu); }, 0, 0},
        {"W > maxRecords", [&](std::vector<uint8_t>& b) { put32(b, 4, kMaxRecords + 1); }, 0, 0},
        {"W != start[c]", [&](std::vector<uint8_t>& b) { put32(b, 4, kMaxRecords - 1); }, 5, 10},
        {"WA > maxAcks", [&](std::vector<uint8_t>& b) { put32(b, 12, kMaxAcks + 1); }, 0, 0},
        {"WA far above maxAcks", [&](std::vector<uint8_t>& b) { put32(b, 12, 0xffffffffu); }, 0, 0},
        {"WA != astart[c]", [&](std::vector<uint8_t>& b) { put32(b, 12, kMaxAcks - 1); }, 5, 10},
        {"start[0] != 0", [&](std::vector<uint8_t>& b) { put32(b, startAt, 1); }, 0, 0},
        {"astart[0] != 0", [&](std::vector<uint8_t>& b) { put32(b, ackAt, 1); }, 0, 0},
        {"decreasing starts", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4 * 3, 3); }, 2, 4},
        {"decreasing astarts", [&](std::vector<uint8_t>& b) { put32(b, ackAt + 4 * 3, 1); }, 2, 4},
        {"a huge start", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4, 0xfffffff0u); }, 0, 0},
        {"a huge astart", [&](std::vector<uint8_t>& b) { put32(b, ackAt + 4, 0xfffffff0u); }, 0, 0},
        {"an astart step that disagrees with the row's ack records",
         [&](std::vector<uint8_t>& b) { put32(b, ackAt + 8, 3); }, 1, 2},
        {"an astart step for a row without an ack record", [&](std::vector<uint8_t>& b) { b[rec(5) + 5] = 0; }, 2, 4},
        {"a word's count above maxFrames", [&](std::vector<uint8_t>& b) { put32(b, 16, 0xffffu); }, kCount,
         kMaxRecords - kMaxFrames},
        // (PacketNum names a slot outside the row's own: the step fails for 1, the record for a slot past all)
        {"an ack record with PacketNum 1", [&](std::vector<uint8_t>& b) { put32(b, rec(3) + 12, 1); }, 1, 2},
        {"an ack record with PacketNum 2^31", [&](std::vector<uint8_t>& b) { put32(b, rec(3) + 12, 1u << 31); }, 1, 2},
        {"an ack record with Status 4", [&](std::vector<uint8_t>& b) { b[rec(3) + 4] = 4; }, kCount, kMaxRecords - 1},
        {"an ack record truncated without cause", [&](std::vector<uint8_t>& b) { b[rec(3) + 4] = SGPU_ROW_TRUNCATED; },
         kCount, kMaxRecords - 1},
        {"an ack record whose DataBytes exceeds its slot",
         [&](std::vector<uint8_t>& b) { put32(b, rec(3) + 16, kAckBytes + 1); }, kCount, kMaxRecords - 1},
        {"an ack record whose Offset is 2^31", [&](std::vector<uint8_t>& b) { put32(b, rec(3), 1u << 31); }, kCount,
         kMaxRecords - 1},
        {"a data record whose Offset + HeaderBytes + DataBytes passes the stride",
         [&](std::vector<uint8_t>& b) { put32(b, rec(2), kStride - 8); }, kCount, kMaxRecords - 1},
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
        std::vector<unsigned> next(kMaxRecords, 0);
        unsigned rowsOut = 99, accepted = 99;
        const SiameseResult r = sgpu_frames_recv_duplex_dense(&dec, 1, &enc, 1, heap, kMaxFrames, kAckSlots, kAckBytes,
                                                              kMaxRecords, kMaxAcks, dev, kStride, kCount,
                                                              results.data(), next.data(), &rowsOut, &accepted);
        char detail[128];
        std::snprintf(detail, sizeof(detail), "returned %d, %u rows, %u accepted", (int)r, rowsOut, accepted);
        const bool forged = std::strcmp(c.what, "nothing forged") != 0;
        expect(r == (forged ? Siamese_InvalidInput : Siamese_Success), c.what, detail);
        expect(rowsOut == c.rows && accepted == c.accepted, c.what, detail);
        sgpu_flush();
        sgpu_decoder_free(dec);
        sgpu_encoder_free(enc);
        sgpu_flush();
        std::free(heap);
    }
    sgpu_decoder_free(receiver);
    sgpu_flush();
    sgpu_host_free(pinned);
    sgpu_device_free(dev);
    sgpu_device_free(devLens);
    sgpu_device_free(devData);
    if (g_failures)
        return 1;
    std::printf("duplex dense forged ok: %zu cases\n", cases.size());
    return 0;
}
