// tests/streams_forged_test.cpp -- TEST ONLY (test_streams_cpu.py).
//
// sgpu_frames_recv_streams on output no scan could have written, as a
// stand-alone host program: the library's host sources and the CPU test double
// of the backend are linked in, and everything is built with
// -fsanitize=address,undefined.  A real stream scan of six rows gives the good
// output; each forgery -- of info, the words, the starts, the records and the
// next words -- is applied to a copy in a heap block of exactly
// sgpu_frames_streams_bytes bytes, so the sanitizer sees any read past it, and
// consumedOut is a heap block of exactly count words.  The program checks the
// return value, the rows routed, the frames accepted and consumedOut itself.
#include "../include/siamese_gpu.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace {
constexpr unsigned kStride = 128, kMaxFrames = 2, kCount = 6, kMaxRecords = kCount * kMaxFrames;
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
} // namespace

int main()
{
    if (sgpu_init(-1) != 0) {
        std::printf("sgpu_init failed\n");
        return 2;
    }
    // six rows of two originals each, 50 + k and 150 + k; row 4 goes on with a third frame, which is cut off
    std::vector<uint8_t> rows((size_t)kCount * kStride, 0);
    std::vector<unsigned> ends(kCount), whole(kCount);
    for (unsigned k = 0; k < kCount; ++k) {
        const std::vector<uint8_t> a = original(50 + k, 12 + k), b = original(150 + k, 12 + k);
        uint8_t* row = rows.data() + (size_t)k * kStride;
        std::memcpy(row, a.data(), a.size());
        std::memcpy(row + a.size() + 1 + k, b.data(), b.size());
        ends[k] = whole[k] = (unsigned)(a.size() + 1 + k + b.size());
        if (k == 4) {
            const std::vector<uint8_t> c = original(250, 30);
            std::memcpy(row + ends[k], c.data(), c.size());
            ends[k] += 9;
        }
    }
    void* dev = sgpu_device_alloc(rows.size());
    void* devEnds = sgpu_device_alloc(4 * kCount);
    const size_t bytes = sgpu_frames_streams_bytes(kCount, kMaxRecords);
    const size_t nextAt = sgpu_frames_streams_next(kCount, kMaxRecords);
    void* pinned = sgpu_host_alloc(bytes);
    if (!dev || !devEnds || !pinned || bytes == 0 || nextAt != sgpu_frames_dense_bytes(kCount, kMaxRecords))
        return 2;
    sgpu_h2d(dev, rows.data(), rows.size());
    sgpu_h2d(devEnds, ends.data(), 4 * kCount);
    const long long t = sgpu_frames_scan_streams(dev, kStride, nullptr, static_cast<unsigned*>(devEnds), kCount,
                                                 kMaxFrames, kMaxRecords, pinned);
    if (t <= 0 || sgpu_gather_wait(t) != 0)
        return 2;
    const std::vector<uint8_t> good(static_cast<uint8_t*>(pinned), static_cast<uint8_t*>(pinned) + bytes);
    const size_t startAt = 16 + 4 * kCount, recAt = sgpu_frames_dense_records(kCount);
    {
        uint32_t word4, next4;
        std::memcpy(&word4, good.data() + 16 + 4 * 4, 4);
        std::memcpy(&next4, good.data() + nextAt + 4 * 4, 4);
        // (maxFrames records are out when the walk meets it: more, not yet partial)
        expect(word4 == (2u | SGPU_PACKED_MORE) && next4 == whole[4], "the scan", "row 4 does not stop at its third frame");
    }

    struct Case
    {
        const char* what;
        std::function<void(std::vector<uint8_t>&)> forge;
        SiameseResult result;
        unsigned rows, accepted;
    };
    const std::vector<Case> cases = {
        {"nothing forged", [](std::vector<uint8_t>&) {}, Siamese_Success, kCount, kMaxRecords},
        {"a next word above the stride", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 2, kStride + 1); },
         Siamese_InvalidInput, 2, 4},
        {"a huge next word", [&](std::vector<uint8_t>& b) { put32(b, nextAt, 0xffffffffu); }, Siamese_InvalidInput, 0,
         0},
        {"a next word below the end of the row's last record",
         [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 3, whole[3] - 1); }, Siamese_InvalidInput, 3, 6},
        {"a next word of zero behind records", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 5, 0); },
         Siamese_InvalidInput, 5, 10},
        {"a next word at the stride", [&](std::vector<uint8_t>& b) { put32(b, nextAt + 4 * 4, kStride); },
         Siamese_Success, kCount, kMaxRecords},
        {"a last record whose end wraps around 2^32",
         [&](std::vector<uint8_t>& b) { put32(b, recAt + 1 * 32, 0xfffffff0u); }, Siamese_InvalidInput, 0, 0},
        {"decreasing starts", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4 * 3, 3); }, Siamese_InvalidInput, 2,
         4},
        {"start[0] != 0", [&](std::vector<uint8_t>& b) { put32(b, startAt, 1); }, Siamese_InvalidInput, 0, 0},
        {"a huge start", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4, 0xfffffff0u); }, Siamese_InvalidInput, 0,
         0},
        {"c far above count", [&](std::vector<uint8_t>& b) { put32(b, 8, 0xffffffffu); }, Siamese_InvalidInput, 0, 0},
        {"W far above maxRecords", [&](std::vector<uint8_t>& b) { put32(b, 4, 0xffffffffu); }, Siamese_InvalidInput, 0,
         0},
        {"W != start[c]", [&](std::vector<uint8_t>& b) { put32(b, 4, kMaxRecords - 1); }, Siamese_InvalidInput, 5, 10},
        {"a word's count above maxFrames", [&](std::vector<uint8_t>& b) { put32(b, 16, 0xffffu); },
         Siamese_InvalidInput, kCount, kMaxRecords - kMaxFrames},
        {"the partial bit on a word", [&](std::vector<uint8_t>& b) { put32(b, 16 + 4 * 3, 2u | SGPU_STREAM_PARTIAL); },
         Siamese_Success, kCount, kMaxRecords},
        {"every flag on a word", [&](std::vector<uint8_t>& b) { put32(b, 16 + 4, 0xffff0002u); }, Siamese_InvalidInput,
         kCount, kMaxRecords},
        {"a record whose Offset + HeaderBytes + DataBytes passes the stride",
         [&](std::vector<uint8_t>& b) { put32(b, recAt + 2 * 32, kStride - 8); }, Siamese_InvalidInput, kCount,
         kMaxRecords - 1},
        {"a record whose DataBytes is the stride", [&](std::vector<uint8_t>& b) { put32(b, recAt + 2 * 32 + 16, kStride); },
         Siamese_InvalidInput, kCount, kMaxRecords - 1},
    };
    for (const Case& c : cases) {
        // (heap blocks of exactly the output's bytes and of count words: an access past either is reported)
        std::vector<uint8_t> b(good);
        c.forge(b);
        uint8_t* heap = static_cast<uint8_t*>(std::malloc(b.size()));
        std::memcpy(heap, b.data(), b.size());
        unsigned* consumed = static_cast<unsigned*>(std::malloc(kCount * sizeof(unsigned)));
        for (unsigned k = 0; k < kCount; ++k)
            consumed[k] = kUntouched;
        SgpuDecoder dec = sgpu_decoder_create();
        std::vector<SiameseResult> results(kMaxRecords, Siamese_Disabled);
        unsigned rowsOut = 99, accepted = 99;
        const SiameseResult r = sgpu_frames_recv_streams(&dec, 1, heap, kMaxFrames, kMaxRecords, dev, kStride, kCount,
                                                         results.data(), consumed, &rowsOut, &accepted);
        char detail[128];
        std::snprintf(detail, sizeof(detail), "returned %d, %u rows, %u accepted", (int)r, rowsOut, accepted);
        expect(r == c.result, c.what, detail);
        expect(rowsOut == c.rows && accepted == c.accepted, c.what, detail);
        for (unsigned k = 0; k < kCount; ++k) {
            uint32_t next;
            std::memcpy(&next, b.data() + nextAt + 4 * k, 4);
            expect(consumed[k] == (k < rowsOut ? next : kUntouched), c.what, "consumedOut");
        }
        sgpu_flush();
        sgpu_decoder_free(dec);
        sgpu_flush();
        std::free(consumed);
        std::free(heap);
    }
    sgpu_host_free(pinned);
    sgpu_device_free(dev);
    sgpu_device_free(devEnds);
    if (g_failures)
        return 1;
    std::printf("streams forged ok: %zu cases\n", cases.size());
    return 0;
}
