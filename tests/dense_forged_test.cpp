// tests/dense_forged_test.cpp -- TEST ONLY (test_dense_cpu.py).
//
// sgpu_frames_recv_dense on output no scan could have written, as a stand-alone
// host program: the library's host sources and the CPU test double of the
// backend are linked in, and everything is built with
// -fsanitize=address,undefined.  A real dense scan of six rows gives the good
// output; each forgery is applied to a copy in a heap block of exactly
// sgpu_frames_dense_bytes bytes, so the sanitizer sees any read past it, and the
// row area is a block of exactly count * stride bytes.  The program checks the
// return value, the rows routed and the frames accepted itself.
#include "../include/siamese_gpu.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace {
constexpr unsigned kStride = 128, kMaxFrames = 2, kCount = 6, kMaxRecords = kCount * kMaxFrames;

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
    // six rows of two originals each: 50 + k and 150 + k
    std::vector<uint8_t> rows((size_t)kCount * kStride, 0);
    std::vector<unsigned> lens(kCount);
    for (unsigned k = 0; k < kCount; ++k) {
        const std::vector<uint8_t> a = original(50 + k, 12 + k), b = original(150 + k, 12 + k);
        uint8_t* row = rows.data() + (size_t)k * kStride;
        std::memcpy(row, a.data(), a.size());
        std::memcpy(row + a.size() + 1 + k, b.data(), b.size());
        lens[k] = (unsigned)(a.size() + 1 + k + b.size());
    }
    void* dev = sgpu_device_alloc(rows.size());
    void* devLens = sgpu_device_alloc(4 * kCount);
    const size_t bytes = sgpu_frames_dense_bytes(kCount, kMaxRecords);
    void* pinned = sgpu_host_alloc(bytes);
    if (!dev || !devLens || !pinned || bytes == 0)
        return 2;
    sgpu_h2d(dev, rows.data(), rows.size());
    sgpu_h2d(devLens, lens.data(), 4 * kCount);
    const long long t = sgpu_frames_scan_dense(dev, kStride, static_cast<unsigned*>(devLens), kCount, kMaxFrames,
                                               kMaxRecords, pinned);
    if (t <= 0 || sgpu_gather_wait(t) != 0)
        return 2;
    const std::vector<uint8_t> good(static_cast<uint8_t*>(pinned), static_cast<uint8_t*>(pinned) + bytes);
    const size_t startAt = 16 + 4 * kCount, recAt = sgpu_frames_dense_records(kCount);

    struct Case
    {
        const char* what;
        std::function<void(std::vector<uint8_t>&)> forge;
        unsigned rows, accepted;
    };
    const std::vector<Case> cases = {
        {"nothing forged", [](std::vector<uint8_t>&) {}, kCount, kMaxRecords},
        {"decreasing starts", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4 * 3, 3); }, 2, 4},
        {"start[0] != 0", [&](std::vector<uint8_t>& b) { put32(b, startAt, 1); }, 0, 0},
        {"a start difference that disagrees with its word", [&](std::vector<uint8_t>& b) { put32(b, startAt + 8, 3); },
         1, 2},
        {"a huge start", [&](std::vector<uint8_t>& b) { put32(b, startAt + 4, 0xfffffff0u); }, 0, 0},
        {"c > count", [&](std::vector<uint8_t>& b) { put32(b, 8, kCount + 1); }, 0, 0},
        {"c far above count", [&](std::vector<uint8_t>& b) { put32(b, 8, 0xffffffffu); }, 0, 0},
        {"W > maxRecords", [&](std::vector<uint8_t>& b) { put32(b, 4, kMaxRecords + 1); }, 0, 0},
        {"W far above maxRecords", [&](std::vector<uint8_t>& b) { put32(b, 4, 0xffffffffu); }, 0, 0},
        {"W != start[c]", [&](std::vector<uint8_t>& b) { put32(b, 4, kMaxRecords - 1); }, 5, 10},
        {"a word's count above maxFrames", [&](std::vector<uint8_t>& b) { put32(b, 16, 0xffffu); }, kCount,
         kMaxRecords - kMaxFrames},
        {"a record whose Offset + HeaderBytes + DataBytes passes the stride",
         [&](std::vector<uint8_t>& b) { put32(b, recAt + 3 * 32, kStride - 8); }, kCount, kMaxRecords - 1},
        {"a record whose Offset is 2^31", [&](std::vector<uint8_t>& b) { put32(b, recAt + 3 * 32, 1u << 31); }, kCount,
         kMaxRecords - 1},
        {"a record whose DataBytes is the stride", [&](std::vector<uint8_t>& b) { put32(b, recAt + 3 * 32 + 16, kStride); },
         kCount, kMaxRecords - 1},
    };
    for (const Case& c : cases) {
        // (a heap block of exactly the output's bytes: a read past it is reported)
        std::vector<uint8_t> b(good);
        c.forge(b);
        uint8_t* heap = static_cast<uint8_t*>(std::malloc(b.size()));
        std::memcpy(heap, b.data(), b.size());
        SgpuDecoder dec = sgpu_decoder_create();
        std::vector<SiameseResult> results(kMaxRecords, Siamese_Disabled);
        unsigned rowsOut = 99, accepted = 99;
        const SiameseResult r = sgpu_frames_recv_dense(&dec, 1, heap, kMaxFrames, kMaxRecords, dev, kStride, kCount,
                                                       results.data(), &rowsOut, &accepted);
        char detail[128];
        std::snprintf(detail, sizeof(detail), "returned %d, %u rows, %u accepted", (int)r, rowsOut, accepted);
        const bool forged = std::strcmp(c.what, "nothing forged") != 0;
        expect(r == (forged ? Siamese_InvalidInput : Siamese_Success), c.what, detail);
        expect(rowsOut == c.rows && accepted == c.accepted, c.what, detail);
        sgpu_flush();
        sgpu_decoder_free(dec);
        sgpu_flush();
        std::free(heap);
    }
    sgpu_host_free(pinned);
    sgpu_device_free(dev);
    sgpu_device_free(devLens);
    if (g_failures)
        return 1;
    std::printf("dense forged ok: %zu cases\n", cases.size());
    return 0;
}
