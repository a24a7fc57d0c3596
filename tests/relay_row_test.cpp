// relay_row_test.cpp -- frames.h relay_row alone: the plain C++ statement of
// what one k_relay item does (ops.h RelayItem), which the test double of the
// backend runs.  A stand-alone host program (tests/test_relay_row.py builds it
// with -fsanitize=address,undefined): every source and every row is a heap
// block of exactly the bytes relay_row may touch, so a read past
// sym[0, min(cap, hs + n)) or a write past row[0, stride) is a report.
//
// Every symbol prefix width hs = 1..4 that can state the length (so the
// non-canonical, wider-than-needed prefixes too), at source offsets 0..15 of
// the block, for the payload lengths of relay_cases.py's edge case; then the
// packets that do not fit: a zero prefix, hs + n = cap + 1, hf + n = stride + 1.
// The expected header is built here, not by frame_write_header.
#include "frames.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sgpu;

namespace {

int g_failures = 0;

void fail(const char* what, unsigned hs, unsigned n, unsigned off)
{
    if (++g_failures <= 20)
        std::printf("FAIL %s: hs %u n %u offset %u\n", what, hs, n, off);
}

// a length prefix of exactly `width` bytes (reference SiameseSerializers.h:566-593)
void put_prefix(unsigned width, unsigned length, uint8_t* out)
{
    switch (width) {
    case 1:
        out[0] = (uint8_t)length;
        break;
    case 2:
        out[0] = (uint8_t)(0x80 | (length >> 8));
        out[1] = (uint8_t)length;
        break;
    case 3:
        out[0] = (uint8_t)(0xC0 | (length >> 16));
        out[1] = (uint8_t)(length >> 8);
        out[2] = (uint8_t)length;
        break;
    default:
        out[0] = (uint8_t)(0xE0 | (length >> 24));
        out[1] = (uint8_t)(length >> 16);
        out[2] = (uint8_t)(length >> 8);
        out[3] = (uint8_t)length;
        break;
    }
}

bool prefix_holds(unsigned width, unsigned length)
{
    return width == 1 ? length < 0x80 : width == 2 ? length < 0x4000 : width == 3 ? length < 0x200000 : true;
}

unsigned narrowest(unsigned length)
{
    return length < 0x80 ? 1 : length < 0x4000 ? 2 : length < 0x200000 ? 3 : 4;
}

// the wire frame of an original: [L = 7 + n][type 0][flow, 3 bytes LE][PacketNum, 3 bytes LE][payload]
std::vector<uint8_t> frame_of(unsigned flow, unsigned num, const uint8_t* data, unsigned n)
{
    std::vector<uint8_t> f(4);
    const unsigned w = narrowest(7 + n);
    put_prefix(w, 7 + n, f.data());
    f.resize(w);
    f.push_back(0);
    for (unsigned k = 0; k < 3; ++k)
        f.push_back((uint8_t)(flow >> (8 * k)));
    for (unsigned k = 0; k < 3; ++k)
        f.push_back((uint8_t)(num >> (8 * k)));
    f.insert(f.end(), data, data + n);
    return f;
}

/// One call: a symbol of prefix width hs and length n (claimed: the prefix may
/// say more than the block holds) at offset `off` of a block that ends where
/// the readable bytes end, a row of exactly `stride` bytes.  fits: the row must
/// be the frame and a zero tail; otherwise zero with length 0.
void one(unsigned hs, unsigned n, unsigned off, uint32_t cap, uint64_t stride, bool fits, const char* what)
{
    const unsigned flow = 0xABCDEF - n % 1000, num = (0x3fffff - 17 * off - n) & 0x3fffff;
    const size_t readable = (size_t)hs + n < cap ? (size_t)hs + n : cap;
    uint8_t* block = (uint8_t*)std::malloc(off + readable);
    uint8_t* sym = block + off;
    std::vector<uint8_t> whole((size_t)hs + n);
    put_prefix(hs, n, whole.data());
    for (unsigned k = 0; k < n; ++k)
        whole[hs + k] = (uint8_t)(k * 131 + n + off + 1);
    std::memcpy(sym, whole.data(), readable);
    uint8_t* row = (uint8_t*)std::malloc((size_t)stride);
    std::memset(row, 0xA5, (size_t)stride);
    uint32_t len = 0xA5A5A5A5u;
    relay_row(sym, cap, flow, num, row, stride, &len);
    std::vector<uint8_t> want;
    if (fits)
        want = frame_of(flow, num, whole.data() + hs, n);
    if (len != want.size())
        fail(what, hs, n, off);
    else if (want.size() > stride || (!want.empty() && std::memcmp(row, want.data(), want.size()) != 0))
        fail(what, hs, n, off);
    else
        for (uint64_t b = want.size(); b < stride; ++b)
            if (row[b] != 0) {
                fail(what, hs, n, off);
                break;
            }
    std::free(row);
    std::free(block);
}

} // namespace

int main()
{
    // relay_cases.py EDGE_LENGTHS
    const unsigned lengths[] = {1,    2,    7,    8,    9,    120,  121,  127,  128,   129,   16376, 16377,
                                16383, 16384, 16385, 7,    8,    9,    1014, 1015, 1016,  8182,  8183,  8184};
    unsigned seen = 0;   // (hs, hf) pairs met, as bits
    unsigned calls = 0;
    for (unsigned hs = 1; hs <= 4; ++hs)
        for (unsigned off = 0; off < 16; ++off)
            for (unsigned n : lengths) {
                if (!prefix_holds(hs, n))
                    continue;
                const unsigned hf = narrowest(7 + n) + 7;
                if (hf != frame_header_bytes(kFrameOriginal, n))
                    fail("frame_header_bytes", hs, n, off);
                seen |= 1u << (4 * (hs - 1) + (hf - 8));
                const uint32_t cap = hs + n;
                const uint64_t total = (uint64_t)hf + n;
                one(hs, n, off, cap, total, true, "row filled to its last byte");
                one(hs, n, off, cap, (total + 15) & ~(uint64_t)15, true, "row of the next multiple of 16");
                one(hs, n, off, cap, total + 16400, true, "long zero tail");
                // a capacity past the symbol (a pending row's finalBytes): nothing past hs + n is read
                one(hs, n, off, cap + 5, total + 3, true, "capacity past the symbol");
                // the packets that do not fit
                one(hs, n, off, cap - 1, total + 16, false, "hs + n = cap + 1");
                one(hs, n, off, cap, total - 1, false, "hf + n = stride + 1");
                calls += 6;
            }
    for (unsigned hs = 1; hs <= 4; ++hs)
        for (unsigned off = 0; off < 16; ++off) {
            // a zero prefix of every width; a prefix the capacity cuts short
            one(hs, 0, off, hs, 32, false, "zero prefix");
            one(hs, 0, off, hs + 40, 32, false, "zero prefix, capacity to spare");
            if (hs > 1)
                one(hs, 100, off, hs - 1, 160, false, "prefix cut short by the capacity");
            calls += hs > 1 ? 3 : 2;
        }
    one(1, 5, 0, 0, 32, false, "capacity zero");
    // hs = 1: hf 8, 9; hs = 2: hf 8, 9, 10; hs = 3 and 4: hf 8, 9, 10
    const unsigned wantSeen = 0x3u | (0x7u << 4) | (0x7u << 8) | (0x7u << 12);
    if (seen != wantSeen) {
        std::printf("FAIL (hs, hf) pairs met: %#x, expected %#x\n", seen, wantSeen);
        ++g_failures;
    }
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("relay_row ok: %u calls\n", calls + 1);
    return 0;
}
