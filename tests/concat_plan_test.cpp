// concat_plan_test.cpp -- frames.h concat_plan and concat_copy alone: the plain
// C++ statement of what k_offsets and k_concat do for one job (ops.h
// ConcatJob), which the test double of the backend runs.  A stand-alone host
// program (tests/test_concat_plan.py builds it with
// -fsanitize=address,undefined): every symbol is a heap block that ends where
// its readable bytes end, the offsets, the records, the info record and the
// stream are heap blocks of exactly the bytes the calls may write, so a read or
// write outside the contract is a report.
//
// The expected offsets, info record and stream are worked out here by a walk of
// its own over the payloads.  The cases are those of stream_cases.py -- the
// short lengths and the prefix width steps, 1 / 63 / 64 / 65 / 129 small
// packets with the stop at item 0, 63, 64 and 128, an exact fit and one byte
// short, holes at position 0 and in the middle, count == 0 -- and the two this
// program alone can make: an invalid packet in every form (stop 1), and a
// running sum that passes 2^32 against a capacity below it.
#include "frames.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sgpu;

namespace {

int g_failures = 0;
unsigned g_jobs = 0;

void fail(const char* what, const char* why, long a = -1)
{
    if (++g_failures <= 20)
        std::printf("FAIL %s: %s %ld\n", what, why, a);
}

unsigned narrowest(unsigned length)
{
    return length < 0x80 ? 1 : length < 0x4000 ? 2 : length < 0x200000 ? 3 : 4;
}

void put_prefix(unsigned width, unsigned length, std::vector<uint8_t>& out)
{
    const uint8_t top[5] = {0, 0, 0x80, 0xC0, 0xE0};
    for (unsigned k = 0; k < width; ++k) {
        uint8_t b = (uint8_t)(length >> (8 * (width - 1 - k)));
        if (k == 0)
            b |= top[width];
        out.push_back(b);
    }
}

struct Packet
{
    long n;          // payload bytes; -1: absent; 0: a prefix of length zero (invalid)
    unsigned cut;    // bytes by which the capacity falls short of the symbol (invalid)
    unsigned width;  // prefix bytes; 0: the narrowest
    bool head;       // only the prefix exists: cap claims the payload, the block ends behind the prefix
};

Packet P(long n, unsigned cut = 0, unsigned width = 0)
{
    return Packet{n, cut, width, false};
}

/// One job: the packets as symbols, concat_plan, then concat_copy for every
/// record, into blocks of exactly the bytes owned.
void job(const std::vector<Packet>& pk, uint64_t capacity, const char* what)
{
    ++g_jobs;
    const uint32_t count = (uint32_t)pk.size();
    std::vector<uint8_t*> blocks(count, nullptr);
    std::vector<const uint8_t*> syms(count, nullptr);
    std::vector<uint32_t> caps(count, 0), hs(count, 0);
    std::vector<std::vector<uint8_t>> data(count);
    bool copy = true;   // every present payload exists (no `head` packet)
    for (uint32_t k = 0; k < count; ++k) {
        if (pk[k].n < 0)
            continue;
        const unsigned n = (unsigned)pk[k].n;
        std::vector<uint8_t> sym;
        hs[k] = pk[k].width ? pk[k].width : narrowest(n);
        put_prefix(hs[k], n, sym);
        if (pk[k].head) {
            copy = false;
            caps[k] = hs[k] + n;
        } else {
            data[k].resize(n);
            for (unsigned b = 0; b < n; ++b)
                data[k][b] = (uint8_t)(b * 131 + n + k + 1);
            sym.insert(sym.end(), data[k].begin(), data[k].end());
            caps[k] = (uint32_t)sym.size() - pk[k].cut;
        }
        const size_t have = pk[k].head ? sym.size() : caps[k];
        blocks[k] = (uint8_t*)std::malloc(have ? have : 1);
        std::memcpy(blocks[k], sym.data(), have);
        syms[k] = blocks[k];
    }
    // the expected sums
    uint32_t p = 0;
    while (p < count && pk[p].n >= 0)
        ++p;
    std::vector<uint32_t> wantOff(count + 1, 0);
    uint64_t off = 0;
    uint32_t d = 0, stop = 0;
    for (; d < p; ++d) {
        if (pk[d].n == 0 || pk[d].cut != 0) {
            stop = 1;
            break;
        }
        if (off + (uint64_t)pk[d].n > capacity) {
            stop = 2;
            break;
        }
        wantOff[d] = (uint32_t)off;
        off += (uint64_t)pk[d].n;
    }
    for (uint32_t k = d; k <= count; ++k)
        wantOff[k] = (uint32_t)off;
    if (off > 0xffffffffull)
        fail(what, "the case's own B does not fit 32 bits");

    uint32_t* offsets = (uint32_t*)std::malloc((size_t)(count + 1) * 4);
    ConcatRec* recs = (ConcatRec*)std::malloc(p ? p * sizeof(ConcatRec) : 1);
    uint32_t* info = (uint32_t*)std::malloc(16);
    std::memset(offsets, 0xA5, (size_t)(count + 1) * 4);
    std::memset(recs, 0xA5, p ? p * sizeof(ConcatRec) : 1);
    std::memset(info, 0xA5, 16);
    concat_plan(syms.data(), caps.data(), count, capacity, offsets, recs, info);

    const uint32_t wantInfo[4] = {d, (uint32_t)off, stop, p};
    for (unsigned i = 0; i < 4; ++i)
        if (info[i] != wantInfo[i])
            fail(what, "info word", i);
    for (uint32_t k = 0; k <= count; ++k)
        if (offsets[k] != wantOff[k])
            fail(what, "offset word", k);
    for (uint32_t k = 0; k < p; ++k) {
        const ConcatRec& r = recs[k];
        if (k < d) {
            if (r.off != wantOff[k] || r.n != (uint32_t)pk[k].n || r.hs != hs[k] || r.flags != kConcatWrite)
                fail(what, "record of a delivered packet", k);
        } else if (r.off | r.n | r.hs | r.flags)
            fail(what, "record behind the stop is not zero", k);
    }
    if (copy) {
        // the stream: exactly B bytes
        uint8_t* dst = (uint8_t*)std::malloc(off ? (size_t)off : 1);
        std::memset(dst, 0xA5, off ? (size_t)off : 1);
        for (uint32_t k = 0; k < p; ++k)
            concat_copy(syms[k], recs[k], dst);
        uint64_t at = 0;
        for (uint32_t k = 0; k < d; ++k) {
            if (std::memcmp(dst + at, data[k].data(), data[k].size()) != 0)
                fail(what, "payload in the stream", k);
            at += data[k].size();
        }
        if (at != off)
            fail(what, "the payloads' sum");
        std::free(dst);
    }
    std::free(offsets);
    std::free(recs);
    std::free(info);
    for (uint8_t* b : blocks)
        std::free(b);
}

uint64_t sum_of(const std::vector<Packet>& pk, size_t n)
{
    uint64_t s = 0;
    for (size_t k = 0; k < n; ++k)
        s += (uint64_t)pk[k].n;
    return s;
}

std::vector<Packet> smalls(unsigned n, unsigned seed)
{
    std::vector<Packet> pk;
    uint32_t x = seed * 2654435761u + 12345u;
    for (unsigned k = 0; k < n; ++k) {
        x = x * 1664525u + 1013904223u;
        pk.push_back(P(1 + (long)((x >> 16) % 40)));
    }
    return pk;
}

} // namespace

int main()
{
    // the short lengths and the prefix width steps
    {
        std::vector<Packet> pk;
        for (long n : {1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 16383, 16384, 16385, 8191, 8192, 8193})
            pk.push_back(P(n));
        job(pk, sum_of(pk, pk.size()), "edge lengths, exact fit");
        job(pk, 0xffffffffull, "edge lengths, the largest capacity");
        job(pk, 0, "edge lengths, no capacity");
        // (a prefix wider than the narrowest is valid: hs comes from the prefix)
        job({P(5, 0, 2), P(5, 0, 3), P(5, 0, 4), P(200, 0, 4)}, 215, "wide prefixes");
    }
    // the scan's pass edges, every stop
    for (unsigned n : {1u, 63u, 64u, 65u, 129u}) {
        const std::vector<Packet> pk = smalls(n, n);
        const uint64_t all = sum_of(pk, n);
        job(pk, all, "small packets, exact fit");
        job(pk, all - 1, "small packets, one byte short at the last");
        job(pk, all + 1000, "small packets, room to spare");
        for (unsigned j : {0u, 63u, 64u, 128u})
            if (j < n) {
                job(pk, sum_of(pk, j + 1) - 1, "small packets, one byte short at item j");
                job(pk, sum_of(pk, j + 1), "small packets, exact fit up to item j");
            }
    }
    // holes
    {
        std::vector<Packet> pk = smalls(10, 7);
        job({}, 100, "count == 0");
        job({}, 0, "count == 0, no capacity");
        pk[0].n = -1;
        job(pk, 1000, "a hole at position 0");
        pk = smalls(10, 8);
        pk[5].n = -1;
        job(pk, 1000, "a hole in the middle");
        job(pk, sum_of(pk, 3) - 1, "a hole in the middle behind a stop");
        pk[9].n = -1;
        job(pk, 1000, "two holes");
    }
    // stop 1: a length of zero, a payload past the capacity, a prefix cut short
    {
        std::vector<Packet> pk = smalls(70, 9);
        pk[66] = P(0);
        job(pk, 100000, "a zero length at item 66");
        pk[0] = P(0);
        job(pk, 100000, "a zero length at item 0");
        pk = smalls(70, 10);
        pk[64] = P(300, 1);   // (cap one byte short of prefix + payload)
        job(pk, 100000, "a payload past its symbol at item 64");
        pk = smalls(5, 11);
        pk[2] = P(300, 301);   // (cap = 1: of a two-byte prefix only the first byte may be read)
        job(pk, 100000, "a two-byte prefix with one readable byte");
        pk[2] = P(300, 302);   // (cap = 0)
        job(pk, 100000, "a symbol with no readable byte");
        pk[2] = P(20000, 20000, 3);   // (cap = 3: the prefix whole, no payload byte)
        job(pk, 100000, "a three-byte prefix and nothing behind it");
        // an invalid packet that would not fit either is invalid: stop 1 wins
        pk = smalls(5, 12);
        pk[3] = P(300, 1);
        job(pk, sum_of(pk, 3), "invalid and past the capacity");
    }
    // the running sum past 2^32: 9 packets of 2^29 - 1 bytes, of which only the
    // prefixes exist.  Eight fit 2^32 - 1; the ninth brings the sum to
    // 4831838199, which is 536870903 mod 2^32 and would fit a 32-bit sum.
    {
        std::vector<Packet> pk(9, Packet{(1l << 29) - 1, 0, 0, true});
        job(pk, 0xffffffffull, "nine packets of 2^29 - 1 against 2^32 - 1");
        job(pk, 8ull * ((1ull << 29) - 1), "eight packets of 2^29 - 1, exact fit");
        job(pk, 8ull * ((1ull << 29) - 1) - 1, "eight packets of 2^29 - 1, one byte short");
        job(pk, 1000, "packets of 2^29 - 1 against 1000 bytes");
        std::vector<Packet> mix = {P(100), Packet{(1l << 29) - 1, 0, 0, true}, P(7)};
        job(mix, 1000, "a 2^29 - 1 byte packet behind 100 bytes against 1000");
    }
    if (g_failures) {
        std::printf("%d failures in %u jobs\n", g_failures, g_jobs);
        return 1;
    }
    std::printf("concat_plan ok: %u jobs\n", g_jobs);
    return 0;
}
