// ack_walk_test.cpp -- frames.h ack_walk and ack_head_valid alone: the plain
// C++ statement of what k_ackwalk does for one row (ops.h kRowTruncated), which
// the test double of the backend runs, and the record check
// sgpu_frames_recv_duplex makes before an acknowledgement reaches an encoder.  A
// stand-alone host program (tests/test_ack_walk.py builds it with
// -fsanitize=address,undefined): every row, every record array and every slot
// array is a heap block of exactly the bytes ack_walk may touch, so a read past
// row[0, stride) or a write past the records or the slots is a report.
//
// The expected records are written out here, field by field, for the smallest
// rows the walk can go wrong on; then the walk runs over rows with an ack at
// every offset behind an original and for every message length around a slot's
// size, against slices of the row.
#include "frames.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace sgpu;

namespace {

int g_failures = 0;

void check(bool ok, const char* what, unsigned a = 0, unsigned b = 0)
{
    if (!ok && ++g_failures <= 20)
        std::printf("FAIL %s (%u, %u)\n", what, a, b);
}

std::vector<uint8_t> ack_of(unsigned flow, const std::vector<uint8_t>& msg)
{
    // [L = 4 + n][type 2][flow, 3 bytes LE][message], L in the narrowest prefix
    const unsigned L = 4 + (unsigned)msg.size();
    std::vector<uint8_t> f;
    if (L < 0x80)
        f.push_back((uint8_t)L);
    else {
        f.push_back((uint8_t)(0x80 | (L >> 8)));
        f.push_back((uint8_t)L);
    }
    f.push_back(2);
    f.push_back((uint8_t)flow);
    f.push_back((uint8_t)(flow >> 8));
    f.push_back((uint8_t)(flow >> 16));
    f.insert(f.end(), msg.begin(), msg.end());
    return f;
}

std::vector<uint8_t> original_of(unsigned flow, unsigned num, unsigned n, uint8_t fill)
{
    std::vector<uint8_t> f = {(uint8_t)(7 + n), 0, (uint8_t)flow, (uint8_t)(flow >> 8), (uint8_t)(flow >> 16),
                              (uint8_t)num, (uint8_t)(num >> 8), (uint8_t)(num >> 16)};
    f.insert(f.end(), n, fill);
    return f;
}

std::vector<uint8_t> message(unsigned n, unsigned seed)
{
    std::vector<uint8_t> m(n);
    for (unsigned i = 0; i < n; ++i)
        m[i] = (uint8_t)(1 + (seed * 31 + i * 7) % 255);
    return m;
}

struct Walk
{
    uint32_t word;
    std::vector<PackedHead> recs;
    std::vector<uint8_t> slots;
};

// the walk over exact heap blocks: bytes[0, stride) is the row
Walk walk(const std::vector<uint8_t>& bytes, uint64_t stride, const uint32_t* len, uint32_t maxFrames, uint32_t ackSlots,
          uint32_t ackBytes)
{
    std::unique_ptr<uint8_t[]> row(new uint8_t[stride]);
    std::memset(row.get(), 0, stride);
    std::memcpy(row.get(), bytes.data(), bytes.size());
    std::unique_ptr<PackedHead[]> recs(new PackedHead[maxFrames]);
    std::unique_ptr<uint8_t[]> slots(new uint8_t[(size_t)ackSlots * ackBytes]);
    std::memset(recs.get(), 0xA5, maxFrames * sizeof(PackedHead));
    std::memset(slots.get(), 0xA5, (size_t)ackSlots * ackBytes);
    Walk w;
    w.word = ack_walk(row.get(), stride, len, maxFrames, ackSlots, ackBytes, recs.get(), slots.get());
    w.recs.assign(recs.get(), recs.get() + maxFrames);
    w.slots.assign(slots.get(), slots.get() + (size_t)ackSlots * ackBytes);
    return w;
}

bool is_zero(const void* p, size_t n)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i)
        if (b[i])
            return false;
    return true;
}

bool ack_rec(const PackedHead& r, unsigned offset, unsigned status, unsigned hdr, unsigned flow, unsigned nth,
             unsigned bytes)
{
    return r.offset == offset && r.status == status && r.type == kFrameAck && r.headerBytes == hdr && r.tailBytes == 0 &&
           r.flow == flow && r.packetNum == nth && r.dataBytes == bytes && is_zero(r.head, 4) && is_zero(r.tail, 8);
}

void smallest_rows()
{
    // stride 16, a 6-byte ack (a 1-byte message)
    {
        const std::vector<uint8_t> f = ack_of(0xAB, {0x05});
        const uint32_t len = 6;
        for (const uint32_t* lp : {&len, (const uint32_t*)nullptr}) {
            const Walk w = walk(f, 16, lp, 1, 1, 16);
            check(w.word == 1, "6-byte ack: row word", w.word);
            check(ack_rec(w.recs[0], 0, kRowOk, 5, 0xAB, 0, 1), "6-byte ack: record");
            check(w.slots[0] == 0x05 && is_zero(w.slots.data() + 1, 15), "6-byte ack: slot");
        }
    }
    // an ack that ends on the row's last byte
    {
        const std::vector<uint8_t> m = message(11, 1);
        const Walk w = walk(ack_of(9, m), 16, nullptr, 2, 1, 16);
        check(w.word == 1 && ack_rec(w.recs[0], 0, kRowOk, 5, 9, 0, 11), "ack to the row's last byte");
        check(std::memcmp(w.slots.data(), m.data(), 11) == 0 && is_zero(w.slots.data() + 11, 5), "its slot");
        check(is_zero(&w.recs[1], sizeof(PackedHead)), "the record behind it is zero");
    }
    // L = 4 (no message), L = 5, type 3
    {
        const Walk a = walk({4, 2, 1, 0, 0}, 16, nullptr, 2, 1, 16);
        check(a.word == kPackedMalformed && is_zero(a.recs.data(), 2 * sizeof(PackedHead)) &&
                  is_zero(a.slots.data(), 16),
              "L = 4 is malformed", a.word);
        const Walk b = walk({5, 2, 1, 0, 0, 0x33}, 16, nullptr, 2, 1, 16);
        check(b.word == 1 && ack_rec(b.recs[0], 0, kRowOk, 5, 1, 0, 1) && b.slots[0] == 0x33, "L = 5", b.word);
        const Walk c = walk({6, 3, 1, 0, 0, 1, 2}, 16, nullptr, 2, 1, 16);
        check(c.word == kPackedMalformed && is_zero(c.slots.data(), 16), "type 3 is malformed", c.word);
    }
    // length words: 0, stride, stride + 16
    {
        const std::vector<uint8_t> f = ack_of(1, {7, 8});
        uint32_t len = 0;
        Walk w = walk(f, 16, &len, 1, 1, 16);
        check(w.word == 0 && is_zero(w.recs.data(), sizeof(PackedHead)) && is_zero(w.slots.data(), 16), "length 0");
        len = 16;
        w = walk(f, 16, &len, 1, 1, 16);
        check(w.word == 1 && w.slots[0] == 7 && w.slots[1] == 8, "length = stride", w.word);
        len = 32;
        w = walk(f, 16, &len, 1, 1, 16);
        check(w.word == kPackedMalformed && is_zero(w.recs.data(), sizeof(PackedHead)) && is_zero(w.slots.data(), 16),
              "length = stride + 16", w.word);
        len = 6;   // the frame is 7 bytes: cut by its row's length
        w = walk(f, 16, &len, 1, 1, 16);
        check(w.word == kPackedMalformed && is_zero(w.slots.data(), 16), "a frame past the row's length", w.word);
    }
    // maxFrames 1 with bytes left; ackSlots 1 with two acks
    {
        std::vector<uint8_t> row = ack_of(1, {0x11});
        const std::vector<uint8_t> second = ack_of(2, {0x21, 0x22});
        row.insert(row.end(), second.begin(), second.end());
        const std::vector<uint8_t> orig = original_of(3, 77, 4, 0x5A);
        row.insert(row.end(), orig.begin(), orig.end());
        Walk w = walk(row, 32, nullptr, 1, 1, 16);
        check(w.word == (1 | kPackedMore), "maxFrames 1 with bytes left", w.word);
        w = walk(row, 32, nullptr, 3, 1, 16);
        check(w.word == (3 | kPackedAcksDropped), "two acks, one slot: row word", w.word);
        check(ack_rec(w.recs[0], 0, kRowOk, 5, 1, 0, 1) && ack_rec(w.recs[1], 6, kRowTruncated, 5, 2, 1, 2),
              "two acks, one slot: records");
        check(w.recs[2].type == kFrameOriginal && w.recs[2].status == kRowOk && w.recs[2].offset == 13 &&
                  w.recs[2].packetNum == 77 && w.recs[2].dataBytes == 4 && w.recs[2].headerBytes == 8,
              "the original behind the dropped ack is kept");
        check(w.slots[0] == 0x11 && is_zero(w.slots.data() + 1, 15), "two acks, one slot: the slot");
        w = walk(row, 32, nullptr, 3, 2, 16);
        check(w.word == 3 && w.recs[1].status == kRowOk && w.slots[16] == 0x21 && w.slots[17] == 0x22 &&
                  is_zero(w.slots.data() + 18, 14),
              "two acks, two slots", w.word);
    }
}

// an ack of every length around the slot size at every offset behind an original
void sweep(uint32_t ackBytes)
{
    const uint64_t stride = 2 * (uint64_t)ackBytes + 96;
    for (unsigned gap = 0; gap < 16; ++gap)
        for (unsigned n : {1u, ackBytes - 1, ackBytes, ackBytes + 1, ackBytes + 17}) {
            const std::vector<uint8_t> m = message(n, gap + n);
            std::vector<uint8_t> row = original_of(5, 1000 + gap, 9, 0x77);
            row.insert(row.end(), gap, 0);
            const unsigned at = (unsigned)row.size();
            const std::vector<uint8_t> f = ack_of(0x010203, m);
            row.insert(row.end(), f.begin(), f.end());
            const std::vector<uint8_t> last = original_of(5, 2000, 3, 0x66);
            const unsigned lastAt = (unsigned)row.size();
            row.insert(row.end(), last.begin(), last.end());
            const uint32_t len = (uint32_t)row.size();
            const Walk w = walk(row, stride, &len, 4, 1, ackBytes);
            const bool whole = n <= ackBytes;
            check(w.word == (3u | (whole ? 0u : kPackedAcksDropped)), "sweep: row word", gap, n);
            check(ack_rec(w.recs[1], at, whole ? kRowOk : kRowTruncated, (unsigned)f.size() - n, 0x010203, 0, n),
                  "sweep: ack record", gap, n);
            const unsigned copy = whole ? n : ackBytes;
            check(std::memcmp(w.slots.data(), m.data(), copy) == 0 && is_zero(w.slots.data() + copy, ackBytes - copy),
                  "sweep: slot", gap, n);
            check(w.recs[2].offset == lastAt && w.recs[2].packetNum == 2000 && w.recs[2].status == kRowOk,
                  "sweep: the frame behind the ack", gap, n);
            check(is_zero(&w.recs[3], sizeof(PackedHead)), "sweep: unused record", gap, n);
            // the record check recv_duplex makes
            check(ack_head_valid(w.recs[1], stride, 1, ackBytes, 0), "sweep: the scan's record is valid", gap, n);
        }
}

// rows without an ack: row_walk's records and word
void same_as_row_walk()
{
    std::vector<uint8_t> row = original_of(1, 2, 30, 0x10);
    row.insert(row.end(), 3, 0);
    const std::vector<uint8_t> rec = {(uint8_t)(4 + 12), 1, 9, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    row.insert(row.end(), rec.begin(), rec.end());
    for (uint32_t m : {1u, 2u, 3u}) {
        const Walk w = walk(row, 64, nullptr, m, 1, 16);
        std::unique_ptr<uint8_t[]> r(new uint8_t[64]);
        std::memset(r.get(), 0, 64);
        std::memcpy(r.get(), row.data(), row.size());
        std::vector<PackedHead> want(m);
        const uint32_t word = row_walk(r.get(), 64, nullptr, m, want.data());
        check(word == w.word && std::memcmp(want.data(), w.recs.data(), m * sizeof(PackedHead)) == 0,
              "a row without an ack: row_walk's output", m);
        check(is_zero(w.slots.data(), 16), "a row without an ack: zero slots", m);
    }
}

// records a scan cannot have produced
void forged()
{
    const Walk w = walk(ack_of(4, {1, 2, 3}), 32, nullptr, 1, 2, 16);
    const PackedHead good = w.recs[0];
    check(ack_head_valid(good, 32, 2, 16, 0), "the scan's own record");
    auto bad = [&](const char* what, void (*edit)(PackedHead&), uint32_t nth = 0, uint32_t slots = 2) {
        PackedHead r = good;
        edit(r);
        check(!ack_head_valid(r, 32, slots, 16, nth), what);
    };
    bad("type", [](PackedHead& r) { r.type = kFrameRecovery; });
    bad("status empty", [](PackedHead& r) { r.status = kRowEmpty; });
    bad("status malformed", [](PackedHead& r) { r.status = kRowMalformed; });
    bad("status 4", [](PackedHead& r) { r.status = 4; });
    bad("truncated with a whole message in a slot", [](PackedHead& r) { r.status = kRowTruncated; });
    bad("no message", [](PackedHead& r) { r.dataBytes = 0; });
    bad("ok but longer than the slot", [](PackedHead& r) { r.dataBytes = 17; });
    bad("header too short", [](PackedHead& r) { r.headerBytes = 4; });
    bad("header too long", [](PackedHead& r) { r.headerBytes = 9; });
    bad("a tail", [](PackedHead& r) { r.tailBytes = 1; });
    bad("head bytes", [](PackedHead& r) { r.head[3] = 1; });
    bad("tail bytes", [](PackedHead& r) { r.tail[7] = 1; });
    bad("flow", [](PackedHead& r) { r.flow = 1u << 24; });
    bad("past the stride", [](PackedHead& r) { r.offset = 25; });
    bad("offset overflow", [](PackedHead& r) { r.offset = 0xfffffffdu; });
    bad("not the nth ack", [](PackedHead& r) { r.packetNum = 1; });
    bad("nth ack of another count", [](PackedHead&) {}, 1);
    bad("ok without a slot", [](PackedHead&) {}, 0, 0);
    PackedHead t = good;   // what the scan writes for an ack past the slots, and for a long one
    t.status = kRowTruncated;
    t.packetNum = 2;
    check(ack_head_valid(t, 32, 2, 16, 2), "truncated: past the slots");
    t.packetNum = 0;
    t.dataBytes = 20;
    check(ack_head_valid(t, 32, 2, 16, 0), "truncated: longer than the slot");
}

} // namespace

int main()
{
    smallest_rows();
    sweep(16);
    sweep(1024);
    same_as_row_walk();
    forged();
    if (g_failures) {
        std::printf("ack_walk: %d failures\n", g_failures);
        return 1;
    }
    std::printf("ack_walk ok\n");
    return 0;
}
