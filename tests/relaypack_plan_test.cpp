// relaypack_plan_test.cpp -- frames.h pack_plan alone, and relay_row into the
// spans it gives: the plain C++ statement of what k_plan and k_pack do for one
// job (ops.h PackJob), which the test double of the backend runs.  A
// stand-alone host program (tests/test_relaypack_plan.py builds it with
// -fsanitize=address,undefined): every symbol is a heap block that ends where
// its readable bytes end, the records, the length words, the info record and
// the rows are heap blocks of exactly the bytes the call may write, so a read
// or write outside the contract is a report.
//
// The expected layout is worked out here by a walk of its own over the frame
// sizes, the expected rows from the payloads and a header built here.  The
// cases are those of relaypack_cases.py: the edge lengths at a stride that
// holds them all and at strides that turn the row after nearly every frame,
// off + T == stride and one byte more, T == stride, 63 / 64 / 65 / 129 small
// packets, absent packets and packets that do not fit, and too few rows
// (maxRows one short, maxRows == 0).
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

// the wire frame of an original: [L = 7 + n][type 0][flow, 3 bytes LE][PacketNum, 3 bytes LE][payload]
std::vector<uint8_t> frame_of(unsigned flow, unsigned num, const std::vector<uint8_t>& data)
{
    std::vector<uint8_t> f;
    put_prefix(narrowest(7 + (unsigned)data.size()), 7 + (unsigned)data.size(), f);
    f.push_back(0);
    for (unsigned k = 0; k < 3; ++k)
        f.push_back((uint8_t)(flow >> (8 * k)));
    for (unsigned k = 0; k < 3; ++k)
        f.push_back((uint8_t)(num >> (8 * k)));
    f.insert(f.end(), data.begin(), data.end());
    return f;
}

struct Packet
{
    int n;          // payload bytes; -1: absent
    unsigned cut;   // bytes by which the capacity falls short of the symbol (a packet that does not fit)
};

/// One job: the packets as symbols with the narrowest prefix, pack_plan, then
/// relay_row for every flagged record, into blocks of exactly the bytes owned.
void job(const std::vector<Packet>& pk, uint64_t stride, uint32_t maxRows, const char* what)
{
    ++g_jobs;
    const uint32_t count = (uint32_t)pk.size();
    const unsigned flow = 0xABCDEF - count, first = 0x3fff00;
    std::vector<uint8_t*> blocks(count, nullptr);
    std::vector<const uint8_t*> syms(count, nullptr);
    std::vector<uint32_t> caps(count, 0);
    std::vector<std::vector<uint8_t>> frames(count);   // empty: takes no space
    uint32_t unfit = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (pk[k].n < 0)
            continue;
        const unsigned n = (unsigned)pk[k].n;
        std::vector<uint8_t> data(n), sym;
        for (unsigned b = 0; b < n; ++b)
            data[b] = (uint8_t)(b * 131 + n + k + 1);
        put_prefix(narrowest(n), n, sym);
        sym.insert(sym.end(), data.begin(), data.end());
        caps[k] = (uint32_t)sym.size() - pk[k].cut;
        blocks[k] = (uint8_t*)std::malloc(caps[k] ? caps[k] : 1);
        std::memcpy(blocks[k], sym.data(), caps[k]);
        syms[k] = blocks[k];
        std::vector<uint8_t> f = frame_of(flow, (first + k) & 0x3fffff, data);
        if (n >= 1 && pk[k].cut == 0 && f.size() <= stride)
            frames[k] = f;
        else
            ++unfit;
    }
    // the expected layout
    struct At
    {
        uint64_t row, off;
    };
    std::vector<At> at(count);
    uint64_t row = 0, off = 0, nframes = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint64_t T = frames[k].size();
        if (!T)
            continue;
        if (off + T > stride) {
            ++row;
            off = 0;
        }
        at[k] = At{row, off};
        off = (off + T + 15) & ~(uint64_t)15;
        ++nframes;
    }
    const uint64_t need = nframes ? row + 1 : 0;
    const uint64_t live = need < maxRows ? need : maxRows;
    std::vector<std::vector<uint8_t>> wantRows(live, std::vector<uint8_t>((size_t)stride, 0));
    std::vector<uint32_t> wantLens(maxRows, 0);
    uint32_t written = 0;
    for (uint32_t k = 0; k < count; ++k)
        if (!frames[k].empty() && at[k].row < maxRows) {
            std::memcpy(wantRows[at[k].row].data() + at[k].off, frames[k].data(), frames[k].size());
            wantLens[at[k].row] = (uint32_t)(at[k].off + frames[k].size());
            ++written;
        }

    PlanRec* recs = (PlanRec*)std::malloc(count ? count * sizeof(PlanRec) : 1);
    uint32_t* lens = (uint32_t*)std::malloc(maxRows ? maxRows * 4 : 1);
    uint32_t* info = (uint32_t*)std::malloc(16);
    std::memset(recs, 0xA5, count * sizeof(PlanRec));
    std::memset(lens, 0xA5, (size_t)maxRows * 4);
    std::memset(info, 0xA5, 16);
    pack_plan(syms.data(), caps.data(), count, stride, maxRows, recs, lens, info);

    if (info[0] != need || info[1] != written || info[2] != unfit || info[3] != nframes - written)
        fail(what, "info record", info[0]);
    for (uint32_t r = 0; r < maxRows; ++r)
        if (lens[r] != wantLens[r])
            fail(what, "length word of row", r);
    // the rows: each a block of its own, written only through the records
    std::vector<uint8_t*> rows(live);
    for (uint64_t r = 0; r < live; ++r) {
        rows[r] = (uint8_t*)std::malloc((size_t)stride);
        std::memset(rows[r], 0xA5, (size_t)stride);
    }
    for (uint32_t k = 0; k < count; ++k) {
        const PlanRec& pr = recs[k];
        const bool frame = !frames[k].empty();
        if (!frame) {
            if (pr.row || pr.off16 || pr.span16 || pr.flags)
                fail(what, "record of an item that is no frame", k);
            continue;
        }
        if (pr.row != at[k].row || (uint64_t)pr.off16 * 16 != at[k].off)
            fail(what, "place of frame", k);
        if ((pr.flags & kPlanWrite) != (at[k].row < maxRows ? kPlanWrite : 0u) || (pr.flags & ~kPlanWrite))
            fail(what, "flags of frame", k);
        // the span: to the next frame of the row, or the row's end
        uint64_t end = stride;
        for (uint32_t j = k + 1; j < count; ++j)
            if (!frames[j].empty()) {
                if (at[j].row == at[k].row)
                    end = at[j].off;
                break;
            }
        if ((uint64_t)pr.span16 * 16 != end - at[k].off)
            fail(what, "span of frame", k);
        if ((pr.flags & kPlanWrite) && pr.row < live && (uint64_t)pr.off16 * 16 + (uint64_t)pr.span16 * 16 <= stride) {
            uint32_t lw = 0;
            relay_row(syms[k], caps[k], flow, (first + k) & 0x3fffff, rows[pr.row] + (uint64_t)pr.off16 * 16,
                      (uint64_t)pr.span16 * 16, &lw);
            if (lw != frames[k].size())
                fail(what, "relay_row's length of frame", k);
        }
    }
    for (uint64_t r = 0; r < live; ++r) {
        if (std::memcmp(rows[r], wantRows[r].data(), (size_t)stride) != 0)
            fail(what, "bytes of row", (long)r);
        std::free(rows[r]);
    }
    std::free(info);
    std::free(lens);
    std::free(recs);
    for (uint8_t* b : blocks)
        std::free(b);
}

std::vector<Packet> present(const std::vector<int>& lengths)
{
    std::vector<Packet> pk;
    for (int n : lengths)
        pk.push_back(Packet{n, 0});
    return pk;
}

uint64_t rows_needed(const std::vector<int>& lengths, uint64_t stride)
{
    uint64_t row = 0, off = 0;
    for (int n : lengths) {
        const uint64_t T = narrowest(7 + n) + 7 + n;
        if (off + T > stride) {
            ++row;
            off = 0;
        }
        off = (off + T + 15) & ~(uint64_t)15;
    }
    return lengths.empty() ? 0 : row + 1;
}

} // namespace

int main()
{
    // relay_cases.py EDGE_LENGTHS, and relaypack_cases.py EDGE_RANGES
    const std::vector<int> edge = {1,    2,    7,    8,    9,    120,  121,  127,  128,   129,   16376, 16377,
                                   16383, 16384, 16385, 7,    8,    9,    1014, 1015, 1016,  8182,  8183,  8184};
    job(present(edge), 16400, (uint32_t)rows_needed(edge, 16400) + 1, "edge lengths, stride 16400");
    const unsigned ranges[][3] = {{0, 10, 144}, {10, 5, 16400}, {15, 3, 32}, {18, 3, 1040}, {21, 3, 8208}};
    for (const auto& r : ranges) {
        const std::vector<int> part(edge.begin() + r[0], edge.begin() + r[0] + r[1]);
        job(present(part), r[2], (uint32_t)rows_needed(part, r[2]), "edge lengths, a row turn after nearly every frame");
    }
    // off + T == stride, one byte more, T == stride; a long frame at a non-zero offset
    job(present({100, 135, 100, 136, 247, 5}), 256, 5, "exact fits");
    job(present({100, 9000, 5000, 40}), 16400, 1, "a 9 KB frame at offset 112");
    // the plan's 64-item batches
    for (unsigned n : {63u, 64u, 65u, 129u}) {
        std::vector<int> small;
        for (unsigned k = 0; k < n; ++k)
            small.push_back(1 + (int)((k * 37 + n) % 40));
        const uint64_t need = rows_needed(small, 256);
        job(present(small), 256, (uint32_t)need + 1, "small packets");
        // too few rows
        job(present(small), 256, (uint32_t)need - 1, "small packets, one row short");
        job(present(small), 256, 0, "small packets, no rows");
    }
    // absent packets and packets that do not fit take no space
    {
        std::vector<Packet> pk = present({60, 67, 74, 81, 88, 95, 102, 109, 116, 123});
        pk[3].n = -1;
        pk[8].n = -1;
        job(pk, 256, 6, "two packets absent");
        pk[5].cut = 1;    // hs + n = cap + 1
        pk[6].n = 0;      // a zero prefix
        pk[9].n = 248;    // T = 257
        job(pk, 256, 6, "absent packets and three that do not fit");
        job(pk, 256, 1, "the same, one row");
        pk[0].cut = 61;   // capacity zero
        job(pk, 256, 6, "the same, the first with no capacity");
        for (Packet& p : pk)
            p.n = -1;
        job(pk, 256, 3, "nothing present");
        job(std::vector<Packet>(), 256, 3, "no items");
        job(std::vector<Packet>(), 256, 0, "no items, no rows");
    }
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("pack_plan ok: %u jobs\n", g_jobs);
    return 0;
}
