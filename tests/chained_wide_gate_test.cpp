// tests/chained_wide_gate_test.cpp -- TEST ONLY (test_chained_wide_cpu.py).
//
// The k_ldpc gate (ops.h LdpcItem) on the hostsim backend: one submission's
// launches built by hand -- a chained matrix job, two wide rows' k_ldpc items
// (row 0 ungated, row 1 gated on the job's outcome word) and the executor
// segment whose two OP_ROWS ops read them (op 1 gated on the same word).
//
//   default  with SGPU_TEST_GE_FORCE_SINGULAR=1 (the hostsim hook) the job
//            reports outcome 0: the ungated row's L0 / L1 and result are what
//            they are when it runs alone, the gated row's destination and
//            scratch pair are untouched, and only the ungated picks count.
//   "open"   without the hook the job succeeds and both rows run.
//
// Linked with the hostsim backend (tools/backend_hostsim.cpp), gf.cpp
// and codedef.cpp.
#include "backend.h"
#include "codedef.h"
#include "gf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sgpu;

namespace {

constexpr uint32_t kElems = 512;     // window elements: ldpcN == kLdpcSplitMin
constexpr uint32_t kBytes = 96;      // symbol bytes (one k_ldpc tile, a tail past 96)
constexpr uint32_t kSpan = kLdpcTileBytes;
constexpr uint8_t kFill = 0xA5;      // "untouched"
constexpr uint32_t kMix = 3;

int fail(const char* what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}

uint8_t* dev(size_t bytes, int fill)
{
    uint8_t* p = static_cast<uint8_t*>(be_dev_alloc(bytes));
    std::memset(p, fill, bytes);
    return p;
}

struct Row
{
    uint32_t row;
    uint8_t* dst;       // kBytes (16-byte lanes)
    uint8_t* scratch;   // L0 at 0, L1 at kSpan
    uint32_t gate;
};

// L0 / L1 and the row's result, restated from the reference's draws
void expect(const Row& r, uint8_t* const* elems, uint8_t* l0, uint8_t* l1, uint8_t* out, uint64_t* bytes)
{
    std::memset(l0, 0, kBytes);
    std::memset(l1, 0, kBytes);
    Pcg32 prng;
    prng.seed(r.row, kElems);
    const uint32_t pairs = (kElems + kPairRate - 1) / kPairRate;
    for (uint32_t i = 0; i < 2 * pairs; ++i) {
        const uint8_t* e = elems[prng.next() % kElems];
        uint8_t* l = (i & 1) ? l1 : l0;
        for (uint32_t b = 0; b < kBytes; ++b)
            l[b] ^= e[b];
        *bytes += kBytes;
    }
    for (uint32_t b = 0; b < kBytes; ++b)
        out[b] = l0[b] ^ gf_mul(l1[b], (uint8_t)kMix);
}

} // namespace

int main(int argc, char** argv)
{
    const bool open = argc > 1 && !std::strcmp(argv[1], "open");
    const char* err = nullptr;
    if (!be_init(0, &err))
        return fail(err ? err : "be_init");

    // the window's elements
    std::vector<uint8_t*> elems(kElems);
    for (uint32_t e = 0; e < kElems; ++e) {
        elems[e] = dev(kBytes, 0);
        for (uint32_t b = 0; b < kBytes; ++b)
            elems[e][b] = (uint8_t)(e * 131u + b * 7u + (e >> 3));
    }

    // result words: the chained 1 x 1 job at word 0 (outcome at word 3)
    const uint32_t geWords = ge_result_words(1, 1, true);
    std::vector<uint32_t> results(geWords + 8, 0xdeadbeefu);
    const uint32_t okWord = 3;

    Row rows[2] = {{5, dev(kBytes + 16, kFill), dev(2 * kSpan, 0), 0},
                   {6, dev(kBytes + 16, kFill), dev(2 * kSpan, 0), 1 + okWord}};

    // the executor segment: two OP_ROWS ops of one wide row each
    const uint32_t E = kElems + 2;
    const uint32_t blockWords = kRowSums + E + kRowWords;
    std::vector<uint8_t> stream((size_t)2 * (kOpWords + blockWords) * 16, 0);
    LdpcItem items[2];
    uint32_t gates[2];
    uint8_t* w = stream.data();
    for (int k = 0; k < 2; ++k) {
        GfOp op;
        std::memset(&op, 0, sizeof(op));
        op.dst = kElems;   // (stageLo; no versioned rows)
        op.kind = OP_ROWS;
        op.n = 1;
        op.valid = E;
        op.mix = 0;
        op.termBegin = rows[k].gate;
        op.termCount = blockWords;
        std::memcpy(w, &op, sizeof(op));
        w += sizeof(op);
        WinEntry* win = reinterpret_cast<WinEntry*>(w) + kRowSums;   // (the 24 sums: none)
        for (uint32_t e = 0; e < kElems; ++e)
            win[e] = WinEntry{(uint64_t)(uintptr_t)elems[e], kBytes, e};
        win[kElems] = WinEntry{(uint64_t)(uintptr_t)rows[k].scratch, kBytes, 0};
        win[kElems + 1] = WinEntry{(uint64_t)(uintptr_t)rows[k].scratch + kSpan, kBytes, 0};
        RowItem r;
        std::memset(&r, 0, sizeof(r));
        r.dst = (uint64_t)(uintptr_t)rows[k].dst;
        r.n = kBytes;
        r.valid = 0;
        r.mask0 = kRowWide;
        r.mask1 = kMix << 24;
        r.row = rows[k].row;
        r.ldpcN = 0;
        r.ldpcOff = kElems;
        r.cutoff = E;
        std::memcpy(win + E, &r, sizeof(r));
        w += (size_t)blockWords * 16;

        LdpcItem& it = items[k];
        it.win = (uint64_t)(uintptr_t)win;
        it.dst = (uint64_t)(uintptr_t)rows[k].scratch;
        it.span = kSpan;
        it.n = kBytes;
        it.row = rows[k].row;
        it.N = kElems;
        it.off = 0;
        it.tileBase = 0;
        it.pair0 = 0;
        it.pair1 = (kElems + kPairRate - 1) / kPairRate;
        gates[k] = rows[k].gate;
    }
    const ExecItem ex{0, (uint32_t)(stream.size() / 16), 2, exec_tiles(0, 1)};

    // the chained job: a 1 x 1 parity matrix (not singular), its solve's row and coefficient
    GeDesc gd;
    std::memset(&gd, 0, sizeof(gd));
    gd.rows = gd.cols = 1;
    gd.flags = kGeChained;
    std::vector<uint8_t> geIn(ge_input_bytes(1, 1, 0), 0);
    GeRow* gr = reinterpret_cast<GeRow*>(geIn.data());
    gr->kind = GE_PARITY;
    gr->jEnd = 1;
    gr->colCount = 1;
    SolveRow srow;
    std::memset(&srow, 0, sizeof(srow));
    uint8_t coef = 0;

    // the submission: the job, then k_ldpc with the gate array, then k_exec
    uint64_t acct[4] = {0, 0, 0, 0};
    be_launch_ge(BeGe{&gd, geIn.data(), 1, results.data(), &srow, &srow, &coef, 1, 1}, GePlace::kCodecStream);
    be_join_ge();
    if (results[okWord] != (open ? 1u : 0u))
        return fail(open ? "the job did not succeed" : "the hook did not force outcome 0");
    be_launch_ldpc(items, 2, acct + 3, gates, results.data());
    be_launch_exec(stream.data(), &ex, 1, acct, results.data(), E);

    uint8_t l0[kBytes], l1[kBytes], out[kBytes];
    for (int k = 0; k < 2; ++k) {
        uint64_t bytes = 0;
        expect(rows[k], elems.data(), l0, l1, out, &bytes);
        const bool ran = k == 0 || open;
        if (ran) {
            if (std::memcmp(rows[k].scratch, l0, kBytes) || std::memcmp(rows[k].scratch + kSpan, l1, kBytes))
                return fail("L0 / L1 of a row that ran");
            if (std::memcmp(rows[k].dst, out, kBytes))
                return fail("result of a row that ran");
            for (uint32_t b = kBytes; b < kBytes + 16; ++b)
                if (rows[k].dst[b] != kFill)
                    return fail("bytes past the row");
            // (the zero tail of the scratch tile past the row's bytes)
            for (uint32_t b = kBytes; b < 2 * kSpan; ++b)
                if (b - (b >= kSpan ? kSpan : 0) >= kBytes && rows[k].scratch[b] != 0)
                    return fail("scratch past the row's bytes");
            acct[3] -= bytes;
        } else {
            for (uint32_t b = 0; b < 2 * kSpan; ++b)
                if (rows[k].scratch[b] != 0)
                    return fail("a gated-off item wrote its scratch");
            for (uint32_t b = 0; b < kBytes + 16; ++b)
                if (rows[k].dst[b] != kFill)
                    return fail("a gated-off row wrote its destination");
        }
    }
    if (acct[3] != 0)
        return fail("k_ldpc bytes: only the items that ran count, once");
    if (acct[0] != 0)
        return fail("executor bytes (wide rows' picks are counted by k_ldpc)");
    std::printf(open ? "open ok\n" : "gate ok\n");
    return 0;
}
